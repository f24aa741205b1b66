// zkp_internal.hpp — declarations shared by the kernel TU and the host prover.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "felt.hpp"
#include "pcg64.hpp"

// ---------------------------------------------------------------- profiling
// Every launch goes through Prof::begin/end; when enabled each launch is
// bracketed by HIP events recorded on the stream it runs on.
struct ProfRec {
  const char* name;
  double bytes;  // algorithmic (compulsory) HBM bytes of this launch
  hipEvent_t start, stop;
};
struct Prof {
  bool enabled = false;
  std::string only;   // non-empty: bracket only the launches of this name
  bool open = false;  // the current launch is bracketed
  std::vector<ProfRec> pending;
  std::vector<hipEvent_t> pool;
  hipEvent_t get_event();
  void begin(const char* name, hipStream_t s, double bytes);
  void end(hipStream_t s);
};

// A launch the kernels cannot take (a shape past their 32-bit offsets, a broken
// internal invariant): thrown as the calling entry point's ZKP_ERR_* status
// (prover.cpp), never an abort() across the C ABI.
[[noreturn]] void launch_fail(int code, const char* what);
// largest LDE domain (n * blowup) the NTT passes index with 32-bit element
// offsets, and the largest trace the OOD evaluation's block tree takes; entry
// points return ZKP_ERR_TRACE_SHAPE past them
constexpr uint32_t MAX_LOG_DOMAIN = 28, MAX_LOG_TRACE = 23;
// Load each kernel translation unit's gfx950 code object on the current device
// now (zkp_ctx_create) instead of at its first launch inside a proof: HIP loads
// a fat binary's code object lazily, on the first use of one of its kernels.
void preload_kernels_module();
void preload_merkle_module();
void preload_ntt_module();
// one empty launch on `s`: HIP binds a stream to a hardware queue at its first dispatch
void warm_stream(hipStream_t s);

// ---------------------------------------------------------------- NTT
// `dit` = bit-reversed in -> natural out (Cooley-Tukey); otherwise natural in ->
// bit-reversed out (Gentleman-Sande). The passes of a transform: ntt_plan.hpp.
struct NttBatch {
  const felt* src;     // batch b reads src + (b / src_div) * src_stride
  felt* dst;           // batch b writes dst + b * dst_stride
  const felt* scale;   // nullable; multiplies element p of batch b by scale[(b % scale_mod) * n + p] on load
  uint64_t src_stride, dst_stride;
  uint32_t src_div, scale_mod, batches;
};

// Full transform over `batches` arrays of size 2^logn using the stage-major
// twiddle table tw (level t at tw[2^t - 1 .. 2^(t+1) - 1) holds w_{2^(t+1)}^j;
// forward table for DIT, inverse table for DIF).
// only_pass >= 0: launch that pass of ntt_plan(logn, dit, batches) alone (the timing
// harness tests/native/kbench_ntt.cpp times the passes one by one; the library always
// runs the whole plan). The radix-2 path (n < 2^11) counts as pass 0.
void launch_ntt(Prof& prof, hipStream_t s, const NttBatch& b, uint32_t logn, bool dit, const felt* tw,
                uint32_t logN, int only_pass = -1);

// ---------------------------------------------------------------- tables
// fill levels 0..top-1 of a stage-major table whose level `top` is present
void launch_build_levels(Prof& prof, hipStream_t s, felt* tab, uint32_t top);
void launch_expand_powers(Prof& prof, hipStream_t s, felt* out, uint64_t count, const felt* lo_tab,
                          const felt* hi_tab);
// S[j*n + p] = ninv * (g * w_N^j)^rev(p)   (j < B; with g^-1 powers and the
// inverse table of a 2^logN domain this builds the inverse coset tables)
void launch_build_coset_scale(Prof& prof, hipStream_t s, felt* S, uint32_t logn, uint32_t B,
                              const felt* tw, uint32_t logN, const felt* glo, const felt* ghi, felt ninv);

// ---------------------------------------------------------------- hashing
// fused builders: leaves + all levels (nodes[1..2L), 8 words each) in ceil(log2(L)/9) launches;
// leaves L (= n*B) of a coset-major LDE matrix (cols x B x n), or the rows of a FRI layer
// (row r = [E[r + k*R] for k < F])
// Optional tree tail: with done (a zeroed per-stream counter) the launch that
// produces the top subtree roots also finishes the tree in its last block and,
// with coin_seed, runs the FRI coin step (seed <- H(seed || root), alpha_out,
// root_out). The launchers return true when the tail ran.
// op: what the last block does with the root (coin state in coin_seed):
//   MERKLE_TAIL_FRI_COIN    reseed, draw alpha -> alpha_out, root -> root_out
//   MERKLE_TAIL_DRAW_COEFFS reseed, draw ncoef composition coefficients -> out
//   MERKLE_TAIL_DRAW_Z      reseed, draw z -> out = (z, z wn), pw tables (logn each)
enum { MERKLE_TAIL_NONE = 0, MERKLE_TAIL_FRI_COIN = 1, MERKLE_TAIL_DRAW_COEFFS = 2, MERKLE_TAIL_DRAW_Z = 3 };
struct MerkleTail {
  uint32_t* done;
  uint32_t* coin_seed;
  felt* alpha_out;
  uint32_t* root_out;
  uint32_t op, method, ncoef, logn;
  felt wn;
  felt* out;
  felt* pw;
};
// The last composition column derived in the leaf pass instead of extended by an
// NTT. On an LDE coset j that is also a CE coset (ce == B), x^n = kappa_j is
// constant and H(x) = sum_c kappa_j^c H_c(x) (CompositionPoly splits H into C
// columns of n coefficients), so H_{C-1}(x) = (H(x) - sum_{c<C-1} kappa_j^c H_c(x))
// * kappa_j^-(C-1): C-1 products per row instead of one coset NTT per coset.
// H = the constraint evaluations (H[jl*n + t], coset jl of the source), kap[2*jl]
// = kappa, kap[2*jl+1] = kappa^-(C-1); the derived value is written to out[jl*n + t]
// (the source's column C-1) and hashed with the row.
struct LastCol {
  const felt* H;
  const felt* kap;
  felt* out;
};
// GlobalUpdate paired columns that are never materialized: the row hash derives
// column c >= wi as k*(lde_{c-d}[t] - lde_{c-d}[t-1]) + cval[c-d]*l0[q] (q = the
// row's index over the source's cosets, t-1 the previous row of its coset; see
// kernels.hip k_gu_lde), and launch_gu_fill writes them for the queried rows only
struct GuLazy {
  const felt* cval;
  const felt* l0;
  felt k;
  uint32_t d, wi, smallk;
};
bool launch_merkle_lde(Prof& prof, hipStream_t s, const felt* lde, uint32_t cols, uint32_t logB, uint64_t n,
                       uint32_t* nodes, uint64_t L, const MerkleTail* tail = nullptr, const LastCol* lc = nullptr,
                       const GuLazy* gl = nullptr);
// FRI layer tree over coset-major evaluations (B cosets of F*m16, m16 = m / F rows each): leaf r = j + B*t'
bool launch_merkle_fri(Prof& prof, hipStream_t s, const felt* E, uint64_t m16, uint32_t logB, uint32_t F,
                       uint32_t* nodes, const MerkleTail* tail = nullptr);
// nodes[1..L) from leaf digests already in nodes[L..2L)
bool merkle_upper(Prof& prof, hipStream_t s, uint32_t* nodes, uint64_t L, const MerkleTail* tail = nullptr);
// sharded commitments: hash the shard's rows (mode 0: LDE rows of cols columns;
// mode 1: FRI rows of 16) into per-destination blocks; then, after the
// all-to-all, rebuild the natural-order leaves of this rank's range and its subtree
// all-to-all in 2^logK chunks along the destination rows: launch_leaf_hash_shard hashes chunk k
void launch_leaf_hash_shard(Prof& prof, hipStream_t s, int mode, const felt* src, uint64_t n, uint32_t cols,
                            uint32_t logBl, uint32_t logrows, uint32_t logrr, uint32_t logK, uint32_t k,
                            uint32_t* send, const LastCol* lc = nullptr, const GuLazy* gl = nullptr);
// sharded tree tops (R <= 64 subtree roots, all-gathered) -> top[1..2R) on the device,
// then the tail's coin step on the root (tail nullable / MERKLE_TAIL_NONE: none)
void launch_shard_top(Prof& prof, hipStream_t s, const uint32_t* roots, uint32_t R, uint32_t* top,
                      const MerkleTail* tail);
void launch_merkle_from_shards(Prof& prof, hipStream_t s, const uint32_t* recv, uint32_t logB, uint32_t logrr,
                               uint32_t logK, uint32_t* nodes, uint32_t* done = nullptr);
constexpr uint32_t PACK_MAX = 16;
struct PackArgs {
  const void* src[PACK_MAX];
  uint64_t bytes[PACK_MAX], off[PACK_MAX];
  uint32_t n;
};
// dst[off[i] ..) = src[i][0 .. bytes[i]) for i < n (byte counts multiples of 4)
void launch_pack(Prof& prof, hipStream_t s, const PackArgs& a, void* dst);
// seed from host words, or (seed_words == nullptr) from the device coin state seed_dev
void launch_grind(Prof& prof, hipStream_t s, const uint32_t* seed_words, const uint32_t* seed_dev, uint64_t base,
                  uint64_t count, uint32_t bits, unsigned long long* result);
// remainder of a last FRI layer of D = m * 2^logB <= 256 values (coefficients
// rem_out[0..m)), commitment H(remainder) and the coin reseed with it (seed in place)
void launch_fri_remainder(Prof& prof, hipStream_t s, const felt* E, uint32_t logB, uint32_t m, felt off_inv,
                          felt wd_inv, felt d_inv, uint32_t* seed, felt* rem_out, uint32_t* commit_out);

// ---- device query tail (world 1): grinding to completion, query positions,
// and every opening of every possible batch proof (rows + full sibling paths)
void launch_grind_all(Prof& prof, hipStream_t s, const uint32_t* seed_dev, uint64_t base, uint64_t limit,
                      uint32_t bits, unsigned long long* result);
// raw DefaultRandomCoin::draw_integers(q, N, *nonce) from the device coin state
void launch_query_positions(Prof& prof, hipStream_t s, const uint32_t* seed_dev, const unsigned long long* nonce,
                            uint32_t q, uint64_t N, uint64_t* pos);
constexpr uint32_t GATHER_MAX_LAYERS = 16;
struct FullGatherArgs {
  const felt* tlde;      // w x B x n (coset-major)
  const felt* clde;      // C x B x n
  const uint32_t* tnodes;
  const uint32_t* cnodes;
  uint64_t n;
  uint32_t w, C, logB, logN, nlayers;
  uint32_t F;                               // values per FRI row (the folding factor)
  const felt* E[GATHER_MAX_LAYERS];         // FRI layer l evaluations, coset-major (m[l] per coset)
  const uint32_t* fnodes[GATHER_MAX_LAYERS];
  uint64_t m[GATHER_MAX_LAYERS];
  uint32_t logrows[GATHER_MAX_LAYERS];      // log2 of the layer's tree leaves (rows)
  uint64_t seg_off[GATHER_MAX_LAYERS + 1];  // words
  uint32_t rec_words[GATHER_MAX_LAYERS + 1];
};
// record of raw position i in segment 0: [w + C row felts | trace path | constraint path]
// (logN sibling digests each, leaf level first); segment 1 + l: [F felts | logrows[l] digests]
void launch_gather_full(Prof& prof, hipStream_t s, const FullGatherArgs& a, uint32_t q, const uint64_t* pos,
                        uint32_t* out);

// ---------------------------------------------------------------- device transcript
// (seed = 8 LE words of the DefaultRandomCoin state, in device memory)
// reseed with `root` (device), then draw `ncoef` composition coefficients into cc
void launch_dt_draw_coeffs(Prof& prof, hipStream_t s, uint32_t* seed, const uint32_t* root, uint32_t method,
                           uint32_t ncoef, felt* cc);
// coefficient-dependent constants of the eval kernels (layout in kernels.hip)
void launch_dt_eval_consts(Prof& prof, hipStream_t s, int air, const felt* cc, felt k, felt w_last, const felt* aval,
                           const felt* zinv, uint32_t ce, uint32_t w, uint32_t num_t, felt* out);
// OOD frame -> reseeds -> DEEP coefficients gamma (w + C) and dk[2..4) = kz, kzg
// (ood[2a + {0,1}] = array a at z, zg; dk[0..2) = z, zg already)
void launch_dt_deep_coeffs(Prof& prof, hipStream_t s, uint32_t* seed, const felt* ood, uint32_t w, uint32_t C,
                           uint32_t method, felt* gamma, felt* dk);
// reseed with the constraint root, draw z: zz = (z, z w_n), pw = z^(2^l) || (z w_n)^(2^l), l < logn
void launch_dt_draw_z(Prof& prof, hipStream_t s, uint32_t* seed, const uint32_t* root, felt wn, uint32_t logn,
                      felt* zz, felt* pw);

// ---------------------------------------------------------------- trace building
// GlobalUpdate trace (120 x n, column-major) from masked/raw global models (60 each),
// ndev x 60 local models and k^-1 (src/aggregation/prover.rs:98-160); tile_buf holds
// 60 * ceil(n / 4096) felts
void launch_gu_trace(Prof& prof, hipStream_t s, const felt* masked, const felt* raw, const felt* local,
                     uint64_t ndev, felt kinv, uint64_t n, felt* tile_buf, felt* out);
// TrainingUpdate traces of the K clients of a round (src/training/prover.rs:90-218), one
// shape (bs, n) for all. Client k's descriptor, read by the kernels through uniform loads:
struct TuClient {
  felt* out;              // its 240 x n column-major trace
  const uint64_t* masks;  // device: n x 120 row-major u64 masks, or null: the PCG64 stream below
  felt pr_inv, lr_inv;    // the inverses of its precision and learning rate
  pcg::u128 pcg_state;    // s_0 of the stream (pcg64.hpp): the mask of row t, cell c is value t * 120 + c
  pcg::u128 pcg_mul[pcg::JUMP_BITS], pcg_inc[pcg::JUMP_BITS];  // its doubled pairs
};
// states: K x (bs + 1) x 120 felts. launch_tu_states (bs > 0), one workgroup per client:
// row 0 = initial[k] (120 felts: [v, s] pairs, w row-major then b), rows 1..bs = the
// signed fixed-point SGD steps over batch[k] = [x (bs x 9) | x signs (bs x 9) | y (bs x 6)],
// ac_inv = the inverse of f64_to_felt(6.0). launch_tu_write: row t of client k's trace =
// [states[k][min(t, bs)] + mask_t | mask_t]; first_last (K x 240 felts) = the masked half
// of its row 0, then of its row n - 1
void launch_tu_states(Prof& prof, hipStream_t s, const TuClient* clients, uint32_t K, const felt* initial,
                      const felt* batch, felt* states, uint32_t bs, felt ac_inv);
void launch_tu_write(Prof& prof, hipStream_t s, const TuClient* clients, uint32_t K, const felt* states,
                     uint64_t bs, uint64_t n, felt* first_last);

// ---------------------------------------------------------------- constraints
// Points of a coset-major shard: local index q = c*n + t is cx[c] * w_n^t,
// cx[c] = g * w_N^(j of local coset c), twn = w_n^t for t < n/2 (the
// stage-major twiddle level logn-1, read contiguously).
struct PointMap {
  const felt* cx;
  const felt* twn;
  uint32_t logn;
};

// The shard evaluates the CE cosets u in [u0, u0 + cel) (CE coset u lives in
// LDE coset u * B/ce); its LDE matrices hold the cosets [j0, j0 + 2^logBl).
struct EvalCommon {
  uint32_t logn, logB, logce, logN;
  uint32_t u0, cel, j0, logBl;
  felt g, w_last;        // domain offset (3), w_n^(n-1)
  PointMap pm;           // x of the shard's CE points (cx per owned CE coset)
  const felt* zinv;      // ce entries: 1/(x^n - 1) on the CE domain (x^n = g^n * w_ce^s);
                         // for MiMC pre-multiplied by the transition coefficient
};
// MiMC: x' - (x + K)^7 ; boundary steps 0 and n-1 on column 0
struct MimcEvalArgs {
  const felt* bcoef;     // device: A, Bc, Cc, D of the regrouped boundary numerator (k_dt_eval_consts)
  const felt* kper;      // 64*ce periodic values on the CE domain
  felt* binv;            // scratch: one felt per 2048 CE points (per-block inverse products)
  felt* dinv;            // M felts: 1/((x - 1)(x - w^(n-1))) per CE point (domain-only, cached in the ctx)
  bool binv_ready;       // dinv already holds this domain's values
};
void launch_eval_mimc(Prof& prof, hipStream_t s, const EvalCommon& c, const MimcEvalArgs& a, const felt* lde,
                      felt* comp);
// linear AIRs (GlobalUpdate, TrainingUpdate): optional transition
// T = sum_c a_c*next_c + b_c*cur_c over Z_T; boundary group 0 at step b0
// (sum_c beta0_c*cur_c - bconst over x - w^b0) and optional group 1 at step b1.
// coefs = [a (width) | b (width) | beta0 (width) | beta1 (width)], width = columns read
struct LinearEvalArgs {
  uint32_t width;
  bool transition, two_groups;
  const felt* coefs;     // device: 4 * width coefficient rows, then bconst0, bconst1
  felt w_bstep, w_bstep1;
  felt* binv;            // scratch: one felt per 2048 CE points
  felt* dinv;            // M felts: the boundary divisor inverses per CE point (cached in the ctx)
  bool binv_ready;       // dinv already holds this domain's values
};
void launch_eval_linear(Prof& prof, hipStream_t s, const EvalCommon& c, const LinearEvalArgs& a, const felt* lde,
                        felt* comp);
// the same in coefficient form (kernels.hip, k_lin_lincomb): the coefficients of
// [A (trans) | B0 | B1 (two)] over bit-reversed positions [p0, p0 + np) of the
// first W coefficient columns (out: np felts per array; twn[j] = w_n^j, j < n/2),
// then, once they are extended to the shard's CE cosets (ev: cel*n per array),
// the per-point formula of k_eval_linear
// Small position ranges split the columns into lincomb_groups(np, W) groups
// (partial sums in `scratch`: 4 * np felts per group, nullable = one group).
uint32_t lincomb_groups(uint64_t np, uint32_t W);
void launch_lin_lincomb(Prof& prof, hipStream_t s, bool trans, bool two, const felt* coef, uint32_t W, uint32_t logn,
                        uint64_t p0, uint64_t np, const felt* coefs, const felt* twn, felt* out, felt* scratch);
void launch_eval_linear_pts(Prof& prof, hipStream_t s, const EvalCommon& c, const LinearEvalArgs& a, const felt* ev,
                            felt* comp);

// The fields of an op and of an operand (include/zkp.h zkp_air_program), for the host
// interpreter and validation (air_program.hpp) and the device interpreter (kernels.hip)
namespace airp {
constexpr uint32_t op_code(uint64_t op) { return (uint32_t)(op & 0xff); }
constexpr uint32_t op_dst(uint64_t op) { return (uint32_t)((op >> 8) & 0xff); }
constexpr uint32_t op_a(uint64_t op) { return (uint32_t)((op >> 16) & 0xffff); }
constexpr uint32_t op_b(uint64_t op) { return (uint32_t)((op >> 32) & 0xffff); }
constexpr uint32_t src_kind(uint32_t operand) { return operand >> 13; }
constexpr uint32_t src_index(uint32_t operand) { return operand & 0x1fff; }
}  // namespace airp

// A registered constraint program's code on the device, as the interpreter of kernels.hip
// (run_program) reads it; the host lays it out with ProgCodeLayout (prover_internal.hpp)
struct ProgPeriodic {
  uint32_t off, mask;    // column's table at per_tab + off, indexed by (periodic index & mask), mask = table length - 1
};
struct ProgCode {
  const uint64_t* ops;   // device: the op stream (read through uniform loads)
  uint32_t nops, nreg;
  const felt* consts;    // device: the constant pool
  const ProgPeriodic* per_desc;  // device: one per periodic column
  const felt* per_tab;   // device: the periodic columns' tables
  const felt* pub;       // device: the instance's public inputs (ZKP_SRC_PUB operands; uniform loads), or null
};
// A program over the CE domain (k_eval_program):
// the op stream runs once per CE point, T = sum_i cc[i] * t_i over Z_T, then per group
// of assertions that share a step sum_k cc[num_t + k] * (cur[col_k] - val_k) over (x - w^step).
constexpr uint32_t PROG_MAX_GROUPS = 4;  // ZKP_AIR_MAX_ASSERTION_STEPS
struct ProgEvalArgs {
  ProgCode code;         // periodic tables over the CE domain, indexed by the CE index (mask = cycle*ce - 1)
  uint32_t num_t, ngroups;
  const uint32_t* a_col; // device: assertion columns, sorted by (step, column)
  const felt* cc;        // device: num_t transition then the assertion coefficients
  const felt* a_val;     // device: assertion values
  uint64_t col_stride;   // felts between two columns of the trace LDE (Bl * n)
  uint32_t grp_end[PROG_MAX_GROUPS];   // assertions [grp_end[g-1], grp_end[g]) share a step
  felt w_step[PROG_MAX_GROUPS];        // w_n^step of the group
  felt* dinv[PROG_MAX_GROUPS];         // M felts each: 1/(x - w^step) per CE point (cached in the ctx)
  bool dinv_ready[PROG_MAX_GROUPS];
  felt* binv;            // scratch: one felt per 2048 CE points
};
// A program's strided assertions (include/zkp.h zkp_air_strided_assertion), in stored order
// (stride, first, column); a group shares (stride, first) and the divisor x^k - w_n^(first k),
// k = n / stride. k_eval_program_strided (eval_program<true>) adds, per group,
//   (sum_j cc_j * (cur[col_j] - val_j) - W_g[q]) * dtab_g[CE index & mask_g]
// after the single-step groups: val_j = 0 for a sequence, whose values enter through
// W_g = sum_j cc_j V_j (launch_strided_combine, then the coset NTT), null for a group of
// periodic assertions alone.
constexpr uint32_t PROG_MAX_STRIDED_GROUPS = 4;  // ZKP_AIR_MAX_STRIDED_GROUPS
struct ProgStridedArgs {
  uint32_t ngroups;
  uint32_t grp_end[PROG_MAX_STRIDED_GROUPS];  // strided assertions [grp_end[g-1], grp_end[g]) form group g
  uint32_t mask[PROG_MAX_STRIDED_GROUPS];     // stride * ce - 1
  const felt* dtab[PROG_MAX_STRIDED_GROUPS];  // stride * ce felts: 1/(x^k - w_n^(first k)) by CE index (cached in the ctx)
  const felt* W[PROG_MAX_STRIDED_GROUPS];     // cel * n felts: W_g over the shard's CE points, or null
  const uint32_t* col;   // device: the strided assertions' columns
  const felt* val;       // device: their values (zero for a sequence)
  const felt* cc;        // device: the coefficient of the first strided assertion
};
// `sa` (nullable): with strided groups the launch is k_eval_program_strided, the same body with them
void launch_eval_program(Prof& prof, hipStream_t s, const EvalCommon& c, const ProgEvalArgs& a, const felt* lde,
                         felt* comp, const ProgStridedArgs* sa = nullptr);
// table[s] = 1/(gk[0] * w_l^s - c0) for s < l = 2^logl (gk: one device felt, g^k; twl[j] = w_l^j,
// j < l/2): the phases of the single-step tables, one field inversion. scratch: l / 2048 + 1 felts
void launch_strided_den_table(Prof& prof, hipStream_t s, const felt* gk, const felt* twl, uint32_t logl, felt c0,
                              felt* scratch, felt* table);
// W_g's coefficient column for every group that holds a sequence (k_strided_combine):
// out[g * n + p] = sum_d cc[desc[d].cc] * tab[desc[d].off + rev(p)] for rev(p) < 2^logk[g], else 0
struct ProgSeq {
  uint32_t cc, off;      // a sequence: its coefficient cc[cc]; its 2^logk n-scaled, twisted coefficients at tab + off
};
struct ProgSeqArgs {
  uint32_t ngroups;                          // groups that hold a sequence
  uint32_t seq_end[PROG_MAX_STRIDED_GROUPS]; // sequences [seq_end[g-1], seq_end[g]) of desc belong to group g
  uint32_t logk[PROG_MAX_STRIDED_GROUPS];
  const ProgSeq* desc;   // device
  const felt* tab;       // device
  const felt* cc;        // device: the coefficient of the first strided assertion
};
void launch_strided_combine(Prof& prof, hipStream_t s, const ProgSeqArgs& a, uint32_t logn, felt* out);
// The sequences of a program with public inputs, interpolated per proof on the device. Sequence d
// holds k = 2^logk values at `off` in three buffers of the same layout:
//   gather: vals[off + i] = pub[pub1 - 1 + i] (bound), or raw[off + i] (a concrete sequence's values)
//   launch_ntt (natural in, bit-reversed out, inverse table): ntt[off + p] = k * c_rev(p)
//   twist:  tab[off + i] = ntt[off + rev(i)] * (n / k) * w_n^(-first i), what k_strided_combine reads
struct ProgPubSeq {
  uint32_t off, logk, first, pub1;
};
struct ProgPubSeqArgs {
  uint32_t nseq, logn;
  const ProgPubSeq* desc;  // device (uniform loads)
  const felt* pub;         // device: the pub table
  const felt* raw;         // device: the concrete sequences' values (the image)
  const felt* itwn;        // device: w_n^-j, j < n/2 (inverse twiddle level logn - 1)
};
// maxk: the longest sequence (the grid covers it for every sequence)
void launch_prog_seq_gather(Prof& prof, hipStream_t s, const ProgPubSeqArgs& a, uint64_t maxk, felt* vals);
void launch_prog_seq_twist(Prof& prof, hipStream_t s, const ProgPubSeqArgs& a, uint64_t maxk, const felt* ntt,
                           felt* tab);

// The natural trace T (column-major, width x n) against a registered program
// (k_check_program; zkp_air_check_trace_device): one frame per thread, then the
// assertions. res[0] (preset to UINT64_MAX) receives the minimum (row << 10) | constraint
// over the failing frames, res[1] the minimum (assertion index << 32) | row over the failing
// asserted cells (singles first, then the strided assertions, cell by cell).
struct ProgStridedCells {
  uint32_t col, first, stride, count;  // cells T[col][first + stride * i], i < count = n / stride
  uint32_t blk0, voff;   // first of its blocks among the strided ones; values at svals + voff, or 0xffffffff: val
  uint32_t pub1, pad;    // pub1 != 0 (a bound assertion): pub[pub1 - 1] periodic, pub[pub1 - 1 + i] a sequence's cell i
  felt val;
};
struct ProgCheckArgs {
  ProgCode code;         // periodic tables: the columns' raw values, indexed by the row (mask = cycle - 1)
  uint32_t nassert, frame_blocks;    // nassert: the singles; frame_blocks: set by the launcher
  uint32_t single_blocks, nstrided;  // single_blocks: set by the launcher
  const ProgStridedCells* sdesc;  // device: one per strided assertion, in stored order
  const felt* svals;     // device: the sequences' values
  const uint32_t* a_col; // device: assertion columns, steps and values in stored (step, column) order
  const uint32_t* a_step;
  const felt* a_val;
  uint64_t n;            // 2 <= n <= 2^MAX_LOG_TRACE
};
// strided_blocks: the blocks of the strided assertions (sum of ceil(count / 64))
void launch_check_program(Prof& prof, hipStream_t s, ProgCheckArgs a, uint32_t width, const felt* T,
                          unsigned long long* res, uint64_t strided_blocks = 0);

// The raw constraint values of a registered program over E = 2^logE cosets of the trace
// (k_program_columns; zkp_air_constraint_degrees_device): ext holds the columns extended
// coset-major (column c, coset j, row t at (c*E + j)*n + t), one point q = j*n + t per thread.
// EMIT i of the chunk [i0, i0 + K) stores its operand at out[(i - i0)*E*n + q]; no
// coefficients, divisor or assertions. code: periodic tables over the E*n domain, indexed by
// the natural index j + E*t (mask = cycle*E - 1), as ProgEvalArgs' over the CE domain.
constexpr uint64_t DEG_CHUNK_FELTS = 1ull << 22;  // K*E*n felts of a chunk stay within this (64 MiB) ...
constexpr uint32_t DEG_CHUNK_MAX = 128;           // ... K at least 1 and at most this
inline uint32_t degrees_chunk(uint64_t n, uint32_t E) {
  const uint64_t k = DEG_CHUNK_FELTS / (n * E);
  return k < 1 ? 1u : k > DEG_CHUNK_MAX ? DEG_CHUNK_MAX : (uint32_t)k;
}
void launch_program_columns(Prof& prof, hipStream_t s, const ProgCode& code, const felt* ext, uint32_t width,
                            uint32_t logn, uint32_t logE, uint32_t i0, uint32_t K, felt* out);
// deg[k] (signed, preset to -1) = the highest index of a non-zero coefficient of column k < K
// (k_column_degrees). Column k is E segments of n at coefs + k*E*n in the library's
// bit-reversed, n-scaled layout: position p of segment m holds coefficient m*n + rev(p).
void launch_column_degrees(Prof& prof, hipStream_t s, const felt* coefs, uint32_t logn, uint32_t logE, uint32_t K,
                           long long* deg);

// GlobalUpdate column pairing (kernels.hip): columns d+i from columns i < d for a
// trace whose transitions hold. check: rows [t0, t0 + 2^logtn) of pairs c0..c0+cw of
// the natural trace (*bad = 1 on a mismatch; row 0 gives c_i); coef: the derived
// coefficient columns at positions [p0, p0 + np) (itwn = the inverse w_n table
// level); lde: the derived LDE columns over Bl cosets (l0 = L_0 over those cosets,
// launch_l0_table)
// MiMC trace vs its transition and assertions (sets *bad on any failing row)
void launch_mimc_check(Prof& prof, hipStream_t s, const felt* T, uint64_t n, felt v0, felt v1, uint32_t* bad);
void launch_gu_check(Prof& prof, hipStream_t s, const felt* T, uint32_t d, uint32_t logn, felt k, uint32_t c0,
                     uint32_t cw, uint64_t t0, uint32_t logtn, felt* cval, uint32_t* bad);
void launch_gu_coef(Prof& prof, hipStream_t s, felt* coef, uint32_t d, uint32_t logn, felt k, const felt* itwn,
                    uint32_t c0, uint32_t cw, uint64_t p0, uint64_t np, const felt* cval);
void launch_gu_lde(Prof& prof, hipStream_t s, felt* lde, uint32_t d, uint32_t logn, uint32_t logBl, felt k,
                   uint32_t c0, uint32_t cw, const felt* cval, const felt* l0);
// scratch: l0_scratch_felts(count, logn) felts (block products + per-coset constants)
size_t l0_scratch_felts(uint64_t count, uint32_t logn);
void launch_l0_table(Prof& prof, hipStream_t s, const PointMap& pm, uint64_t count, felt ninv, felt* out,
                     felt* scratch);
// the lazy paired columns [wi, w) of the queried rows: pos = natural LDE indices
// (npos of them), the rows of cosets [j0, j0 + 2^logBl) held here are written
void launch_gu_fill(Prof& prof, hipStream_t s, felt* lde, uint32_t w, uint32_t logn, uint32_t logB, uint32_t j0,
                    uint32_t logBl, const uint64_t* pos, uint32_t npos, const GuLazy& gl);

// composition polynomial from CE-coset interpolations (see kernels.hip): for the
// bit-reversed positions [p0, p0 + nR), n * c_m = (sum_u Si_u * W_u * w_ce^-um) * g^-mn / ce;
// consts = [g^-mn / ce for m < C | w_ce^-k for k < ce/2] (ce in {2, 4, 8, 16}; 32 for
// zkp_air_constraint_degrees_device, which keeps all C = ce segments)
void launch_comp_dft(Prof& prof, hipStream_t s, const felt* recv, const uint32_t* blk, const felt* Si,
                     const felt* consts, uint32_t ce, uint32_t C, uint32_t logn, uint64_t p0, uint64_t nR, felt* out,
                     uint32_t* hi_flag = nullptr);

// OOD evaluation of bit-reversed arrays (arrays contiguous, stride n) at x0 and x1
// partial[(a * nblocks + b) * 2 + {0,1}] ; pw0/pw1 = x^(2^l) tables (logn entries, device)
// (arrays a >= ntwo at x0 only)
void launch_eval_bitrev(Prof& prof, hipStream_t s, const felt* arrays, uint32_t narrays, uint32_t ntwo, uint32_t logn,
                        const felt* pw0, const felt* pw1, felt* partial, felt ninv, felt* out);
// its two halves for a sharded proof: a rank evaluates the 2048-coefficient blocks
// [b0, b0 + nbl) of every array (partial[(a * nbl + b - b0) * 2 + k]); after the
// all-gather of those rank blocks the tail combines all n / 2048 of them
void launch_eval_bitrev_blocks(Prof& prof, hipStream_t s, const felt* arrays, uint32_t narrays, uint32_t ntwo,
                               uint32_t logn, const felt* pw0, const felt* pw1, uint32_t b0, uint32_t nbl,
                               felt* partial);
void launch_eval_bitrev_tail(Prof& prof, hipStream_t s, const felt* partial, uint32_t narrays, uint32_t logn,
                             uint32_t nbl, const felt* pw0, const felt* pw1, felt ninv, felt* out);

// DEEP composition over the LDE domain (natural order out)
struct DeepArgs {
  uint32_t w, C, logB, logn, logN;
  uint32_t j0, logBl;    // shard cosets [j0, j0 + 2^logBl); output coset-major
  const felt* tlde;      // w x Bl x n
  const felt* clde;      // C x Bl x n
  const felt* gamma;     // w + C
  const felt* dk;        // device: z, z*w_n, kz, kzg (drawn / formed on the device)
  felt g;
  const felt* inv;       // 1 / (x - z) of the shard's LDE points (launch_deep_denominators)
  felt ginv;             // w_n^-1: 1 / (x_t - z w_n) = ginv * inv[t - 1] within a coset
};
// The DEEP inverse table: table[q] = 1 / (x_q - z) over the `count` points of m
// (whole cosets, n >= 8), z = zz[0] and pw[l] = z^(2^l) on the device. The 8 points
// x0 w_8^i of a coset have the product z^8 - x0^8, so only the count/8 values
// 1 / (y - z^8) go through the three batch-inversion phases, over m8 = the 8th
// powers of m's points (cx^8, the w_{n/8} table, logn - 3), and one expansion pass
// makes 8 inverses from each. The phases leave those values scaled by their total
// product T and invert nothing; the one field inversion, of T in closed form, runs
// on s2 beside them (s2 must already be ordered after z; ev joins it to s before
// the expansion). scratch: deep_den_scratch(count) felts.
struct DeepRoots {
  felt w8, w8_2, w8_3;   // w_8 = w_n^(n/8), its square and cube
};
inline uint64_t deep_den_scratch(uint64_t count) { return count / 8 + count / (8 * 2048) + 2; }
void launch_deep_denominators(Prof& prof, hipStream_t s, hipStream_t s2, hipEvent_t ev, const PointMap& m,
                              const PointMap& m8, const DeepRoots& r, uint64_t count, const felt* zz, const felt* pw,
                              felt* scratch, felt* table);
void launch_deep(Prof& prof, hipStream_t s, const DeepArgs& a, felt* out);
// coefficient-form DEEP for wide traces (winterfell combines the trace polynomials
// before extending): out[p] = sum_{c < w} gamma[c] * coef[c*n + p]
// over the bit-reversed, n-scaled coefficient columns -> one combined column (same layout)
void launch_deep_lincomb(Prof& prof, hipStream_t s, const felt* coef, uint32_t w, uint64_t n, uint64_t p0,
                         uint64_t np, const felt* gamma, felt* out,  // positions [p0, p0 + np) -> out[0, np)
                         felt* scratch);  // column-group partials (np per group, see lincomb_groups), nullable

// FRI fold-by-F (F = 2, 4, 8, 16) over coset-major evaluations of the cosets [j0, j0+Bl)
// (F*m16 positions each, m16 = m / F): natural row r = j + B*t', x_r = off * w_D^r; alpha
// read from device; eps_inv_dev = fold_constants
void launch_fri_fold(Prof& prof, hipStream_t s, const felt* E, uint64_t m16, uint32_t Bl, uint32_t j0,
                     uint32_t logB, uint32_t F, const felt* alpha, felt off_inv, const felt* itw, uint32_t logD,
                     const felt* eps_inv_dev, felt* out);
// the FRI tail in one block (world 1): layers of <= 128 rows (tree, coin step,
// fold) and the remainder, in order. Folding by 2 has up to 7 such layers (128 .. 2 rows).
constexpr uint32_t FRI_TAIL_MAX = 7;
struct FriTailLayer {
  const felt* E;        // layer evaluations, coset-major (B cosets of F * 2^logm16)
  uint32_t* nodes;      // the layer's tree (16 * rows words)
  uint32_t logm16;      // log2 of the rows per coset (m / F)
  felt off_inv;
  const felt* lev;      // w_D^-r table of the layer's domain
  felt* out;            // folded evaluations (the next layer)
  felt* alpha_out;      // device transcript slots
  uint32_t* root_out;
};
struct FriTailArgs {
  uint32_t nl, logB, F;
  FriTailLayer ly[FRI_TAIL_MAX];
  uint32_t* coin_seed;
  const felt* eps_inv;
  const felt* rem_E;    // last layer: rem_m positions per coset
  uint32_t rem_m;
  felt rem_off_inv, wd_inv, d_inv;
  felt* rem_out;
  uint32_t* commit_out;
};
void launch_fri_tail(Prof& prof, hipStream_t s, const FriTailArgs& a);
// device-side coin step of the FRI loop: seed = merge(seed, root); *alpha_out = draw(); root copied to root_out
void launch_coin_fri_layer(Prof& prof, hipStream_t s, uint32_t* seed, const uint32_t* root, felt* alpha_out,
                           uint32_t* root_out);

// gathers for query openings
struct GatherSeg {
  const void* src;
  uint64_t idx_off, count, out_off;  // out_off in 32-bit words
  uint32_t words;                    // 4 (felt) or 8 (digest)
  uint32_t pad;
};
void launch_gather_multi(Prof& prof, hipStream_t s, const GatherSeg* segs, uint32_t nseg, uint64_t max_count,
                         const uint64_t* idx, uint32_t* out, double bytes);
void launch_gather_felts(Prof& prof, hipStream_t s, const felt* src, const uint64_t* idx, felt* out, uint64_t count);
void launch_gather_digests(Prof& prof, hipStream_t s, const uint32_t* nodes, const uint64_t* idx, uint32_t* out,
                           uint64_t count);
