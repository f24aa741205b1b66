// prover_stages.cpp — the stage helpers of a proof (prover_internal.hpp): row
// commitments, the OOD evaluation, constraint evaluation, the composition constants,
// DEEP, and the query openings. World-1 paths; the sharded parts of the commitment
// and the OOD are in prover_shard.cpp.
#include "prover_internal.hpp"

using namespace zkpi;

namespace zkpi {

// commit the rows of a coset-major source held by this rank (cosets [j0, j0+Bl)):
// mode 0 = LDE rows (cols columns, n rows per coset), mode 1 = FRI rows (cols =
// folding factor values, 2^logrows rows per coset). Unsharded sources hold all B cosets.
// Unsharded trees finish in the last block of their top launch (MerkleTail);
// sharded trees in k_shard_top over the all-gathered subtree roots. With coin
// (coefficients, z or a FRI layer's alpha) that block also runs the coin step,
// and the function returns true when it did.
bool commit_rows(zkp_ctx* ctx, zkp_comm* cm, int mode, const felt* src, uint64_t n, uint32_t cols, uint32_t logB,
                 uint32_t logrows, bool sharded, const std::string& name, TreeShard& tr, uint8_t root[32],
                 bool fetch_root, const MerkleTail* coin, const LastCol* lc, const GuLazy* gl) {
  Prof& pf = ctx->prof;
  hipStream_t st = ctx->stream;
  const uint64_t L = 1ull << (logB + logrows);
  if (!sharded) {
    tr.logR = 0;
    tr.Lr = L;
    tr.nodes = ctx->buf<uint32_t>(name, (size_t)16 * L);
    uint32_t* done = ctx->buf<uint32_t>("merkle_done", 1);
    if (!ctx->have_cached("merkle_done")) HIP_CHECK(hipMemsetAsync(done, 0, 4, st));
    MerkleTail tail = coin ? *coin : MerkleTail{};
    tail.done = done;
    bool ran = mode == 0 ? launch_merkle_lde(pf, st, src, cols, logB, n, tr.nodes, L, &tail, lc, gl)
                         : launch_merkle_fri(pf, st, src, 1ull << logrows, logB, cols, tr.nodes, &tail);
    tr.top.assign(2, {});
    if (fetch_root) {  // otherwise the caller reads nodes[1] later
      ctx->download(root, tr.nodes + 8, 32);
      memcpy(tr.top[1].data(), root, 32);
    }
    return ran && coin;
  }
  return commit_rows_sharded(ctx, cm, mode, src, n, cols, logB, logrows, name, tr, root, fetch_root, coin, lc, gl);
}

// device -> host copies of one round trip (one sync)
void fetch_all(zkp_ctx* ctx, const std::vector<Fetch>& fs) {
  size_t tot = 0;
  for (const Fetch& f : fs) tot += (f.bytes + 15) & ~(size_t)15;
  uint8_t* hp = (uint8_t*)ctx->pinned(tot + 16);
  uint8_t* stage = ctx->buf<uint8_t>("fetch_stage", tot + 16);
  // pack the segments on the device (k_pack, PACK_MAX per launch), then one D2H copy
  size_t o = 0;
  PackArgs pa{};
  auto flush = [&] {
    if (pa.n) launch_pack(ctx->prof, ctx->stream, pa, stage);
    pa.n = 0;
  };
  for (const Fetch& f : fs) {
    if (f.bytes % 4) throw ZkpFail{ZKP_ERR_ARGUMENT, "fetch of a non-word-sized segment"};
    if (f.bytes) {
      pa.src[pa.n] = f.dev;
      pa.bytes[pa.n] = f.bytes;
      pa.off[pa.n] = o;
      if (++pa.n == PACK_MAX) flush();
    }
    o += (f.bytes + 15) & ~(size_t)15;
  }
  flush();
  HIP_CHECK(hipMemcpyAsync(hp, stage, tot, hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  o = 0;
  for (const Fetch& f : fs) {
    memcpy(f.host, hp + o, f.bytes);
    o += (f.bytes + 15) & ~(size_t)15;
  }
}

// OOD values of bit-reversed arrays at the two points whose power tables
// dpw[0..logn) / dpw[logn..2logn) are in device memory; returns the device
// array ood[2a + {0,1}] (array a at the two points; arrays a >= ntwo at the
// first point only, their second entry is zero)
// Sharded (cm world R > 1, at least R blocks of 2048 coefficients): each rank
// evaluates 1/R of every array's blocks (the partial Horner sums of SURVEY
// §8(e)(4)), the rank blocks are all-gathered (narrays * nb * 32 bytes in all)
// and every rank combines them: the same values as one rank evaluating it all.
felt* ood_launch(zkp_ctx* ctx, const felt* arrays, uint32_t narrays, uint32_t ntwo, uint32_t logn,
                 const felt* dpw, zkp_comm* cm) {
  uint32_t logE = logn < 11 ? logn : 11;
  if (logn - logE > 12) throw ZkpFail{ZKP_ERR_TRACE_SHAPE, "OOD evaluation supports n <= 2^23"};
  const uint32_t nb = 1u << (logn - logE);
  felt* part = ctx->buf<felt>("ood_part", (size_t)2 * narrays * nb);
  felt* dv = ctx->buf<felt>("ood_vals", (size_t)2 * narrays);
  const felt ninv = inv(felt_u64(1ull << logn));
  const uint32_t R = cm ? (uint32_t)cm->world : 1u;
  if (R == 1 || nb < R) {
    launch_eval_bitrev(ctx->prof, ctx->stream, arrays, narrays, ntwo, logn, dpw, dpw + logn, part, ninv, dv);
    return dv;
  }
  return ood_launch_sharded(ctx, arrays, narrays, ntwo, logn, dpw, cm, part, dv);
}

// Domain points of every LDE coset j (g*w_N^j, entries [0, B)) and CE coset u
// (g*w_M^u, entries [B, B+ce)); domain-only, cached per (n, B, ce).
felt* coset_points(zkp_ctx* ctx, uint32_t logn, uint32_t logB, uint32_t logce) {
  const uint32_t B = 1u << logB, ce = 1u << logce;
  const std::string cxkey = "coset_x_" + std::to_string(logn) + "_" + std::to_string(logB) + "_" +
                            std::to_string(logce);
  felt* cx = ctx->buf<felt>(cxkey, B + ce);
  if (!ctx->have_cached(cxkey)) {
    std::vector<felt> h(B + ce);
    const felt g = felt_u64(3);
    felt wN = root_of_unity(logn + logB), wM = root_of_unity(logn + logce);
    for (uint32_t j = 0; j < B; j++) h[j] = mul(g, pow_u64(wN, j));
    for (uint32_t u = 0; u < ce; u++) h[B + u] = mul(g, pow_u64(wM, u));
    ctx->upload(cx, h.data(), h.size() * 16);
  }
  return cx;
}

// (g*w_N^j)^8 of every LDE coset j: the coset offsets of the 8th powers of the LDE
// points, over which the DEEP inverse table is seeded; domain-only, cached per (n, B).
const felt* coset_points8(zkp_ctx* ctx, uint32_t logn, uint32_t logB) {
  const uint32_t B = 1u << logB;
  const std::string key = "coset_x8_" + std::to_string(logn) + "_" + std::to_string(logB);
  felt* cx8 = ctx->buf<felt>(key, B);
  if (!ctx->have_cached(key)) {
    std::vector<felt> h(B);
    const felt g8 = pow_u64(felt_u64(3), 8), wN8 = pow_u64(root_of_unity(logn + logB), 8);
    for (uint32_t j = 0; j < B; j++) h[j] = mul(g8, pow_u64(wN8, j));
    ctx->upload(cx8, h.data(), h.size() * 16);
  }
  return cx8;
}

// w_n^-1 for n = 2^logn (host, computed once)
felt deep_ginv(uint32_t logn) {
  static const std::vector<felt> tab = [] {
    std::vector<felt> t(MAX_LOG_TRACE + 1);
    for (uint32_t l = 0; l <= MAX_LOG_TRACE; l++) t[l] = inv(root_of_unity(l));
    return t;
  }();
  return tab[logn];
}

// DefaultConstraintEvaluator::evaluate over the CE cosets [u0, u0 + cel) held by
// this rank (its LDE cosets are [j0, j0 + 2^logBl)): composition evaluations
// comp[ul * n + t] = H(g * w_M^(u0+ul) * w_n^t), i.e. CE domain index (u0+ul) + ce*t.
// dt_cc = the composition coefficients (device; transition then boundary).
// Linear AIRs (GlobalUpdate, TrainingUpdate) evaluate in coefficient form when
// `coef` (the trace coefficient columns) is given (k_lin_lincomb): sharded, every
// rank of `cm` combines 1/R of the positions and the combined columns are
// all-gathered, so every rank calls this, with or without CE cosets (cel = 0).
// ZKP_EVAL_POINTWISE=1 (A/B switch) keeps k_eval_linear over the trace LDE.
void constraint_eval(zkp_ctx* ctx, const AirDesc& air, uint32_t logn, uint32_t logB, uint32_t logce, uint32_t u0,
                     uint32_t cel, uint32_t j0, uint32_t logBl, const felt* cx, const felt* twn, const felt* dt_cc,
                     const felt* dt_aval, const felt* tlde, felt* comp, const felt* coef, zkp_comm* cm) {
  Prof& pf = ctx->prof;
  hipStream_t st = ctx->stream;
  const uint32_t B = 1u << logB, ce = 1u << logce, logN = logn + logB, w = air.w;
  const uint64_t n = 1ull << logn;
  const felt g = felt_u64(3);
  felt wn = root_of_unity(logn);
  EvalCommon ec;
  ec.logn = logn; ec.logB = logB; ec.logce = logce; ec.logN = logN;
  ec.u0 = u0; ec.cel = cel; ec.j0 = j0; ec.logBl = logBl;
  ec.g = g;
  ec.w_last = pow_u64(wn, n - 1);
  ec.pm = PointMap{cx + B + u0, twn, logn};
  // 1/(x^n - 1) on the CE domain: x^n = g^n * w_ce^s (domain-only: cached per (n, ce))
  const std::string zkey = "zinv_" + std::to_string(logn) + "_" + std::to_string(logce);
  std::vector<felt>& zinv = ctx->host_cache[zkey];
  if (zinv.empty()) {
    zinv.resize(ce);
    felt gn = pow_u64(g, n), wce = root_of_unity(logce);
    for (uint32_t s = 0; s < ce; s++) zinv[s] = inv(sub(mul(gn, pow_u64(wce, s)), one()));
  }
  felt* dz = ctx->buf<felt>(zkey, ce);
  if (!ctx->have_cached(zkey)) ctx->upload(dz, zinv.data(), ce * 16);
  const std::string dom = std::to_string(logn) + "_" + std::to_string(logB) + "_" + std::to_string(u0) + "_" +
                          std::to_string(cel);
  // the coset-scale rows of the CE cosets (LDE cosets u * B/ce), gathered into one table per
  // (n, B, ce), cached: what extends a coefficient column to the CE cosets
  auto sce_rows = [&]() -> const felt* {
    const uint32_t cstep = logB - logce;
    const felt* S = ctx->S(logn, logB);
    if (!cstep) return S;
    const std::string skey = "Sce_" + std::to_string(logn) + "_" + std::to_string(logB) + "_" + std::to_string(logce);
    felt* t = ctx->buf<felt>(skey, (size_t)ce * n);
    if (!ctx->have_cached(skey))
      HIP_CHECK(hipMemcpy2DAsync(t, n * 16, S, (n << cstep) * 16, n * 16, ce, hipMemcpyDeviceToDevice, st));
    return t;
  };
  if (air.prog) {
    // a registered constraint program: k_eval_program reads the coefficients from dt_cc as drawn
    if (!cel) return;
    const airp::Program& pr = *air.prog;
    // the program's device image, in 16-byte units: the code sections (ProgCodeLayout), then
    // the assertion columns. A context keeps one image, the last
    // (id, n, ce) it evaluated (ids are never reused): proving another instance replaces it,
    // so registering and freeing ids does not grow the context.
    // Periodic column of cycle c over the CE domain: interpolate over <w_c>, evaluate at
    // g^(n/c) * <w_{c ce}> (as kper_* below), indexed by the CE index mod c*ce.
    const ProgCodeLayout lay(pr, ce);
    // Strided assertions append [columns | values | sequence descriptors | sequence tables]:
    // per sequence the k coefficients of V_j, interpolated over <w_k>, twisted by
    // w_n^(-first i) and multiplied by n (the coefficient layout k_strided_combine writes).
    // With public inputs (zkp_air_register_params; pr is the instance) the image holds no value of
    // pub and is shared by every instance of the id: the sequence tables section holds the concrete
    // sequences' raw values, a section of ProgPubSeq descriptors follows it, and the periodic
    // assertions' values and the sequences' coefficients are per-proof device arrays (below).
    const bool params = pr.num_pub != 0;
    const std::vector<airp::Strided>& sv = pr.strided;
    const size_t S = sv.size();
    size_t nseq = 0, seq_felts = 0;
    for (const airp::Strided& a : sv)
      if (a.sequence()) nseq++, seq_felts += a.nvals;
    const size_t o_col = lay.end(), o_scol = o_col + (pr.a_col.size() + 3) / 4, o_sval = o_scol + (S + 3) / 4,
                 o_sdesc = o_sval + S, o_stab = o_sdesc + (nseq + 1) / 2, o_pseq = o_stab + seq_felts,
                 total = o_pseq + (params ? nseq : 0);
    felt* dimg = ctx->buf<felt>("prog_image", total);
    std::vector<felt>& img = ctx->host_cache["prog_image"];  // kept: a large image is copied from it asynchronously
    std::vector<felt>& tag = ctx->host_cache["prog_image_tag"];
    const felt want[2] = {make((uint64_t)air.id, logn), make(logce, total)};
    if (tag.size() != 2 || !eq(tag[0], want[0]) || !eq(tag[1], want[1])) {
      const auto img_t0 = std::chrono::steady_clock::now();
      tag.clear();
      img.assign(total, zero());
      lay.write(img.data());
      if (!pr.a_col.empty()) memcpy(img.data() + o_col, pr.a_col.data(), pr.a_col.size() * 4);
      for (size_t p = 0; p < pr.periodic.size(); p++) {
        const size_t cyc = pr.periodic[p].size();
        std::vector<felt> kc = pr.periodic[p];
        host_interpolate(kc, one());
        const std::vector<felt> kv = host_evaluate(kc, cyc * ce, pow_u64(g, n / cyc));
        memcpy(img.data() + lay.tab[p], kv.data(), kv.size() * 16);
      }
      uint32_t* scol = reinterpret_cast<uint32_t*>(img.data() + o_scol);
      ProgSeq* sdesc = reinterpret_cast<ProgSeq*>(img.data() + o_sdesc);
      ProgPubSeq* pseq = reinterpret_cast<ProgPubSeq*>(img.data() + o_pseq);
      size_t soff = 0, q = 0;
      for (size_t j = 0; j < S; j++) {
        scol[j] = sv[j].col;
        img[o_sval + j] = params ? zero() : sv[j].val;
        if (!sv[j].sequence()) continue;
        if (params) {
          const uint32_t k = sv[j].nvals;
          if (sv[j].pub < 0) memcpy(img.data() + o_stab + soff, sv[j].values.data(), (size_t)k * 16);
          pseq[q] = ProgPubSeq{(uint32_t)soff, ilog2(k), (uint32_t)sv[j].first,
                               sv[j].pub < 0 ? 0u : (uint32_t)sv[j].pub + 1};
          sdesc[q++] = ProgSeq{(uint32_t)j, (uint32_t)soff};
          soff += k;
          continue;
        }
        std::vector<felt> pc = sv[j].values;
        host_interpolate(pc, one());
        const felt tw = inv(pow_u64(wn, sv[j].first));
        felt sc = felt_u64(n);
        for (size_t i = 0; i < pc.size(); i++) {
          img[o_stab + soff + i] = mul(pc[i], sc);
          sc = mul(sc, tw);
        }
        sdesc[q++] = ProgSeq{(uint32_t)j, (uint32_t)soff};
        soff += pc.size();
      }
      ctx->upload(dimg, img.data(), total * 16);
      tag.assign(want, want + 2);
      if (pf.enabled) {  // the image's host cost: periodic tables, sequence interpolation, staging
        auto& hs = ctx->stats["host_prog_image"];
        hs.launches += 1;
        hs.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - img_t0).count();
        hs.bytes += (double)total * 16;
      }
    }
    ec.zinv = dz;
    ProgEvalArgs pa{};
    pa.code = lay.code(dimg);
    const felt* dsval = dimg + o_sval;
    const felt* dstab = dimg + o_stab;
    if (params) {
      // the instance, once per proof on the proof's stream: the pub table (through the pinned
      // ring, or above its 1 MiB an asynchronous copy from the instance's own vector, which the
      // proof's AirDesc keeps alive), the strided assertions' values, and every sequence
      // interpolated on the device: gather, one inverse NTT per group, twist
      felt* dpub = ctx->buf<felt>("prog_pub", pr.num_pub);
      ctx->upload(dpub, pr.pub.data(), (size_t)pr.num_pub * 16);
      pa.code.pub = dpub;
      if (S) {
        std::vector<felt> sval(S);
        for (size_t j = 0; j < S; j++) sval[j] = sv[j].val;  // zero for a sequence
        felt* d = ctx->buf<felt>("prog_sval", S);
        ctx->upload(d, sval.data(), S * 16);
        dsval = d;
      }
      if (nseq) {
        felt* vals = ctx->buf<felt>("prog_seq_vals", seq_felts);
        felt* ntt = ctx->buf<felt>("prog_seq_ntt", seq_felts);
        felt* tab = ctx->buf<felt>("prog_seq_tab", seq_felts);
        ProgPubSeqArgs ga{};
        ga.nseq = (uint32_t)nseq;
        ga.logn = logn;
        ga.desc = reinterpret_cast<const ProgPubSeq*>(dimg + o_pseq);
        ga.pub = dpub;
        ga.raw = dimg + o_stab;
        ga.itwn = ctx->itws(logN) + ((n >> 1) - 1);
        uint64_t maxk = 1;
        for (const airp::Strided& a : sv) maxk = std::max<uint64_t>(maxk, a.nvals);
        launch_prog_seq_gather(pf, st, ga, maxk, vals);
        // the sequences of one group are consecutive and share k: one batched transform each
        size_t off = 0;
        for (size_t j = 0; j < S;) {
          size_t e = j, cnt = 0;
          while (e < S && sv[e].stride == sv[j].stride && sv[e].first == sv[j].first) cnt += sv[e++].sequence();
          const uint64_t k = n / sv[j].stride;
          if (cnt && k > 1) {
            NttBatch ib{vals + off, ntt + off, nullptr, k, k, 1, 1, (uint32_t)cnt};
            launch_ntt(pf, st, ib, ilog2(k), false, ctx->itws(logN), logN);
          } else if (cnt) {
            HIP_CHECK(hipMemcpyAsync(ntt + off, vals + off, cnt * 16, hipMemcpyDeviceToDevice, st));
          }
          off += cnt * k;
          j = e;
        }
        launch_prog_seq_twist(pf, st, ga, maxk, ntt, tab);
        dstab = tab;
      }
    }
    pa.num_t = pr.num_t;
    pa.a_col = reinterpret_cast<const uint32_t*>(dimg + o_col);
    pa.cc = dt_cc;
    pa.a_val = dt_aval;
    pa.col_stride = n << logBl;
    pa.binv = ctx->buf<felt>("binv_scratch", ((uint64_t)cel * n) / 2048 + 1);
    // groups of assertions that share a step (sorted by step): one divisor table
    // 1/(x - w^step) each, domain-only, cached per (domain, step)
    for (size_t k = 0; k < air.a_step.size(); k++) {
      if (k == 0 || air.a_step[k] != air.a_step[k - 1]) {
        if (pa.ngroups == PROG_MAX_GROUPS) throw ZkpFail{ZKP_ERR_UNSUPPORTED_AIR, "assertions over more than 4 steps"};
        const uint32_t gi = pa.ngroups++;
        const std::string key = "binv_prog_" + dom + "_" + std::to_string(air.a_step[k]);
        pa.w_step[gi] = pow_u64(wn, air.a_step[k]);
        pa.dinv[gi] = ctx->buf<felt>(key, (uint64_t)cel * n);
        pa.dinv_ready[gi] = ctx->have_cached(key);
      }
      pa.grp_end[pa.ngroups - 1] = (uint32_t)k + 1;
    }
    if (!S) {
      launch_eval_program(pf, st, ec, pa, tlde, comp);
      return;
    }
    ProgStridedArgs sa{};
    ProgSeqArgs qa{};
    sa.col = reinterpret_cast<const uint32_t*>(dimg + o_scol);
    sa.val = dsval;
    sa.cc = qa.cc = dt_cc + pr.num_t + pr.a_col.size();
    qa.desc = reinterpret_cast<const ProgSeq*>(dimg + o_sdesc);
    qa.tab = dstab;
    int wslot[PROG_MAX_STRIDED_GROUPS] = {-1, -1, -1, -1};  // the group's column of W, if it holds a sequence
    uint32_t seqs = 0;
    for (size_t j = 0; j < S; j++) {
      const uint64_t k = n / sv[j].stride, len = sv[j].stride * ce;
      if (j == 0 || sv[j].stride != sv[j - 1].stride || sv[j].first != sv[j - 1].first) {
        if (sa.ngroups == PROG_MAX_STRIDED_GROUPS)
          throw ZkpFail{ZKP_ERR_UNSUPPORTED_AIR, "strided assertions over more than 4 groups"};
        const uint32_t gi = sa.ngroups++;
        sa.mask[gi] = (uint32_t)(len - 1);
        // 1/(x^k - w_n^(first k)) by CE index modulo stride * ce: x^k = g^k w_len^s. Domain-only:
        // built once per (n, ce, stride, first) by the batch inversion of the single-step
        // tables; g^k sits behind the table for the kernels to read
        const std::string key = "dstr_" + std::to_string(logn) + "_" + std::to_string(logce) + "_" +
                                std::to_string(sv[j].stride) + "_" + std::to_string(sv[j].first);
        felt* tab = ctx->buf<felt>(key, len + 1);
        if (!ctx->have_cached(key)) {
          const felt gk = pow_u64(g, k);
          ctx->upload(tab + len, &gk, 16);
          launch_strided_den_table(pf, st, tab + len, ctx->tws(logN) + (len / 2 - 1), ilog2(len),
                                   pow_u64(wn, sv[j].first * k), pa.binv, tab);
        }
        sa.dtab[gi] = tab;
      }
      const uint32_t gi = sa.ngroups - 1;
      sa.grp_end[gi] = (uint32_t)j + 1;
      if (sv[j].sequence()) {
        if (wslot[gi] < 0) {
          wslot[gi] = (int)qa.ngroups++;
          qa.logk[wslot[gi]] = ilog2(k);
        }
        qa.seq_end[wslot[gi]] = ++seqs;
      }
    }
    if (qa.ngroups) {
      // W_g for the groups that hold a sequence: combined from the coefficients as drawn, then
      // extended to the CE cosets like the linear AIRs' combined columns (no host round trip)
      felt* wc = ctx->buf<felt>("strided_w_coef", (size_t)qa.ngroups * n);
      felt* wev = ctx->buf<felt>("strided_w_ev", (size_t)qa.ngroups * cel * n);
      launch_strided_combine(pf, st, qa, logn, wc);
      NttBatch eb{wc, wev, sce_rows() + (uint64_t)u0 * n, n, n, cel, cel, qa.ngroups * cel};
      launch_ntt(pf, st, eb, logn, true, ctx->tws(logN), logN);
      for (uint32_t gi = 0; gi < sa.ngroups; gi++)
        if (wslot[gi] >= 0) sa.W[gi] = wev + (size_t)wslot[gi] * cel * n;
    }
    launch_eval_program(pf, st, ec, pa, tlde, comp, &sa);
    return;
  }
  // coefficient-dependent constants, built on the device from the drawn coefficients
  // (MiMC: Z_T constants with the transition coefficient folded in, then b0, b1;
  // linear AIRs: the 4 coefficient rows + the two boundary sums)
  const uint32_t lw = air.id == ZKP_AIR_TRAINING_UPDATE ? w / 2 : w;
  felt* dconst = ctx->buf<felt>("eval_consts", air.id == ZKP_AIR_MIMC ? (size_t)ce + 4 : 4 * (size_t)lw + 2);
  launch_dt_eval_consts(pf, st, air.id, dt_cc, air.k, ec.w_last, dt_aval, dz, ce, w, air.num_t, dconst);
  ec.zinv = air.id == ZKP_AIR_MIMC ? dconst : dz;
  // coefficient form for the linear AIRs (profiles/r03_ab_linear_coef_eval.txt)
  const bool coef_form = air.id != ZKP_AIR_MIMC && coef;
  if (!cel && !coef_form) return;
  // linear AIRs: the divisor tables and the final per-point formula (both forms)
  auto linear = [&](LinearEvalArgs& la, const std::string& key) {
    la.binv = ctx->buf<felt>("binv_scratch", ((uint64_t)cel * n) / 2048 + 1);
    la.dinv = ctx->buf<felt>(key, (uint64_t)cel * n);
    la.binv_ready = ctx->have_cached(key);
    if (!coef_form) {
      launch_eval_linear(pf, st, ec, la, tlde, comp);
      return;
    }
    const uint32_t R = cm ? (uint32_t)cm->world : 1u, rank = cm ? (uint32_t)cm->rank : 0u;
    const uint32_t narr = (la.transition ? 1u : 0u) + 1u + (la.two_groups ? 1u : 0u);
    const uint64_t nR = n / R;
    felt* lc = ctx->buf<felt>("lin_coef", (size_t)narr * n);
    felt* mine = R > 1 ? ctx->buf<felt>("lin_mine", (size_t)narr * nR) : lc;
    felt* part = ctx->buf<felt>("lincomb_part", (size_t)4 * lincomb_groups(nR, la.width) * nR);
    launch_lin_lincomb(pf, st, la.transition, la.two_groups, coef, la.width, logn, (uint64_t)rank * nR, nR,
                       dconst, twn, mine, part);
    for (uint32_t i = 0; R > 1 && i < narr; i++) cm->all_gather(st, mine + i * nR, lc + i * n, nR * 16);
    if (!cel) return;
    // extend to the CE cosets u0..u0+cel
    const felt* Sce = sce_rows();
    felt* ev = ctx->buf<felt>("lin_ev", (size_t)narr * cel * n);
    NttBatch eb{lc, ev, Sce + (uint64_t)u0 * n, n, n, cel, cel, narr * cel};
    launch_ntt(pf, st, eb, logn, true, ctx->tws(logN), logN);
    launch_eval_linear_pts(pf, st, ec, la, ev, comp);
  };
  if (air.id == ZKP_AIR_MIMC) {
    // periodic column K over the CE domain: interpolate over <w_64>, evaluate at g^(n/64) * <w_{64 ce}>
    // (domain-only: cached per (n, ce))
    const std::string kkey = "kper_" + std::to_string(logn) + "_" + std::to_string(logce);
    felt* dk = ctx->buf<felt>(kkey, 64 * (size_t)ce);
    if (!ctx->have_cached(kkey)) {
      std::vector<felt> kc(64);
      for (int j = 0; j < 64; j++) kc[j] = felt_u64((uint64_t)(j + 1) * 1000000ull);
      host_interpolate(kc, one());
      std::vector<felt> kv = host_evaluate(kc, 64 * ce, pow_u64(g, n / 64));
      ctx->upload(dk, kv.data(), kv.size() * 16);
    }
    MimcEvalArgs ma;
    ma.bcoef = dconst + ce;  // the regrouped boundary constants A, Bc, Cc, D
    ma.kper = dk;
    // divisor inverses depend only on the domain and the assertion steps: cache per config
    std::string key = "binv_mimc_" + dom;
    ma.binv = ctx->buf<felt>("binv_scratch", ((uint64_t)cel * n) / 2048 + 1);
    ma.dinv = ctx->buf<felt>(key, (uint64_t)cel * n);
    ma.binv_ready = ctx->have_cached(key);
    launch_eval_mimc(pf, st, ec, ma, tlde, comp);
  } else if (air.id == ZKP_AIR_GLOBAL_UPDATE) {
    // GlobalUpdate: T = sum_i a^i (k*next_i - k*cur_i - next_{i+60}); B = sum_c b_c (cur_c - v_c)
    LinearEvalArgs la;
    la.width = w;
    la.transition = true;
    la.two_groups = false;
    la.coefs = dconst;  // [next | cur | beta0 | beta1 | bconst0, bconst1]
    la.w_bstep = pow_u64(wn, air.a_step[0]);
    la.w_bstep1 = zero();
    linear(la, "binv_lin_" + dom + "_" + std::to_string(air.a_step[0]));
  } else {
    // TrainingUpdate: transitions identically zero; boundary groups at rows 0 and n-1 over
    // the masked columns 0..w/2 (the mask columns are never read)
    const uint32_t half = w / 2;
    LinearEvalArgs la;
    la.width = half;
    la.transition = false;
    la.two_groups = true;
    la.coefs = dconst;
    la.w_bstep = one();
    la.w_bstep1 = ec.w_last;
    linear(la, "binv_tu_" + dom);
  }
}

// LastCol constants per LDE coset j (ce == B): kappa_j = (g w_N^j)^n = g^n w_B^j and
// kappa_j^-(C-1), at [2j, 2j+1] (shape-only: cached per (n, B, C))
const felt* last_col_kappa(zkp_ctx* ctx, uint32_t logn, uint32_t logB, uint32_t C) {
  const uint32_t B = 1u << logB;
  const std::string key = "lastcol_kap_" + std::to_string(logn) + "_" + std::to_string(logB) + "_" +
                          std::to_string(C);
  felt* d = ctx->buf<felt>(key, 2 * (size_t)B);
  if (!ctx->have_cached(key)) {
    std::vector<felt> h(2 * (size_t)B);
    const felt gn = pow_u64(felt_u64(3), 1ull << logn), wB = root_of_unity(logB);
    for (uint32_t j = 0; j < B; j++) {
      h[2 * j] = mul(gn, pow_u64(wB, j));
      h[2 * j + 1] = inv(pow_u64(h[2 * j], C - 1));
    }
    ctx->upload(d, h.data(), h.size() * 16);
  }
  return d;
}

// constants of k_comp_dft: [g^-mn / ce for m < C | w_ce^-k for k < ce/2]
std::vector<felt> comp_dft_consts(uint64_t n, uint32_t logce, uint32_t C) {
  const uint32_t ce = 1u << logce;
  std::vector<felt> dc((size_t)C + ce / 2);
  const felt g = felt_u64(3), ce_inv = inv(felt_u64(ce)), gn_inv = inv(pow_u64(g, n)),
             wce_inv = inv(root_of_unity(logce));
  for (uint32_t m = 0; m < C; m++) dc[m] = mul(pow_u64(gn_inv, m), ce_inv);
  for (uint32_t k = 0; k < ce / 2; k++) dc[C + k] = pow_u64(wce_inv, k);
  return dc;
}

// Sharded, each rank combines 1/R of the positions and the combined column is
// all-gathered (n * 16 bytes in all) instead of every rank reading all w columns.
void deep_evaluations(zkp_ctx* ctx, zkp_comm* cm, hipStream_t st, DeepArgs da, const felt* coef, uint64_t n,
                      const felt* Sj0, uint32_t logN, felt* out) {
  if (da.w < DEEP_COEF_MIN_W) {
    launch_deep(ctx->prof, st, da, out);
    return;
  }
  const uint32_t Bl = 1u << da.logBl;
  const uint32_t R = (uint32_t)cm->world;
  felt* acomb = ctx->buf<felt>("deep_acoef", n);
  const uint64_t nR = n / R;
  felt* part = ctx->buf<felt>("lincomb_part", (size_t)lincomb_groups(nR, da.w) * nR);
  if (R == 1) {
    launch_deep_lincomb(ctx->prof, st, coef, da.w, n, 0, n, da.gamma, acomb, part);
  } else {
    felt* mine = ctx->buf<felt>("deep_acoef_rank", nR);
    launch_deep_lincomb(ctx->prof, st, coef, da.w, n, (uint64_t)cm->rank * nR, nR, da.gamma, mine, part);
    cm->all_gather(st, mine, acomb, nR * 16);
  }
  felt* alde = ctx->buf<felt>("deep_alde", (size_t)Bl * n);
  NttBatch lb{acomb, alde, Sj0, n, n, Bl, Bl, Bl};
  launch_ntt(ctx->prof, st, lb, da.logn, true, ctx->tws(logN), logN);
  // [1 | delta_0 .. delta_{C-1}]; keyed by C: one name for every C regrew the buffer at a
  // larger C and left its leading 1 unwritten
  const std::string g1key = "deep_g1_" + std::to_string(da.C);
  felt* g1 = ctx->buf<felt>(g1key, (size_t)da.C + 1);
  if (!ctx->have_cached(g1key)) {
    const felt unit = one();
    ctx->upload(g1, &unit, 16);
  }
  HIP_CHECK(hipMemcpyAsync(g1 + 1, da.gamma + da.w, (size_t)da.C * 16, hipMemcpyDeviceToDevice, st));
  da.w = 1;
  da.tlde = alde;
  da.gamma = g1;
  launch_deep(ctx->prof, st, da, out);
}

// Gathers every opening at the sorted unique LDE positions `pos` (this rank
// holds the LDE cosets [j0, j0 + Bl)); collective over cm when sharded.
void gather_openings(zkp_ctx* ctx, zkp_comm* cm, const std::vector<uint64_t>& pos, uint64_t n, uint32_t logB,
                     uint32_t j0, const felt* tlde, uint32_t w, const TreeShard& ttree, const felt* clde, uint32_t C,
                     const TreeShard& ctree, const std::vector<FriLayer>& layers, uint32_t L, uint32_t F,
                     Openings& op) {
  Prof& pf = ctx->prof;
  hipStream_t st = ctx->stream;
  const uint32_t R = (uint32_t)cm->world, rank = (uint32_t)cm->rank;
  const uint32_t B = 1u << logB, Bl = B / R;
  const uint64_t N = n << logB;
  // Openings: every item is (owner rank, local index) or a host-side top node.
  // Each rank gathers all items from its own memory (index 0 for items it does
  // not own), the gathered buffers are all-gathered, and every item is taken
  // from its owner's copy.
  struct SegPlan {
    const void* src;
    std::vector<uint64_t> idx;
    std::vector<int32_t> owner;  // -1: host top node (value in host_dig)
    std::vector<const uint8_t*> host_dig;
    uint32_t words;
  };
  auto row_owner = [&](uint64_t j) -> uint32_t { return R > 1 ? (uint32_t)(j / Bl) : 0; };
  auto lde_values = [&](const felt* src, uint32_t cols) {
    SegPlan sp{src, {}, {}, {}, 4};
    sp.idx.reserve(pos.size() * cols);
    sp.owner.reserve(pos.size() * cols);
    sp.host_dig.reserve(pos.size() * cols);
    for (uint64_t p : pos) {
      uint64_t j = p & (B - 1), t = p >> logB;
      uint32_t ow = row_owner(j);
      for (uint32_t c = 0; c < cols; c++) {
        sp.idx.push_back(ow == rank ? ((uint64_t)c * Bl + (j - j0)) * n + t : 0);
        sp.owner.push_back((int32_t)ow);
        sp.host_dig.push_back(nullptr);
      }
    }
    return sp;
  };
  auto path_nodes = [&](const TreeShard& tr, const BatchPlan& bp) {
    SegPlan sp{tr.nodes, {}, {}, {}, 8};
    for (auto& pth : bp.paths)
      for (uint64_t k : pth) {
        TreeShard::Loc lc = tr.locate(k);
        if (lc.host) {
          sp.idx.push_back(0);
          sp.owner.push_back(-1);
          sp.host_dig.push_back(tr.top[lc.local].data());
        } else {
          sp.idx.push_back(lc.owner == (tr.logR ? rank : 0u) ? lc.local : 0);
          sp.owner.push_back(tr.logR ? (int32_t)lc.owner : (int32_t)rank);
          sp.host_dig.push_back(nullptr);
        }
      }
    return sp;
  };
  op.bt = plan_batch(N, pos);
  const BatchPlan& bt = op.bt;
  const BatchPlan& bc = bt;  // the constraint tree has the same shape and positions
  std::vector<std::vector<uint64_t>> fpos(L);
  op.bf.assign(L, BatchPlan{});
  std::vector<BatchPlan>& bf = op.bf;
  std::vector<SegPlan> plan;
  plan.push_back(lde_values(tlde, w));
  plan.push_back(path_nodes(ttree, bt));
  plan.push_back(lde_values(clde, C));
  plan.push_back(path_nodes(ctree, bc));
  {
    std::vector<uint64_t> cur = pos;
    for (uint32_t l = 0; l < L; l++) {
      const FriLayer& ly = layers[l];
      const uint64_t m16 = ly.m / F, Rows = (uint64_t)B * m16;
      fpos[l] = fold_positions(cur, Rows);
      bf[l] = plan_batch(Rows, fpos[l]);
      SegPlan sp{ly.E, {}, {}, {}, 4};
      for (uint64_t r : fpos[l])
        for (uint32_t k = 0; k < F; k++) {
          uint64_t i = r + k * Rows;  // natural index in the layer
          uint64_t j = i & (B - 1), tt = i >> logB;
          uint32_t ow = ly.sharded ? (uint32_t)(j / Bl) : rank;
          sp.idx.push_back(ow == rank ? (j - ly.jc) * ly.m + tt : 0);
          sp.owner.push_back((int32_t)ow);
          sp.host_dig.push_back(nullptr);
        }
      plan.push_back(sp);
      plan.push_back(path_nodes(ly.tree, bf[l]));
      cur = fpos[l];
    }
  }
  std::vector<GatherSeg>& segs = op.segs;
  segs.clear();
  std::vector<uint64_t> all_idx;
  uint64_t out_words = 0, max_count = 1;
  for (auto& sp : plan) {
    GatherSeg gs;
    gs.src = sp.src;
    gs.idx_off = all_idx.size();
    gs.count = sp.idx.size();
    gs.out_off = out_words;
    gs.words = sp.words;
    gs.pad = 0;
    all_idx.insert(all_idx.end(), sp.idx.begin(), sp.idx.end());
    out_words += gs.count * sp.words;
    max_count = std::max<uint64_t>(max_count, gs.count);
    segs.push_back(gs);
  }
  size_t seg_bytes = segs.size() * sizeof(GatherSeg), idx_bytes = all_idx.size() * 8;
  size_t up_bytes = seg_bytes + idx_bytes, down_bytes = out_words * 4;
  ctx->stage_end("7a_query_plan");
  uint8_t* hp = (uint8_t*)ctx->pinned(std::max(up_bytes, down_bytes * R) + 64);
  memcpy(hp, segs.data(), seg_bytes);
  memcpy(hp + seg_bytes, all_idx.data(), idx_bytes);
  uint8_t* dup = ctx->buf<uint8_t>("gather_in", up_bytes + 16);
  uint32_t* dout = ctx->buf<uint32_t>("gather_out", out_words + 4);
  uint32_t* dall = R > 1 ? ctx->buf<uint32_t>("gather_all", out_words * R + 4) : dout;
  HIP_CHECK(hipMemcpyAsync(dup, hp, up_bytes, hipMemcpyHostToDevice, st));
  launch_gather_multi(pf, st, (const GatherSeg*)dup, (uint32_t)segs.size(), max_count,
                      (const uint64_t*)(dup + seg_bytes), dout, (double)down_bytes * 2);
  if (R > 1) cm->all_gather(st, dout, dall, down_bytes);
  HIP_CHECK(hipMemcpyAsync(hp, dall, down_bytes * R, hipMemcpyDeviceToHost, st));
  ctx->sync();
  ctx->stage_end("7b_gather");
  op.gathered.assign(out_words, 0);
  std::vector<uint32_t>& gathered = op.gathered;
  {
    const uint32_t* all = reinterpret_cast<const uint32_t*>(hp);
    for (size_t si = 0; si < plan.size(); si++) {
      const SegPlan& sp = plan[si];
      const GatherSeg& gs = segs[si];
      for (size_t it = 0; it < sp.idx.size(); it++) {
        uint32_t* dst = gathered.data() + gs.out_off + it * sp.words;
        if (sp.owner[it] < 0) {
          memcpy(dst, sp.host_dig[it], 32);
        } else {
          uint32_t ow = R > 1 ? (uint32_t)sp.owner[it] : 0;
          memcpy(dst, all + (size_t)ow * out_words + gs.out_off + it * sp.words, sp.words * 4);
        }
      }
    }
  }
}

// Openings assembled on the host from the device's full gather (k_gather_full,
// world 1): the row values of every drawn position and the full sibling path of
// every leaf; the batch plans (plan_batch) pick their nodes from those paths.
// `raw` = the drawn positions in draw order (the gather's record order), `pos`
// = sorted unique; the result has gather_openings' segment layout.
void openings_from_full(const std::vector<uint64_t>& raw, const std::vector<uint64_t>& pos, const uint32_t* full,
                        const FullGatherArgs& ga, const std::vector<FriLayer>& layers, uint32_t L, uint32_t F,
                        Openings& op) {
  const uint32_t w = ga.w, C = ga.C, nv = w + C, logN = ga.logN;
  const uint64_t N = 1ull << logN, B = 1ull << ga.logB;
  auto missing = [] { return ZkpFail{ZKP_ERR_DEVICE, "device query gather is missing an opening"}; };
  // (leaf node index L + row, record index) sorted by node: node k at height d is on
  // the path of the leaves whose node index lies in [k << d, (k + 1) << d)
  struct Leaves {
    std::vector<std::pair<uint64_t, uint32_t>> v;
    uint32_t logL;
    // record of any drawn leaf below node k (height d above the leaves); -1 if none
    int64_t below(uint64_t k, uint32_t d) const {
      auto it = std::lower_bound(v.begin(), v.end(), std::make_pair(k << d, 0u));
      return it != v.end() && (it->first >> d) == k ? (int64_t)it->second : -1;
    }
    // height of node k above the leaves
    uint32_t height(uint64_t k) const { return logL - (63 - __builtin_clzll(k)); }
  };
  auto leaves_of = [&](uint64_t Lcount, uint32_t logL) {
    Leaves lv;
    lv.logL = logL;
    lv.v.reserve(raw.size());
    for (size_t i = 0; i < raw.size(); i++) lv.v.push_back({Lcount + (raw[i] & (Lcount - 1)), (uint32_t)i});
    std::sort(lv.v.begin(), lv.v.end());
    return lv;
  };
  op.segs.clear();
  op.gathered.clear();
  op.gathered.reserve(full ? 4096 : 0);
  auto begin_seg = [&](uint32_t words) {
    GatherSeg g{};
    g.out_off = op.gathered.size();
    g.words = words;
    op.segs.push_back(g);
  };
  auto put = [&](const uint32_t* src, uint32_t words) {
    op.gathered.insert(op.gathered.end(), src, src + words);
    op.segs.back().count++;
  };
  // a batch path node k is the sibling, at height d, of a drawn leaf's path: the record
  // of a leaf below k ^ 1 holds it at path slot d
  auto paths = [&](const BatchPlan& bp, const Leaves& lv, uint32_t seg, uint32_t path_off) {
    begin_seg(8);
    for (auto& pth : bp.paths)
      for (uint64_t k : pth) {
        const uint32_t d = lv.height(k);
        const int64_t i = lv.below(k ^ 1ull, d);
        if (i < 0) throw missing();
        put(full + ga.seg_off[seg] + (uint64_t)i * ga.rec_words[seg] + path_off + 8 * d, 8);
      }
  };
  const Leaves l0 = leaves_of(N, logN);
  op.bt = plan_batch(N, pos);
  for (int seg = 0; seg < 2; seg++) {  // values, then batch paths, of the trace and constraint commitments
    begin_seg(4);
    for (uint64_t p : pos) {
      const int64_t i = l0.below(N + p, 0);
      if (i < 0) throw missing();
      const uint32_t* r = full + (uint64_t)i * ga.rec_words[0];
      for (uint32_t c = seg ? w : 0; c < (seg ? nv : w); c++) put(r + 4 * c, 4);
    }
    paths(op.bt, l0, 0, 4 * nv + (seg ? 8 * logN : 0));
  }
  op.bf.assign(L, BatchPlan{});
  std::vector<uint64_t> cur = pos;
  for (uint32_t l = 0; l < L; l++) {
    const uint64_t Rows = B * (layers[l].m / F);
    const Leaves lv = leaves_of(Rows, ga.logrows[l]);
    std::vector<uint64_t> fp = fold_positions(cur, Rows);
    op.bf[l] = plan_batch(Rows, fp);
    begin_seg(4);
    for (uint64_t r : fp) {
      const int64_t i = lv.below(Rows + r, 0);
      if (i < 0) throw missing();
      const uint32_t* rec = full + ga.seg_off[1 + l] + (uint64_t)i * ga.rec_words[1 + l];
      for (uint32_t k = 0; k < F; k++) put(rec + 4 * k, 4);
    }
    paths(op.bf[l], lv, 1 + l, 4 * F);
    cur = fp;
  }
}

// constants of the fold iDFTs, cached per context: w_16^-m for m < 8 (w_8^-m and
// w_4^-m by stride), then 1/16, 1/8, 1/4, 1/2
const felt* fold_constants(zkp_ctx* ctx) {
  felt* deps = ctx->buf<felt>("eps_inv", 12);
  if (!ctx->have_cached("eps_inv")) {
    std::vector<felt> eps(12);
    felt einv = inv(root_of_unity(4));
    eps[0] = one();
    for (int m = 1; m < 8; m++) eps[m] = mul(eps[m - 1], einv);
    for (int k = 0; k < 4; k++) eps[8 + k] = inv(felt_u64(16 >> k));
    ctx->upload(deps, eps.data(), eps.size() * 16);
  }
  return deps;
}

}  // namespace zkpi
