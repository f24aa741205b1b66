/*
 * zkp.h — C-ABI of the MI355X-native STARK prover (libzkp.so).
 *
 * Drop-in boundary for the reference's proving path: winterfell 0.12's
 * `Prover::prove(&self, trace) -> Result<Proof, ProverError>` as driven by the
 * project's plug-ins
 *   /root/reference/src/aggregation/prover.rs:194-248  (GlobalUpdateProver)
 *   /root/reference/src/training/prover.rs:221-300     (TrainingUpdateProver)
 * and called from /root/reference/src/main.rs:228,424,468.
 * The `Default*` engine components those plug-ins select (DefaultTraceLde,
 * DefaultConstraintEvaluator, DefaultConstraintCommitment, Blake3_256,
 * MerkleTree, DefaultRandomCoin, FRI) are what this library replaces.
 *
 * Conventions
 *  - Field: winter-math f128 (p = 2^128 - 45*2^40 + 1). A felt is 16 bytes,
 *    canonical, little-endian: identical to `BaseElement` memory and to
 *    `Serializable` bytes (reference: src/aggregation/air.rs:10).
 *  - Traces are column-major (`ColMatrix`, what `TraceTable::init(transpose(rows))`
 *    produces: src/aggregation/prover.rs:157-160, src/helper.rs:197-211):
 *    element (row r, column c) lives at cols[c * n + r].
 *  - Inputs are borrowed for the call; outputs are callee-allocated and
 *    released with zkp_free(). No exceptions or aborts cross the ABI: every
 *    entry point returns a zkp_status.
 *  - Calls on one zkp_ctx are synchronous and must not overlap (the
 *    reference's `prove(&self)` is blocking). Use one ctx per thread.
 *  - There is no CPU fallback: if no gfx950 device is present every compute
 *    entry point fails with ZKP_ERR_DEVICE.
 */
#ifndef ZKP_H
#define ZKP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkp_felt {
  uint64_t lo;
  uint64_t hi;
} zkp_felt;

/* AIRs are identified by id because the device cannot run Rust
 * `Air::evaluate_transition`; parameters come from `pub_inputs.to_elements()`.
 *  MIMC          : builder-defined MiMC AIR (the reference has none, F2).
 *                  width 1, pub = [x0, x_last].
 *  GLOBAL_UPDATE : GlobalUpdateAir, src/aggregation/air.rs:89-151. width 120,
 *                  pub = GlobalUpdateInputs::to_elements() (123 felts, air.rs:57-81).
 *  TRAINING_UPDATE: TrainingUpdateAir, src/training/air.rs:101-292. width 240,
 *                  pub = TrainingUpdateInputs::to_elements() (air.rs:74-98: 244 + bs*(FE+AC)
 *                  felts); transitions identically zero (current_step() == 0). */
typedef enum zkp_air_id {
  ZKP_AIR_MIMC = 1,
  ZKP_AIR_GLOBAL_UPDATE = 2,
  ZKP_AIR_TRAINING_UPDATE = 3
} zkp_air_id;

/* ---- caller-defined AIRs: constraint programs ------------------------------
 * A zkp_air_program states an AIR as data: the transition constraints as a
 * straight-line program of field operations that the device runs at every point
 * of the constraint-evaluation domain (and the host verifier at the OOD point),
 * periodic columns, and single-row assertions. Registered through zkp_air_register
 * or zkp_air_register_strided its values are concrete for one instance: constants,
 * assertion steps and assertion values are what `Air::new` derives from the public
 * inputs, `pub_elems` still seeds the coin, and the program itself never reads it.
 * zkp_air_register_params (below) registers one program for every instance: its
 * operands and assertion values may come from each proof's `pub_elems`. Each entry
 * returns an id (>= 16) that every entry point taking a zkp_air_id accepts.
 *
 * Op encoding (one uint64_t per op):
 *   bits  0..7   opcode (ZKP_OP_*)
 *   bits  8..15  destination register (ADD, SUB, MUL; 0 for EMIT)
 *   bits 16..31  operand a
 *   bits 32..47  operand b (ADD, SUB, MUL; 0 for EMIT)
 *   bits 48..63  zero
 * An operand is (kind << 13) | index with kind one of ZKP_SRC_*:
 *   REG index < num_registers, CUR / NEXT index < width (the frame's two rows),
 *   PERIODIC index < num_periodic, CONST index < num_constants, PUB (zkp_air_register_params
 *   only) index < num_pub.
 * ADD / SUB / MUL write registers[dst] = a op b; EMIT a yields the value of the
 * next transition constraint, in order (exactly num_constraints EMITs). A register
 * must be written before it is read.
 *
 * degrees[i] (1..17) is constraint i's declared degree in trace-column factors
 * (winterfell `TransitionConstraintDegree::new`); the AIR's constraint-evaluation
 * blowup comes from the largest one. Registration walks the code (ADD/SUB -> max,
 * MUL -> sum, periodic values and constants -> 0) and refuses a constraint whose
 * syntactic degree exceeds its declared degree.
 * Periodic column p holds periodic_cycles[p] values (a power of two in 2..1024,
 * at most the trace length it is used with), all columns' values concatenated in
 * periodic_values. Assertions are single-row (`Assertion::single`), over at most
 * 4 distinct steps; they are kept sorted by (step, column), the order in which
 * winterfell draws their composition coefficients, so a caller may pass them in
 * any order. */
enum { ZKP_OP_ADD = 0, ZKP_OP_SUB = 1, ZKP_OP_MUL = 2, ZKP_OP_EMIT = 3 };
enum { ZKP_SRC_REG = 0, ZKP_SRC_CUR = 1, ZKP_SRC_NEXT = 2, ZKP_SRC_PERIODIC = 3, ZKP_SRC_CONST = 4 };
#define ZKP_AIR_OPERAND(kind, index) ((uint64_t)(((uint32_t)(kind) << 13) | (uint32_t)(index)))
#define ZKP_AIR_OP(opcode, dst, a, b) \
  ((uint64_t)(opcode) | ((uint64_t)(dst) << 8) | ((uint64_t)(a) << 16) | ((uint64_t)(b) << 32))
enum {
  ZKP_AIR_FIRST_ID = 16,         /* registered ids start here */
  ZKP_AIR_MAX_CONSTRAINTS = 1024,
  ZKP_AIR_MAX_DEGREE = 17,
  ZKP_AIR_MAX_CONSTANTS = 256,
  ZKP_AIR_MAX_PERIODIC = 8,
  ZKP_AIR_MAX_CYCLE = 1024,
  ZKP_AIR_MAX_ASSERTIONS = 1024,
  ZKP_AIR_MAX_ASSERTION_STEPS = 4,
  ZKP_AIR_MAX_OPS = 8192,
  ZKP_AIR_MAX_REGISTERS = 32
};
typedef struct zkp_air_assertion {
  uint32_t column;
  uint32_t reserved;  /* 0 */
  uint64_t step;
  zkp_felt value;
} zkp_air_assertion;
typedef struct zkp_air_program {
  uint32_t width;                      /* trace columns, 1..255 */
  uint32_t num_constraints;            /* 1..1024 */
  const uint8_t* degrees;              /* num_constraints declared degrees, 1..17 */
  uint32_t num_constants;              /* <= 256 */
  const zkp_felt* constants;           /* canonical felts */
  uint32_t num_periodic;               /* <= 8 */
  const uint32_t* periodic_cycles;     /* num_periodic cycle lengths */
  const zkp_felt* periodic_values;     /* sum of the cycles, column after column */
  uint32_t num_assertions;             /* <= 1024 */
  const zkp_air_assertion* assertions;
  uint32_t num_registers;              /* 1..32 */
  uint32_t num_ops;                    /* 1..8192 */
  const uint64_t* ops;
} zkp_air_program;
/* Validates everything that does not depend on the trace length and stores a copy
 * in a process-wide table (thread-safe); *air_id receives the new id. Ids are never
 * reused. ZKP_ERR_ARGUMENT on a refused program: zkp_air_last_error() names the
 * failing field (per thread, valid until the thread's next zkp_air_* call). */
int zkp_air_register(const zkp_air_program* program, int* air_id);
/* Frees the id (ZKP_ERR_ARGUMENT if it is not registered). Sessions and proofs
 * already running under it keep their copy. */
int zkp_air_unregister(int air_id);
const char* zkp_air_last_error(void);

/* Strided assertions (winterfell `Assertion::periodic` and `Assertion::sequence`),
 * registered beside a program's single-row ones. With k = n / stride:
 *   periodic (num_values = 0): T[column][first_step + stride*i] = value for every i < k;
 *   sequence (num_values = k): T[column][first_step + stride*i] = values[i].
 * stride is a power of two >= 2 and first_step < stride. All assertions of an AIR are
 * kept sorted by (stride, first_step, column), stride counting as 0 for the single-row
 * ones: the singles come first in their (step, column) order, the strided ones follow,
 * and each takes one composition coefficient in that order (the proof's context counts
 * each once). Assertions that share (stride, first_step) form one group with the divisor
 * x^k - w_n^(first_step * k); a group's term is sum_j cc_j * (T_col_j(x) - V_j(x)) over it,
 * V_j the constant `value`, or for a sequence P_j(x * w_n^-first_step) with P_j the
 * polynomial of degree < k through values[i] at w_k^i (w_k = w_n^stride). A sequence of
 * equal values therefore gives the field elements of the periodic form, and stride = n
 * those of a single-row assertion at first_step.
 * Registration refuses (ZKP_ERR_ARGUMENT, zkp_air_last_error() names strided[i]): a
 * stride that is not a power of two >= 2, first_step >= stride, a column outside the
 * width, a value that is not canonical, a num_values that is not a power of two, a
 * sequence without values, more than ZKP_AIR_MAX_SEQUENCE_VALUES sequence values in the
 * program, more than ZKP_AIR_MAX_ASSERTIONS assertions (single and strided together),
 * more than ZKP_AIR_MAX_STRIDED_GROUPS distinct (stride, first_step), and two assertions
 * over one cell: on one column, strided against strided when first_a = first_b modulo
 * the smaller stride, single against strided when step = first_step modulo stride.
 * num_strided = 0 is zkp_air_register. The singles keep their limit of 4 steps. */
enum {
  ZKP_AIR_MAX_STRIDED_GROUPS = 4,
  ZKP_AIR_MAX_SEQUENCE_VALUES = 1 << 18 /* per program, all sequences together */
};
typedef struct zkp_air_strided_assertion {
  uint32_t column;
  uint32_t num_values;     /* 0: periodic, `value` holds; >= 1 (a power of two): sequence of that many `values` */
  uint64_t first_step;
  uint64_t stride;
  zkp_felt value;
  const zkp_felt* values;  /* null for periodic */
} zkp_air_strided_assertion;
int zkp_air_register_strided(const zkp_air_program* program, const zkp_air_strided_assertion* strided,
                             uint32_t num_strided, int* air_id);

/* Public inputs: one id, many instances. zkp_air_register_params registers a program whose
 * values may come from the `pub_elems` of each proof instead of from the registration, the
 * way winterfell's `Air::new(trace_info, pub_inputs, options)` derives them:
 *  - an operand of kind ZKP_SRC_PUB is pub[index] (degree 0, like a constant),
 *    index < num_pub and < ZKP_AIR_MAX_PUB_OPERAND;
 *  - a binding gives an assertion its value from pub (see the kinds below). `index` refers
 *    to the caller's arrays as passed, before the library sorts them. A bound assertion's
 *    own value / values must be zero / null; a bound sequence still states num_values.
 * Refused with ZKP_ERR_ARGUMENT (zkp_air_last_error() names bindings[i] or ops[pc]): num_pub
 * of 0 or above ZKP_AIR_MAX_PUB, a pub_offset or a sequence run that ends past num_pub, an
 * index outside its array, an unknown kind, two bindings of one assertion, a bound assertion
 * that states a value, a PUB operand index >= num_pub. The other rules are those of
 * zkp_air_register_strided, which is the num_pub = 0 case of this entry (there every
 * ZKP_SRC_PUB operand is refused).
 * Under such an id every entry that takes pub_elems (zkp_prove, zkp_prove_device,
 * zkp_prove_sharded* over one rank, zkp_session_create, zkp_channel_create, zkp_verify)
 * requires n_pub == num_pub and canonical felts: ZKP_ERR_PUB_INPUTS (zkp_verify:
 * ZKP_VERIFY_PUB_INPUTS) otherwise. Every value of a proof is that of the concrete program
 * with pub's values substituted, proved with the same pub_elems: the bytes are identical.
 * Device: the image cached per (id, n, blowup) holds no value of pub, so instances of one id
 * do not upload it again. Per proof the pub table goes up once (read by the interpreter
 * through uniform loads, like the constants), the bound values of the single and periodic
 * assertions ride the small per-proof value arrays, and each sequence is interpolated on
 * the device (gather from the pub table, inverse NTT of size k, twist and scale) in three
 * buffers shared by all instances, instead of once per registration on the host. */
enum { ZKP_SRC_PUB = 5 };
enum { ZKP_AIR_MAX_PUB = 1 << 19, ZKP_AIR_MAX_PUB_OPERAND = 1 << 13 };
enum { ZKP_BIND_ASSERTION = 0,   /* assertions[index].value       = pub[pub_offset] */
       ZKP_BIND_STRIDED   = 1 }; /* strided[index]: periodic value = pub[pub_offset];
                                    sequence values[i]             = pub[pub_offset + i] */
typedef struct zkp_air_binding { uint32_t kind, index; uint64_t pub_offset; } zkp_air_binding;
int zkp_air_register_params(const zkp_air_program* program, const zkp_air_strided_assertion* strided,
                            uint32_t num_strided, uint32_t num_pub, const zkp_air_binding* bindings,
                            uint32_t num_bindings, int* air_id);

/* Checks that need the trace length n. A registered id's entry points return
 * ZKP_ERR_PUB_INPUTS (zkp_verify: ZKP_VERIFY_PUB_INPUTS) for:
 *  - a width other than the program's;
 *  - an assertion step >= n;
 *  - a strided assertion's stride > n, or a sequence with num_values * stride != n;
 *  - a periodic cycle > n;
 *  - an n that divides d - 1, d being the largest declared degree (degree 9 over
 *    8 rows). The quotient of a degree-d constraint has (d-1)(n-1) + 1 coefficients.
 *    winterfell's count gives ceil((d-1)(n-1)/n) composition columns of n
 *    coefficients each, which is one coefficient short exactly in that case, so no
 *    proof of such a shape verifies.
 * Sharded proving over more than one rank returns ZKP_ERR_UNSUPPORTED_AIR for a
 * registered id from its arguments alone, before the first collective (the
 * communicator stays usable); a communicator of one rank accepts it.
 * Memory: a context keeps the device image of one program (the last id, n and
 * blowup it evaluated), and one table of n * ce divisor inverses per distinct
 * (domain, assertion step) it has met, like the built-in ids' tables. Instances
 * that assert other rows therefore add tables until the context is destroyed.
 * A strided group adds, per distinct (n, ce, stride, first_step), one table of
 * stride * ce divisor inverses (x^k depends on the CE index modulo stride * ce only),
 * kept like the single-step tables. The image also carries each sequence's k
 * interpolated coefficients. A group that holds a sequence costs, per proof, one
 * column of n coefficients and its n * ce evaluations; those two buffers are shared
 * by all instances and sized by the largest shape met. */

/* Host-only trace validation (winterfell's debug-build `validate` of a trace,
 * which `Prover::prove` runs before proving): every transition constraint on the
 * rows 0..n-2 with the periodic values of the row, then every assertion. A valid
 * trace returns ZKP_OK with *bad_row = UINT64_MAX. Otherwise still ZKP_OK, with
 * either the first failing row and its first failing constraint in *bad_row /
 * *bad_constraint (*bad_assertion = UINT32_MAX), or, when every transition holds,
 * *bad_row = the step of the first failing assertion (in stored order) and its
 * index in *bad_assertion (*bad_constraint = UINT32_MAX). The stored order is the
 * singles, then the strided assertions; a strided assertion reports its lowest
 * failing row. Registered ids only:
 * the built-in ids return ZKP_ERR_UNSUPPORTED_AIR. */
int zkp_air_check_trace(int air_id, const zkp_felt* trace_cols, uint32_t width, uint64_t n, uint64_t* bad_row,
                        uint32_t* bad_constraint, uint32_t* bad_assertion);
/* The same for an id of zkp_air_register_params, against the instance that pub_elems states
 * (n_pub == num_pub, canonical felts: ZKP_ERR_PUB_INPUTS otherwise); it also takes an id
 * without public inputs with n_pub = 0. zkp_air_check_trace itself returns ZKP_ERR_PUB_INPUTS
 * for an id with public inputs. */
int zkp_air_check_trace_pub(int air_id, const zkp_felt* pub_elems, uint64_t n_pub, const zkp_felt* trace_cols,
                            uint32_t width, uint64_t n, uint64_t* bad_row, uint32_t* bad_constraint,
                            uint32_t* bad_assertion);

/* winterfell `BatchingMethod`. */
enum { ZKP_BATCHING_LINEAR = 0, ZKP_BATCHING_ALGEBRAIC = 1, ZKP_BATCHING_HORNER = 2 };
/* winterfell `FieldExtension` (only None is supported, as in the reference). */
enum { ZKP_FIELD_EXTENSION_NONE = 1 };

/* winterfell `ProofOptions::new(num_queries, blowup_factor, grinding_factor,
 * field_extension, fri_folding_factor, fri_remainder_max_degree,
 * batching_constraints, batching_deep)`; the reference's set is
 * (40, 16, 21, None, 16, 7, Algebraic, Algebraic) at src/main.rs:98-107.
 *
 * Accepted: num_queries 1..255, blowup_factor a power of two in 2..128 and at
 * least the AIR's constraint-evaluation blowup, grinding_factor 0..32,
 * fri_folding_factor F in {2, 4, 8, 16}, fri_remainder_max_degree 2^k - 1 <= 255.
 * The FRI layers must also fit the trace: with L the number of layers (the domain
 * n * blowup_factor is divided by F while it exceeds
 * (fri_remainder_max_degree + 1) * blowup_factor), a trace of n rows needs
 * n >= F^L, so that the remainder has at least one coefficient. Shapes past that
 * (n = 64, blowup 8, remainder degree 0 at F = 16) have no verifying proof. A proof
 * also has at most 16 FRI layers (zkp_transcript.fri_roots); F = 16 never gets past
 * 7, F = 2 reaches 17 at n = 2^17, blowup 8, remainder degree 0. For both kinds of
 * shape the prover, session and channel entries return ZKP_ERR_INVALID_OPTIONS and
 * zkp_verify ZKP_VERIFY_UNACCEPTABLE_OPTIONS, decided on the host before any
 * device work.
 * Sharded proving (zkp_prove_sharded*) over more than one rank takes F = 16 only:
 * every rank returns ZKP_ERR_INVALID_OPTIONS for another factor from its arguments
 * alone, before the first collective, and the communicator stays usable. A
 * communicator of one rank takes all four factors. */
typedef struct zkp_proof_options {
  uint32_t num_queries;
  uint32_t blowup_factor;
  uint32_t grinding_factor;
  uint32_t field_extension;
  uint32_t fri_folding_factor;
  uint32_t fri_remainder_max_degree;
  uint32_t batching_constraints;
  uint32_t batching_deep;
} zkp_proof_options;

/* Status codes; non-zero values map onto winterfell `ProverError` classes. */
typedef enum zkp_status {
  ZKP_OK = 0,
  ZKP_ERR_INVALID_OPTIONS = 1,
  ZKP_ERR_UNSUPPORTED_FIELD_EXTENSION = 2,
  ZKP_ERR_TRACE_SHAPE = 3,   /* n < 8, n not a power of two, width 0 or > 255, n > 2^23, n*blowup > 2^28 */
  ZKP_ERR_PUB_INPUTS = 4,    /* wrong number of public input elements / inconsistent values */
  ZKP_ERR_DEVICE = 5,        /* HIP failure or no device */
  ZKP_ERR_NONCE = 6,         /* grinding nonce not found */
  ZKP_ERR_OOM = 7,
  ZKP_ERR_UNSUPPORTED_AIR = 8,
  ZKP_ERR_ARGUMENT = 9
} zkp_status;

typedef struct zkp_ctx zkp_ctx;

/* Per-proof transcript summary (debug / parity aid; optional out-param). */
typedef struct zkp_transcript {
  uint8_t trace_root[32];
  uint8_t constraint_root[32];
  uint8_t fri_roots[16][32];
  uint8_t remainder_commitment[32];
  uint32_t num_fri_layers;
  uint32_t num_composition_columns;
  uint64_t pow_nonce;
  zkp_felt z;
  uint32_t num_unique_queries;
  uint64_t query_positions[255];
} zkp_transcript;

/* ---- context --------------------------------------------------------- */
/* Bind to HIP device `device` (ordinal). One ctx per caller thread. */
int zkp_ctx_create(int device, zkp_ctx** out);
void zkp_ctx_destroy(zkp_ctx* ctx);
/* Free the idle stage-session context the ctx keeps for its next zkp_session_create
 * (at most one; it holds the last session's device buffers and domain tables). */
int zkp_ctx_trim(zkp_ctx* ctx);
/* The message of the context's last call that took ctx, empty after one that succeeded
 * (storage owned by ctx, valid until its next call). */
const char* zkp_last_error(const zkp_ctx* ctx);
void zkp_free(void* p);

/* ---- whole-proof entry points (≙ Prover::prove) ------------------------ */
/* Host trace (column-major, width*n felts) -> serialized proof
 * (≙ winterfell `Proof::to_bytes()`, src/main.rs:229,425,469). */
int zkp_prove(zkp_ctx* ctx, zkp_air_id air, const zkp_felt* trace_cols, uint32_t width,
              uint64_t n, const zkp_felt* pub_elems, uint64_t n_pub,
              const zkp_proof_options* opts, uint8_t** proof, uint64_t* proof_len,
              zkp_transcript* transcript /* nullable */);

/* Same, with the trace already resident in device memory (HBM). */
int zkp_prove_device(zkp_ctx* ctx, zkp_air_id air, const void* d_trace_cols, uint32_t width,
                     uint64_t n, const zkp_felt* pub_elems, uint64_t n_pub,
                     const zkp_proof_options* opts, uint8_t** proof, uint64_t* proof_len,
                     zkp_transcript* transcript /* nullable */);

/* zkp_air_check_trace (above) for a trace in device memory (width x n zkp_felt, column-major,
 * as zkp_prove_device takes it), checked on the device: one thread per frame (rows r, r + 1),
 * then the assertions (k_check_program). *bad_row / *bad_constraint / *bad_assertion
 * mean exactly what zkp_air_check_trace's mean and hold the same values for the same
 * trace: the UINT64_MAX / UINT32_MAX sentinels, the first failing row and its first
 * failing constraint, otherwise the first failing assertion in stored order.
 * Status: a null pointer (ctx included) returns ZKP_ERR_ARGUMENT; otherwise the status
 * zkp_air_check_trace returns for the same (air_id, width, n): ZKP_ERR_UNSUPPORTED_AIR
 * for built-in and unregistered ids, ZKP_ERR_TRACE_SHAPE for a bad n or width,
 * ZKP_ERR_PUB_INPUTS for the n-dependent refusals listed above; all of them decided on
 * the host before any launch, so the context stays usable. n above 2^23 (the longest
 * trace the prover takes) returns ZKP_ERR_TRACE_SHAPE. A HIP failure returns
 * ZKP_ERR_DEVICE. Field elements that are not canonical are outside the contract, as
 * for the host check. The call synchronises the context's stream once, to read the 16
 * result bytes; the trace is only read. The prover never calls it: a caller that wants
 * winterfell's debug-build validation back calls it before zkp_prove_device. */
int zkp_air_check_trace_device(zkp_ctx* ctx, int air_id, const void* d_trace_cols, uint32_t width, uint64_t n,
                               uint64_t* bad_row, uint32_t* bad_constraint, uint32_t* bad_assertion);
/* zkp_air_check_trace_pub for a trace in device memory: the statuses and results of
 * zkp_air_check_trace_pub, checked as zkp_air_check_trace_device checks. The pub table and
 * the bound single values go up once per call; the cached image holds no value of pub. */
int zkp_air_check_trace_device_pub(zkp_ctx* ctx, int air_id, const zkp_felt* pub_elems, uint64_t n_pub,
                                   const void* d_trace_cols, uint32_t width, uint64_t n, uint64_t* bad_row,
                                   uint32_t* bad_constraint, uint32_t* bad_assertion);

/* Each transition constraint's actual degree on a trace in device memory: the other half of
 * winterfell's debug-build checks (its evaluator compares every constraint's actual degree
 * with the declared one). Registration only bounds a constraint's degree syntactically, with
 * periodic values, constants and pub[i] counted as 0; but a periodic column of cycle c is a
 * polynomial of degree n - n/c (winterfell: TransitionConstraintDegree::with_cycles), so a
 * constraint can exceed what it declares, and terms that cancel or a pub value of zero can
 * leave it below. The proof's shape (ce, composition columns C) comes from the declarations.
 *
 * degrees[i] receives the degree of constraint i as a polynomial, i.e. of the program applied
 * to the trace columns' interpolants, the periodic columns' polynomials and the instance's pub
 * (not divided by the transition divisor), or ZKP_DEGREE_ZERO for the zero polynomial. The
 * trace need not satisfy the constraints and is only read. The report:
 *   eval_blowup    E = max(2, next_pow2(B)), B the largest zkp_air_degree_bounds value. The
 *                  degrees are measured on the n * E points g * <w_(n E)>: a constraint is a
 *                  product of at most B polynomials of degree <= n - 1, so its degree is at most
 *                  B (n - 1) < E n and nothing aliases. E does not depend on the declared
 *                  degrees: an under-declared program is the case in which the proof's own n * ce
 *                  points are too few.
 *   columns        C of a proof of this id at this n (from the declared degrees)
 *   columns_needed max(1, ceil((max_degree - (n - 1) + 1) / n)): the columns the largest
 *                  quotient fills; 1 when every constraint is zero
 *   first_under    the first i with degrees[i] > declared_i * (n - 1) (winterfell's comparison,
 *                  per constraint); UINT32_MAX if none
 *   proof_fits     the condition that decides whether a proof can verify. The transition divisor
 *                  (x^n - 1) / (x - w^(n-1)) has degree n - 1, so the quotient of a constraint of
 *                  degree D has D - (n - 1) + 1 coefficients; the C composition columns hold C n.
 *                  D - n + 2 <= C n, i.e. max_degree <= (C + 1) n - 2 (or all zero): 1, else 0.
 *                  When 0, the prover keeps C columns of the quotient and drops the rest, and the
 *                  bytes zkp_prove returns verify nowhere; declaring the degree `minimal`
 *                  = ceil(degree / (n - 1)) of the offending constraint repairs it.
 * Status, all decided on the host before the first HIP call, in zkp_air_check_trace_device_pub's
 * order (the context stays usable; zkp_last_error has a message): ZKP_ERR_ARGUMENT for a null
 * ctx, d_trace_cols, degrees or report, and for n_pub set with null pub_elems;
 * ZKP_ERR_UNSUPPORTED_AIR for a built-in or unregistered id; then whatever
 * zkp_air_check_trace_device_pub returns for the same arguments (ZKP_ERR_TRACE_SHAPE,
 * ZKP_ERR_PUB_INPUTS: the entry describes a proof of this shape, so "n divides d - 1" is refused
 * here too); ZKP_ERR_ARGUMENT for capacity < num_constraints; ZKP_ERR_UNSUPPORTED_AIR for E > 32;
 * ZKP_ERR_TRACE_SHAPE for n * E > 2^28. A HIP failure returns ZKP_ERR_DEVICE.
 * Device work: the columns are interpolated and extended to the E cosets; k_program_columns runs
 * the program once per point and chunk and stores the raw constraint values of K constraints at
 * a time; each is interpolated by the composition's route (per-coset inverse NTT, cross-coset
 * DFT keeping all E segments) and k_column_degrees finds its top non-zero coefficient. K is the
 * largest count for which K * E * n felts stay within 2^22 (64 MiB), at least 1 and at most 128:
 * beside the extended trace (width * E * n felts) the call holds two such chunk buffers, whatever
 * num_constraints is. All of it lives in buffers of its own: no buffer, image or table of a proof
 * or of the trace check is written. The call synchronises its stream once, to read the degrees.
 * zkp_prove never calls it. */
#define ZKP_DEGREE_ZERO UINT64_MAX /* the constraint is the zero polynomial on this trace */
typedef struct zkp_air_degree_report {
  uint32_t num_constraints;
  uint32_t eval_blowup;
  uint32_t columns;
  uint32_t columns_needed;
  uint64_t max_degree; /* largest actual degree, ZKP_DEGREE_ZERO if all are zero */
  uint32_t first_under;
  uint32_t proof_fits;
} zkp_air_degree_report;
int zkp_air_constraint_degrees_device(zkp_ctx* ctx, int air_id, const zkp_felt* pub_elems, uint64_t n_pub,
                                      const void* d_trace_cols, uint32_t width, uint64_t n, uint64_t* degrees,
                                      uint32_t capacity, zkp_air_degree_report* report);
/* Host only, no context, thread-safe: per constraint, the syntactic degree with every periodic
 * operand counted as 1 (ADD / SUB -> max, MUL -> sum, saturated at 255). ZKP_ERR_UNSUPPORTED_AIR
 * for an id that is not registered, ZKP_ERR_ARGUMENT for a null pointer or capacity <
 * num_constraints (*num_constraints is still set). */
int zkp_air_degree_bounds(int air_id, uint8_t* bounds, uint32_t capacity, uint32_t* num_constraints);
/* Host only, no context, thread-safe: the status zkp_air_constraint_degrees_device decides on the
 * host for these arguments after its null-pointer checks (capacity apart), with the message in
 * zkp_air_last_error; on ZKP_OK *eval_blowup = E and *chunk = K of such a call (both nullable). */
int zkp_air_constraint_degrees_shape(int air_id, const zkp_felt* pub_elems, uint64_t n_pub, uint32_t width,
                                     uint64_t n, uint32_t* eval_blowup, uint32_t* chunk);

/* ---- multi-GPU: coset-sharded proving ----
 * One proof is split over `world` ranks by LDE coset (rank r owns the cosets
 * [r*B/world, (r+1)*B/world)); the exchange steps are leaf-digest all-to-alls
 * for the Merkle commitments, an all-to-all + all-gather that reassemble the
 * composition polynomial, and all-gathers of subtree roots, small FRI layers
 * and query openings. Every rank passes the full trace and returns the same
 * proof bytes (identical to zkp_prove's). world must be a power of two <= the
 * blowup factor; n >= 256 * world.
 * Replaces, for a multi-GPU node, the single `Prover::prove` call
 * (src/main.rs:424,468) — the reference itself has no multi-device path. */
typedef struct zkp_comm zkp_comm;
/* RCCL communicator (one process per GPU): rank 0 makes the id, the caller
 * broadcasts its 128 bytes (e.g. with torch.distributed), every rank creates. */
int zkp_comm_rccl_unique_id(uint8_t id[128]);
int zkp_comm_rccl_create(zkp_ctx* ctx, const uint8_t id[128], int world, int rank, zkp_comm** out);
/* In-process group: `world` communicators for ranks run as threads of one
 * process (each with its own zkp_ctx; GPUs may be shared). comms[world]. */
int zkp_comm_local_group(int world, zkp_comm** comms);
/* Caller transport: one process per rank, the collectives carried by the
 * caller's own channel (torch.distributed/gloo, MPI, sockets ...) through pinned
 * host staging. Each callback is a blocking collective over all ranks that
 * returns 0 on success: all_to_all sends block s of `send` (block_bytes each) to
 * rank s and receives rank s's block for this rank into block s of `recv`;
 * all_gather puts rank s's `send` (bytes) at recv + s*bytes. abort (nullable)
 * is called when this rank's proof fails, to release blocked peers. The
 * exchange points are those of the RCCL backend; RCCL stays the production
 * transport over xGMI. */
typedef struct zkp_host_transport {
  void* user;
  int (*all_to_all)(void* user, const void* send, void* recv, uint64_t block_bytes);
  int (*all_gather)(void* user, const void* send, void* recv, uint64_t bytes);
  void (*abort)(void* user);
} zkp_host_transport;
int zkp_comm_host_create(int world, int rank, const zkp_host_transport* transport, zkp_comm** out);
void zkp_comm_destroy(zkp_comm* comm);
int zkp_comm_rank(const zkp_comm* comm);
int zkp_comm_world(const zkp_comm* comm);
/* The rank count the transport itself reports: ncclCommCount for an RCCL
 * communicator (so a run can show that RCCL saw every rank), the group size for
 * the in-process and caller transports; -1 on error. */
int zkp_comm_backend_world(const zkp_comm* comm);
/* Fabric check before proving (collective; no reference counterpart): one
 * all-to-all of world blocks of block_bytes (multiple of 4) and one all-gather
 * of block_bytes per rank, each run twice on the context's stream with
 * rank-tagged words verified on the host. a2a_ms / ag_ms (nullable) receive
 * the faster round's wall time of each collective on this rank. A mismatch
 * is ZKP_ERR_DEVICE naming the peer and word. */
int zkp_comm_check(zkp_ctx* ctx, zkp_comm* comm, uint64_t block_bytes, double* a2a_ms, double* ag_ms);
/* Collective: every rank of `comm` must call it with the same arguments. */
int zkp_prove_sharded(zkp_ctx* ctx, zkp_comm* comm, zkp_air_id air, const zkp_felt* trace_cols,
                      uint32_t width, uint64_t n, const zkp_felt* pub_elems, uint64_t n_pub,
                      const zkp_proof_options* opts, uint8_t** proof, uint64_t* proof_len,
                      zkp_transcript* transcript /* nullable */);

/* As zkp_prove_sharded with the full trace already in this rank's HBM. */
int zkp_prove_sharded_device(zkp_ctx* ctx, zkp_comm* comm, zkp_air_id air, const void* d_trace_cols,
                             uint32_t width, uint64_t n, const zkp_felt* pub_elems, uint64_t n_pub,
                             const zkp_proof_options* opts, uint8_t** proof, uint64_t* proof_len,
                             zkp_transcript* transcript /* nullable */);

/* Device scratch helpers so callers (bench, tests) can keep traces in HBM. */
int zkp_device_alloc(zkp_ctx* ctx, uint64_t bytes, void** d_ptr);
int zkp_device_free(zkp_ctx* ctx, void* d_ptr);
int zkp_copy_to_device(zkp_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
int zkp_copy_to_host(zkp_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);

/* ---- stage entry points (for a winter-prover fork / stage parity) ------ */
/* ≙ DefaultTraceLde::new (src/aggregation/prover.rs:216-224): interpolate each
 * column over <w_n>, evaluate on 3*<w_{n*blowup}>, hash rows with BLAKE3 and
 * build the Merkle tree. Outputs: LDE (column-major, natural domain order,
 * width*n*blowup felts; nullable) and root. */
int zkp_trace_lde_commit(zkp_ctx* ctx, const zkp_felt* trace_cols, uint32_t width, uint64_t n,
                         uint32_t blowup, zkp_felt* lde_out /* nullable */, uint8_t root[32]);

/* Batched BLAKE3 of rows of a column-major felt matrix (≙ RowMatrix::commit_to_rows
 * leaf hashing) followed by MerkleTree::new; returns the root. */
int zkp_merkle_commit_rows(zkp_ctx* ctx, const zkp_felt* cols, uint32_t width, uint64_t rows,
                           uint8_t root[32]);

/* Minimum-nonce grinding (sequential winterfell semantics):
 * smallest nonce >= 1 with trailing_zeros(u64_le(BLAKE3(seed || nonce_le)[0..8])) >= bits. */
int zkp_grind(zkp_ctx* ctx, const uint8_t seed[32], uint32_t bits, uint64_t* nonce);

/* ---- stage sessions: the plug-in hooks of a winter-prover fork ----------
 * A zkp_session holds one proof's device-resident state (trace polynomials and
 * LDE, composition evaluations and LDE, DEEP and FRI layers, Merkle trees), so
 * a fork of winter-prover 0.12 keeps `Prover::prove` / `generate_proof` and its
 * own channel (`DefaultRandomCoin<Blake3_256>`) and replaces only the stages:
 *   zkp_session_trace_lde  ≙ Prover::new_trace_lde -> DefaultTraceLde::new
 *                            (src/aggregation/prover.rs:216-224, src/training/prover.rs:273-281)
 *   zkp_eval_constraints   ≙ Prover::new_evaluator(..).evaluate(..)
 *                            (src/aggregation/prover.rs:226-233, src/training/prover.rs:283-290)
 *   zkp_composition_commit ≙ Prover::build_constraint_commitment
 *                            (src/aggregation/prover.rs:235-248, src/training/prover.rs:292-300)
 *   zkp_ood_frame          ≙ the OOD frame of generate_proof (trace at z, z*g; composition at z)
 *   zkp_deep_fri           ≙ DeepCompositionPoly + its LDE + FriProver::build_layers / set_remainder
 *   zkp_query              ≙ trace_lde.query, constraint_commitment.query, fri_prover.build_proof
 * (the last three are internal to winterfell 0.12's generate_proof).
 * Calls must come in that order (ZKP_ERR_ARGUMENT otherwise); zkp_query may be
 * repeated. Every value is bit-identical to the matching part of zkp_prove's proof
 * when the caller's channel draws what zkp_prove's transcript draws. One GPU. */
typedef struct zkp_session zkp_session;
int zkp_session_create(zkp_ctx* ctx, zkp_air_id air, uint32_t width, uint64_t n, const zkp_felt* pub_elems,
                       uint64_t n_pub, const zkp_proof_options* opts, zkp_session** out);
/* Releases the session's device buffers (the ctx stays usable). */
void zkp_session_destroy(zkp_session* s);
/* The session's shape as the AIR defines it (each pointer nullable): ce = the
 * constraint-evaluation blowup (zkp_eval_constraints' evals_out holds n*ce values),
 * num_columns = C composition columns, fri_layers = FRI layers before the remainder. */
int zkp_session_shape(const zkp_session* s, uint32_t* ce, uint32_t* num_columns, uint32_t* fri_layers);
/* Host trace (column-major width*n) -> interpolation, coset LDE, row commitment; root out. */
int zkp_session_trace_lde(zkp_session* s, const zkp_felt* trace_cols, uint8_t root[32]);
/* Composition coefficients as the caller's channel drew them (ConstraintCompositionCoefficients:
 * the num_transition transition coefficients, then one per assertion) -> composition
 * evaluations over the CE domain g*<w_{n*ce}> (stay in HBM for zkp_composition_commit;
 * evals_out, nullable, receives the n*ce values in natural domain order). */
int zkp_eval_constraints(zkp_session* s, const zkp_felt* coeffs, uint32_t n_coeffs, zkp_felt* evals_out);
/* CompositionPoly::new (segments into C columns of n coefficients) + LDE + row commitment.
 * evals = NULL: the session's zkp_eval_constraints output; otherwise n*ce host values in
 * natural CE-domain order (e.g. from a CPU evaluator). num_columns (nullable) = C. */
int zkp_composition_commit(zkp_session* s, const zkp_felt* evals, uint8_t root[32], uint32_t* num_columns);
/* OOD frame at z: trace_ood[0..w) = T(z), trace_ood[w..2w) = T(z*w_n); comp_ood[0..C) = H_j(z).
 * z is any canonical element (< p) off the LDE domain: with N = n * blowup, a z with
 * z^N = 3^N has z or z*w_n on the coset 3*<w_N>, where zkp_deep_fri divides by
 * (x - z)(x - z*w_n) at every point x, and is refused with ZKP_ERR_ARGUMENT before
 * anything is launched (the session stays at this stage and takes another z). A point
 * of the trace domain (z = w_n^k) is accepted: the frame is then rows k and k + 1 of
 * the trace. Every challenge of the stage entry points (composition and DEEP
 * coefficients, z, FRI alphas) must be canonical; one >= p is ZKP_ERR_ARGUMENT. */
int zkp_ood_frame(zkp_session* s, zkp_felt z, zkp_felt* trace_ood, zkp_felt* comp_ood);
/* Called once per FRI layer with its Merkle root; returns that layer's alpha in *alpha
 * (a fork binds it to `channel.commit_fri_layer(root); channel.draw_fri_alpha()`); non-zero aborts. */
typedef int (*zkp_fri_channel)(void* user, uint32_t layer, const uint8_t root[32], zkp_felt* alpha);
/* DEEP composition with the caller's coefficients (width + C), then the FRI layers (fold 16)
 * and the remainder polynomial: remainder (nullable; capacity *remainder_len) receives its
 * coefficients, *remainder_len their count, remainder_commitment = hash_elements(remainder). */
int zkp_deep_fri(zkp_session* s, const zkp_felt* deep_coeffs, zkp_fri_channel channel, void* user,
                 zkp_felt* remainder, uint64_t* remainder_len, uint8_t remainder_commitment[32]);
/* Openings at sorted, unique LDE positions (< n*blowup): returns, in zkp_prove's wire
 * format, u8(1) | trace values | trace batch paths | constraint values | constraint batch
 * paths | u8(L) | per FRI layer: values | batch paths. Free with zkp_free. */
int zkp_query(zkp_session* s, const uint64_t* positions, uint64_t n_positions, uint8_t** out, uint64_t* out_len);

/* ---- host channel for stage sessions -------------------------------------
 * ≙ winter-prover 0.12 ProverChannel over DefaultRandomCoin<Blake3_256>, seeded as
 * generate_proof seeds it (Context::to_elements() || pub_inputs.to_elements(), the
 * same seed as zkp_prove's transcript). A winter-prover fork keeps its own channel;
 * a C or Python caller of the session stages draws from this one. Host-only. */
typedef struct zkp_channel zkp_channel;
int zkp_channel_create(zkp_air_id air, uint32_t width, uint64_t n, const zkp_felt* pub_elems, uint64_t n_pub,
                       const zkp_proof_options* opts, zkp_channel** out);
void zkp_channel_destroy(zkp_channel* ch);
/* reseed(root): a commitment (trace, constraint, FRI layer, remainder) */
int zkp_channel_commit(zkp_channel* ch, const uint8_t root[32]);
/* reseed(hash_elements(els)): the OOD frame, trace part (T(z) || T(z*g)) then composition part */
int zkp_channel_commit_felts(zkp_channel* ch, const zkp_felt* els, uint64_t n);
/* count coefficients drawn with `method` (ZKP_BATCHING_*: ConstraintCompositionCoefficients,
 * DeepCompositionCoefficients), or with count = 0 one element (the OOD point z, a FRI alpha) */
int zkp_channel_draw(zkp_channel* ch, uint32_t method, uint32_t count, zkp_felt* out);
/* the coin's seed (the grinding seed for zkp_grind after the remainder commitment) */
int zkp_channel_seed(const zkp_channel* ch, uint8_t seed[32]);
/* query positions: draw_integers(num_queries, n*blowup, nonce), sorted and deduplicated;
 * out holds num_queries values, *n_unique receives the count kept */
int zkp_channel_query_positions(zkp_channel* ch, uint64_t nonce, uint64_t* out, uint32_t* n_unique);

/* ---- verification (≙ winterfell `verify`) ------------------------------ */
/* Status codes of zkp_verify; values map onto winter-verifier `VerifierError`. */
typedef enum zkp_verify_status {
  ZKP_VERIFY_OK = 0,
  ZKP_VERIFY_INCONSISTENT_BASE_FIELD = 32,  /* InconsistentBaseField */
  ZKP_VERIFY_UNACCEPTABLE_OPTIONS = 33,     /* UnacceptableProofOptions */
  ZKP_VERIFY_DESERIALIZATION = 34,          /* ProofDeserializationError */
  ZKP_VERIFY_PUB_INPUTS = 35,               /* public inputs rejected by Air::new */
  ZKP_VERIFY_INCONSISTENT_OOD = 36,         /* InconsistentOodConstraintEvaluations */
  ZKP_VERIFY_TRACE_QUERY = 37,              /* TraceQueryDoesNotMatchCommitment */
  ZKP_VERIFY_CONSTRAINT_QUERY = 38,         /* ConstraintQueryDoesNotMatchCommitment */
  ZKP_VERIFY_POW = 39,                      /* QuerySeedProofOfWorkVerificationFailed */
  ZKP_VERIFY_FRI = 40,                      /* FriVerificationFailed */
  ZKP_VERIFY_RANDOM_COIN = 41               /* RandomCoinError */
} zkp_verify_status;

/* Checks a proof produced by zkp_prove / zkp_prove_sharded against the public
 * inputs (`pub_inputs.to_elements()`) and the one acceptable option set.
 * Replaces `verify::<AIR, Blake3_256<Felt>, DefaultRandomCoin<..>, MerkleTree<..>>(
 * proof, pub_inputs, &AcceptableOptions::OptionSet(vec![options]))` at
 * src/main.rs:251-257, 430-436, 478-484. Host-only: needs no device and no ctx.
 * Returns ZKP_VERIFY_OK, a zkp_verify_status or ZKP_ERR_ARGUMENT. */
int zkp_verify(zkp_air_id air, const uint8_t* proof, uint64_t proof_len, const zkp_felt* pub_elems,
               uint64_t n_pub, const zkp_proof_options* acceptable);

/* ---- trace construction helper ---------------------------------------- */
/* Host-side MiMC AIR trace: out[0] = seed mod p,
 * out[i+1] = (out[i] + K[i % 64])^7 with K[j] = (j+1)*10^6
 * (get_round_constants, src/helper.rs:404-406). Trace building, like
 * `TraceTable` construction in the reference — not part of the proving path. */
int zkp_build_mimc_trace(const uint8_t seed[16], uint64_t n, zkp_felt* out);

/* GlobalUpdateProver::build_trace on the device (src/aggregation/prover.rs:98-160;
 * SURVEY.md §8(f) row 4): writes the 120 x n column-major trace into HBM at
 * d_trace_out (ready for zkp_prove_device). raw_global = flattened raw global
 * model (54 weights then 6 biases), blinding = the 60 masks (prover.rs:68-72),
 * local_updates = ndev x 60 flattened local models (row-major), k = the
 * aggregation factor (pub element 120). Rows: 0 = [masked | 0], 1..ndev =
 * [masked + k^-1 * prefix sum of (local_i - raw) | local_{r-1} - raw],
 * ndev+1.. = [final | 0]. n must be a power of two >= max(8, ndev + 2).
 * final_state (nullable, 60 felts) receives row ndev + 1's masked state, the
 * `new_global` of GlobalUpdateProver::get_pub_inputs (prover.rs:163-190). */
int zkp_build_global_update_trace(zkp_ctx* ctx, const zkp_felt* raw_global, const zkp_felt* blinding,
                                  const zkp_felt* local_updates, uint64_t ndev, zkp_felt k, uint64_t n,
                                  void* d_trace_out, zkp_felt* final_state /* nullable */);

/* TrainingUpdateProver::build_trace on the device (src/training/prover.rs:90-218):
 * writes the 240 x n column-major trace into HBM at d_trace_out (ready for
 * zkp_prove_device). initial_state = the 120 felts of row 0 before masking:
 * [value, sign] pairs, w row-major (6 x 9) then b (6) (prover.rs:98-103); x_batch,
 * x_sign = bs x 9 features and their signs, y_batch = bs x 6 one-hot labels
 * (row-major; unused when bs = 0). The bs signed fixed-point SGD steps
 * (src/signed.rs, src/helper.rs:245-400) run on the device; signs are field
 * elements and any canonical value is taken as the reference's arithmetic takes it.
 * masks = n x 120 u64 in host memory, row t's 120 masks contiguous. Rows: column
 * c < 120 of row t = state_min(t, bs)[c] + masks[t][c], column 120 + c = masks[t][c].
 * n must be a power of two >= 16 and > bs (ZKP_ERR_TRACE_SHAPE otherwise); a felt
 * >= p is ZKP_ERR_ARGUMENT; a learning_rate or precision of 0 is accepted
 * (winterfell inv(0) = 0). first_last (nullable, 240 felts) receives columns 0..119
 * of row 0, then of row n - 1: the `initial_masked` and `final_masked` of
 * TrainingUpdateProver::get_pub_inputs (prover.rs:236-270). raw_states (nullable,
 * (bs + 1) x 120 felts) receives the unmasked state after each sample. */
int zkp_build_training_update_trace(zkp_ctx* ctx, const zkp_felt* initial_state, const zkp_felt* x_batch,
                                    const zkp_felt* x_sign, const zkp_felt* y_batch, uint64_t bs,
                                    zkp_felt learning_rate, zkp_felt precision, const uint64_t* masks, uint64_t n,
                                    void* d_trace_out, zkp_felt* first_last /* nullable */,
                                    zkp_felt* raw_states /* nullable */);

/* The TrainingUpdate traces of all clients of a round in one call: one upload of every
 * client's packed inputs, the K SGD chains side by side in one launch (none for bs = 0),
 * one launch that writes the K traces, one synchronisation. A round has one shape, so bs
 * and n are the batch's; a client carries what zkp_build_training_update_trace takes per
 * trace, with the same meaning, and a mask source of either kind:
 *   masks != NULL: n x 120 u64 in host memory, as the single entry's;
 *   masks == NULL: the masks are the PCG64 stream of (pcg_state, pcg_inc), made on the
 *     device (they are never uploaded): the mask of row t, cell c is value t * 120 + c of
 *       s_0 = state, s_{j+1} = s_j * 0x2360ED051FC65DA44385DF649FCCF645 + inc (mod 2^128),
 *       value e = out(s_{e+1}), out(s) = rotr64((s >> 64) ^ (s mod 2^64), s >> 122)
 *     (zkp_pcg64_masks restates it on the host). With state and inc taken from
 *     numpy.random.default_rng(seed).bit_generator.state["state"], these are the bits of
 *     default_rng(seed).integers(0, 2**64, (n, 120), dtype=uint64). Halves: [0] = the low
 *     64 bits, [1] = the high.
 * Refusals are decided on the host before anything is uploaded or launched, leave the
 * context usable and name the client's index in zkp_last_error: a null clients or required
 * pointer, num_clients of 0 or above ZKP_TU_MAX_CLIENTS, a felt >= p, or two clients whose
 * 240 * n * 16-byte output ranges overlap are ZKP_ERR_ARGUMENT; n and bs follow the single
 * entry's ZKP_ERR_TRACE_SHAPE rules. */
#define ZKP_TU_MAX_CLIENTS 64
typedef struct zkp_training_client {
  const zkp_felt* initial_state;         /* 120 felts */
  const zkp_felt* x_batch;               /* bs x 9 (unused when bs = 0, as x_sign and y_batch) */
  const zkp_felt* x_sign;                /* bs x 9 */
  const zkp_felt* y_batch;               /* bs x 6 */
  zkp_felt learning_rate, precision;
  const uint64_t* masks;                 /* n x 120 host u64, or NULL: pcg_state, pcg_inc */
  uint64_t pcg_state[2], pcg_inc[2];     /* lo, hi; read only when masks is NULL */
  void* d_trace_out;                     /* device: 240 * n * 16 bytes */
  zkp_felt* first_last;                  /* nullable, 240 felts */
  zkp_felt* raw_states;                  /* nullable, (bs + 1) x 120 felts */
} zkp_training_client;
int zkp_build_training_update_traces(zkp_ctx* ctx, const zkp_training_client* clients, uint32_t num_clients,
                                     uint64_t bs, uint64_t n);

/* Values [first_index, first_index + count) of the PCG64 stream of (state, inc) defined
 * above, into out (host only, no context): what the device writes as masks, restated for
 * a fork and for CPU checks. Halves are lo, hi. ZKP_ERR_ARGUMENT for a null pointer. */
int zkp_pcg64_masks(const uint64_t state[2], const uint64_t inc[2], uint64_t first_index, uint64_t count,
                    uint64_t* out);

/* ---- profiling ------------------------------------------------------- */
/* When enabled, every kernel launch is bracketed with HIP events on the
 * stream it runs on; zkp_kernel_stats reports per-kernel launch count and
 * total device milliseconds since the last reset. */
int zkp_set_profiling(zkp_ctx* ctx, int enabled);
/* Restrict the bracketing to launches named `kernel_name` (as in the stats
 * table, e.g. "ntt_dit"); NULL = every launch. Fewer events in a timed region. */
int zkp_set_profiling_kernel(zkp_ctx* ctx, const char* kernel_name /* nullable */);
int zkp_kernel_stats(zkp_ctx* ctx, const char* kernel_name, uint64_t* launches, double* total_ms);
int zkp_reset_stats(zkp_ctx* ctx);
/* Returns a newline-separated "name launches total_ms algorithmic_bytes" table (free with zkp_free). */
int zkp_kernel_stats_table(zkp_ctx* ctx, char** table);

#ifdef __cplusplus
}
#endif
#endif /* ZKP_H */
