"""The option space and the shape thresholds of sharded proofs (zkp_prove_sharded).

A proof over R > 1 ranks picks device and host paths from the options and the shape
that the single-GPU prover never takes; test_gpu_sharded.py reaches them at remainder
degree 7, ALGEBRAIC batching, 30 or 40 queries, grinding on and blowup 8 or 16 only.
The ranks run as threads on one GPU (prove_local_group). Every proving case asserts:
every rank's bytes == the single-GPU proof (ctx.prove) == the oracle's (O.prove), and
both verifiers accept it. The arithmetic is integer: no tolerance. The shapes, and the
thresholds restated in Python, are in sharded_cases.py.

  group  cases                                      branch reached
  -----  -----------------------------------------  ---------------------------------------------
  a      MiMC, FRI_SHAPES x grinding 4, 0           ProofRun::fri_layers (csrc/prover.cpp): a layer
                                                    replicated inside the loop; every layer sharded
                                                    and `if (sh) replicate(L)` after it; one, two and
                                                    three sharded layers; dev_tail with dev_query
                                                    false at a last domain of 16, 64 and 256 (the
                                                    device remainder's limit), the host remainder at
                                                    2048 points and without grinding; remainders of
                                                    1, 8, 32 and 256 coefficients; the smallest n
                                                    that R = 2 and R = 8 accept
         n = 2^17 at R = 2; CHUNKED_TREES           commit_rows_sharded (csrc/prover_shard.cpp):
                                                    logK = 2, a FRI tree and the trace and constraint
                                                    trees exchanged in 4 chunks, at R = 2, 4 and 8
  b      METHOD_PAIRS, GlobalUpdate; the two        k_shard_top's merkle_tail_op (csrc/merkle.hip):
         asymmetric pairs, MiMC, TrainingUpdate     LINEAR and HORNER draws of 180, 3 and 480
                                                    coefficients (480: two strides of its 256 threads)
  c      1, 2, 255 queries x grinding 0, 3          gather_openings over a communicator
                                                    (csrc/prover_stages.cpp): row ownership j / Bl,
                                                    host-side top nodes, the all-gather of every
                                                    rank's openings, dedupe and shared paths; Bl = 1
                                                    on a wide trace with repeated draws
         255 queries, device-resident GlobalUpdate  launch_gu_fill over each rank's share of the rows
  d      blowups 2, 4, 32, 64, 128                  Bl = B >> logR from 1 to 64; CE cosets 1 per 4 to
                                                    64 LDE cosets (ce_owner, ce_first); celmax at
                                                    ce == R (GlobalUpdate and TrainingUpdate, B = R = 2);
                                                    MiMC n = 2048 at B = 32 ends on 256 points as well
         GlobalUpdate, B = 2 at world 4             ProofRun::init: R > B, ZKP_ERR_ARGUMENT on every
                                                    rank before the first collective
  e      MiMC n = 2^14 at R = 8                     ood_launch_sharded at R = 8 with the derived last
                                                    column (composition_gather_lde: the rank's slice
                                                    only); an invalid trace: second attempt on 8 ranks
         traces from a device pointer               zkp_prove_sharded_device: MiMC and TrainingUpdate
                                                    skip gather_host_slices / the column uploads
  f      group a over a counting caller transport   which FRI layers stayed sharded: HostComm, and the
                                                    all_to_all calls of every rank

Where the issue's table and the code disagree, the code's arithmetic wins (ProofRun::init
wants n >= 256 R): B = R = 4 runs at 1024 rows, not 512, for GlobalUpdate and for
TrainingUpdate (batch size 5), and TrainingUpdate's 480 coefficients at R = 8 are drawn at
its smallest 2048-row batch (9), since 512 rows admit R = 2 only. The R > B refusal uses
n = 1024, so that the world is the only thing wrong with it.

Group f's count (sharded_cases.all_to_all_calls, read from commit_rows_sharded and
ProofRun::composition_exchange): one all_to_all for the composition exchange, and for every
sharded tree (trace, constraint, each sharded FRI layer) one per chunk of its leaf exchange,
4 chunks when the tree's logrows - logR >= 12, else 1. Every other collective is an all_gather.

The invalid trace of group e cannot verify: there both verifiers must reject the proof.
The n = 2^17 case, the CHUNKED_TREES cases and the device-resident GlobalUpdate trace at
n = 2^14 are compared with the single-GPU proof only (test_fold16_above_32768_rows,
test_gpu_parity.py and test_gpu_options.py tie those shapes to the oracle).

Not covered: RCCL and anything else that needs more than one process or more than one GPU
(test_gpu_sharded_gloo.py runs one process per rank over gloo); ranks on different devices;
R above 8 or not a power of two in the communicator; folding factors other than 16, which a
group refuses; the rejection redo of a LINEAR draw (test_gpu_options.py)."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import oracle_ref as O
import sharded_cases as S
from option_cases import METHOD_PAIRS, options
from proof_format import sections
from test_gpu_options import gu_inputs, mimc_inputs, tu_inputs
from test_gpu_parity import felts_of
from zk_stark_project_amd import ProofOptions, _native
from zk_stark_project_amd._native import ZkpError, verify_status
from zk_stark_project_amd.field import to_bytes
from zk_stark_project_amd.sharded import prove_local_group

pytestmark = pytest.mark.gpu

GU_UPDATES = 6  # local updates in the GlobalUpdate traces (any n >= 64 holds them)


@pytest.fixture(scope="module")
def rank_ctxs():
    cs = [_native.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


# ---------------------------------------------------------------- inputs and references (once per case)
def inputs_of(kind, size):
    """(air, trace, public inputs): size = n for "mimc" and "global_update", the batch size for "training_update"."""
    if kind == "mimc":
        return mimc_inputs(size)
    if kind == "global_update":
        return gu_inputs(GU_UPDATES, size)
    return tu_inputs(size)


_single = {}


def single_proof(ctx, kind, size, opts):
    key = (kind, size, opts)
    if key not in _single:
        air, trace, pub_el = inputs_of(kind, size)
        _single[key] = ctx.prove(air, trace.data, pub_el, opts)[0]
    return _single[key]


@functools.lru_cache(maxsize=None)
def oracle_proof(kind, size, opts):
    air, trace, pub_el = inputs_of(kind, size)
    return O.prove(air, trace.to_bytes(), trace.data.shape[0], trace.data.shape[1], to_bytes(pub_el), opts)[0]


def check_ranks(results, single):
    for r, (data, _) in enumerate(results):
        assert data == single, f"rank {r} proof differs from the single-GPU proof"


def check_verifiers(air, proof, pub_el, opts, valid=True):
    pub = to_bytes(pub_el)
    ov, pv = O.verify(air, proof, pub, opts), verify_status(air, proof, felts_of(pub), opts)  # oracle, product
    assert (ov == 0 and pv == 0) if valid else (ov != 0 and pv != 0), (ov, pv)


def check_sharded(ctx, rank_ctxs, kind, size, R, opts, oracle=True, device=False):
    """One proof over R ranks, from the host trace or from its copy in HBM: the three assertions."""
    air, trace, pub_el = inputs_of(kind, size)
    w, n = trace.data.shape[:2]
    single = single_proof(ctx, kind, size, opts)
    if device:
        d = ctx.alloc(trace.data.nbytes)
        try:
            ctx.to_device(d, trace.data)
            res = prove_local_group(R, air, d, pub_el, opts, contexts=rank_ctxs[:R], shape=(w, n))
        finally:
            ctx.free(d)
    else:
        res = prove_local_group(R, air, trace.data, pub_el, opts, contexts=rank_ctxs[:R])
    check_ranks(res, single)
    if oracle:
        assert single == oracle_proof(kind, size, opts), "single-GPU proof differs from the oracle"
    check_verifiers(air, single, pub_el, opts)
    return res


# ---------------------------------------------------------------- a. FRI replication, remainder and tail
FRI_CASES = [k for k in S.FRI_SHAPES if k != S.FRI_BIG]


@pytest.mark.parametrize("grind", [4, 0])
@pytest.mark.parametrize("n,R,B,r", FRI_CASES)
def test_fri_replication_and_tail(ctx, rank_ctxs, n, R, B, r, grind):
    """Each row of FRI_SHAPES with grinding (device remainder and first grinding chunk where the
    last domain has <= 256 points, then host positions and gather_openings) and without."""
    L, _, last, _ = S.FRI_SHAPES[(n, R, B, r)]
    res = check_sharded(ctx, rank_ctxs, "mimc", n, R, options(20, B, grind, r))
    proof, tr = res[0]
    assert tr.num_fri_layers == L
    assert len(sections(proof)["remainder"]) == 16 * last // B


def test_three_sharded_layers_chunked_fri_tree(ctx, rank_ctxs):
    n, R, B, r = S.FRI_BIG
    res = check_sharded(ctx, rank_ctxs, "mimc", n, R, options(20, B, 4, r), oracle=False)
    assert res[0][1].num_fri_layers == S.FRI_SHAPES[S.FRI_BIG][0]


@pytest.mark.parametrize("n,R", S.CHUNKED_TREES)
def test_chunked_trace_trees(ctx, rank_ctxs, n, R):
    check_sharded(ctx, rank_ctxs, "mimc", n, R, ProofOptions(40, 8, 12), oracle=False)


# ---------------------------------------------------------------- b. batching methods through k_shard_top
@pytest.mark.parametrize("constraints,deep", METHOD_PAIRS)
def test_batching_methods_global_update(ctx, rank_ctxs, constraints, deep):
    """180 constraint coefficients drawn in k_shard_top."""
    n, B, R = S.GU_METHODS
    check_sharded(ctx, rank_ctxs, "global_update", n, R, options(20, B, 4, 7, constraints, deep))


@pytest.mark.parametrize("constraints,deep", S.ASYMMETRIC_PAIRS)
def test_batching_methods_mimc(ctx, rank_ctxs, constraints, deep):
    """3 constraint coefficients."""
    n, B, R = S.MIMC_METHODS
    check_sharded(ctx, rank_ctxs, "mimc", n, R, options(20, B, 4, 7, constraints, deep))


@pytest.mark.parametrize("constraints,deep", S.ASYMMETRIC_PAIRS)
@pytest.mark.parametrize("bs,n,B,R", S.TU_METHODS)
def test_batching_methods_training_update(ctx, rank_ctxs, bs, n, B, R, constraints, deep):
    """480 constraint coefficients: the HORNER reversal spans two strides of k_shard_top's block."""
    assert inputs_of("training_update", bs)[1].data.shape[1] == n
    check_sharded(ctx, rank_ctxs, "training_update", bs, R, options(20, B, 4, 7, constraints, deep))


# ---------------------------------------------------------------- c. query counts
@pytest.mark.parametrize("grind", S.QUERY_GRINDS)
@pytest.mark.parametrize("q", S.QUERY_COUNTS)
@pytest.mark.parametrize("n,B,R", S.MIMC_QUERIES)
def test_query_count_mimc(ctx, rank_ctxs, n, B, R, q, grind):
    res = check_sharded(ctx, rank_ctxs, "mimc", n, R, options(q, B, grind))
    assert 1 <= res[0][1].num_unique_queries <= q


@pytest.mark.parametrize("grind", S.QUERY_GRINDS)
@pytest.mark.parametrize("q", S.QUERY_COUNTS)
def test_query_count_global_update_one_coset_per_rank(ctx, rank_ctxs, q, grind):
    n, B, R = S.GU_QUERIES
    res = check_sharded(ctx, rank_ctxs, "global_update", n, R, options(q, B, grind))
    assert 1 <= res[0][1].num_unique_queries <= q
    if q == 255:  # 255 draws over 1024 positions: a run without repeats has probability ~ e^-32
        assert res[0][1].num_unique_queries < 255


@pytest.mark.parametrize("n,R", S.GU_FILL)
def test_query_count_255_device_paired_global_update(ctx, rank_ctxs, n, R):
    """A device-resident GlobalUpdate trace is proven paired and lazily: launch_gu_fill fills the
    paired columns of the queried rows that each rank holds."""
    o = ProofOptions.reference()
    check_sharded(ctx, rank_ctxs, "global_update", n, R, options(255, o.blowup_factor, o.grinding_factor),
                  device=True)


# ---------------------------------------------------------------- d. blowup edges
@pytest.mark.parametrize("n,B,R", S.GU_BLOWUPS)
def test_blowup_edges_global_update(ctx, rank_ctxs, n, B, R):
    check_sharded(ctx, rank_ctxs, "global_update", n, R, options(20, B, 4))


@pytest.mark.parametrize("n,B,R", S.MIMC_BLOWUPS)
def test_blowup_edges_mimc(ctx, rank_ctxs, n, B, R):
    check_sharded(ctx, rank_ctxs, "mimc", n, R, options(20, B, 4))


@pytest.mark.parametrize("bs,n,B,R", S.TU_BLOWUPS)
def test_blowup_edges_training_update(ctx, rank_ctxs, bs, n, B, R):
    assert inputs_of("training_update", bs)[1].data.shape[1] == n
    check_sharded(ctx, rank_ctxs, "training_update", bs, R, options(20, B, 4))


def test_world_above_blowup_is_refused(ctx, rank_ctxs):
    """R > B: every rank returns ZKP_ERR_ARGUMENT before its first collective, so none can
    block; the same contexts then prove a sharded case."""
    n, B, R = S.REFUSED_WORLD
    air, trace, pub_el = inputs_of("global_update", n)
    comms = _native.local_group(R)
    codes = [None] * R

    def run(r):
        try:
            rank_ctxs[r].prove_sharded(comms[r], air, trace.data, pub_el, options(20, B, 4))
            codes[r] = 0
        except ZkpError as e:
            codes[r] = e.code

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)  # a refusal returns at once; the limit only turns a hang into a failure
    assert not any(t.is_alive() for t in threads), "a refused rank is still blocked"
    for c in comms:
        c.close()
    assert codes == [S.ERR_ARGUMENT] * R
    check_sharded(ctx, rank_ctxs, "global_update", n, R, options(20, 2 * B, 4))


# ---------------------------------------------------------------- e. OOD split at R = 8, traces from HBM
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ood_split_world8_mimc(ctx, rank_ctxs, device):
    """n = 2^14 at R = 8: the OOD blocks are split, and the derived last composition column
    keeps the rank's slice of its coefficients only."""
    n, R = S.OOD_SPLIT_R8
    check_sharded(ctx, rank_ctxs, "mimc", n, R, ProofOptions(40, 8, 8), device=device)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ood_split_world8_mimc_invalid_trace(ctx, rank_ctxs, device):
    """The `transition` edit of test_mimc_sharded_invalid_trace_lastcol: the dropped-segment
    flags are all-gathered and all 8 ranks prove again without the derived column."""
    n, R = S.OOD_SPLIT_R8
    opts = ProofOptions(40, 8, 8)
    air, trace, pub_el = inputs_of("mimc", n)
    data = np.array(trace.data, copy=True)
    data[0, n // 2 + 9, 0] ^= np.uint64(0x77)
    single, _ = ctx.prove(air, data, pub_el, opts)
    if device:
        d = ctx.alloc(data.nbytes)
        try:
            ctx.to_device(d, data)
            res = prove_local_group(R, air, d, pub_el, opts, contexts=rank_ctxs[:R], shape=(1, n))
        finally:
            ctx.free(d)
    else:
        res = prove_local_group(R, air, data, pub_el, opts, contexts=rank_ctxs[:R])
    check_ranks(res, single)
    ref, _ = O.prove(air, data.tobytes(), 1, n, to_bytes(pub_el), opts)
    assert single == ref, "single-GPU proof differs from the oracle"
    check_verifiers(air, single, pub_el, opts, valid=False)


def test_ood_split_world8_device_paired_global_update(ctx, rank_ctxs):
    """launch_gu_coef derives the paired coefficients over the rank's position slice only."""
    n, R = S.OOD_SPLIT_R8
    check_sharded(ctx, rank_ctxs, "global_update", n, R, ProofOptions.reference(), oracle=False, device=True)


def test_device_trace_mimc(ctx, rank_ctxs):
    n, B, R = S.DEVICE_TRACES["mimc"]
    check_sharded(ctx, rank_ctxs, "mimc", n, R, options(20, B, 4), device=True)


def test_device_trace_training_update(ctx, rank_ctxs):
    bs, n, B, R = S.DEVICE_TRACES["training_update"]
    assert inputs_of("training_update", bs)[1].data.shape[1] == n
    check_sharded(ctx, rank_ctxs, "training_update", bs, R, options(20, B, 4), device=True)


# ---------------------------------------------------------------- f. the FRI cases reach their path
class CountingGroup:
    """The ranks of one process over the caller transport (_native.host_comm): a collective
    publishes the rank's pinned send buffer, meets the others at a barrier, copies its blocks
    out of theirs, and meets them again before any buffer is reused. Counts every rank's calls.
    A rank that fails aborts the barrier (the transport's abort), so its peers fail too."""
    WAIT = 120  # seconds: no collective waits that long unless a rank is lost

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.sent = [None] * world
        self.calls = [{"all_to_all": 0, "all_gather": 0} for _ in range(world)]

    def comm(self, r):
        def collective(name, a2a):
            def cb(send, recv, nbytes):
                self.calls[r][name] += 1
                self.sent[r] = send
                self.barrier.wait(self.WAIT)
                for s in range(self.world):
                    if nbytes:
                        ctypes.memmove(recv + s * nbytes, self.sent[s] + (r * nbytes if a2a else 0), nbytes)
                self.barrier.wait(self.WAIT)
            return cb
        return _native.host_comm(r, self.world, collective("all_to_all", True), collective("all_gather", False),
                                 abort=self.barrier.abort)

    def prove(self, contexts, air, trace, pub, opts):
        comms = [self.comm(r) for r in range(self.world)]
        results, errors = [None] * self.world, [None] * self.world

        def run(r):
            try:
                results[r] = contexts[r].prove_sharded(comms[r], air, trace, pub, opts)
            except Exception as e:  # noqa: BLE001 — re-raised below
                errors[r] = e

        threads = [threading.Thread(target=run, args=(r,)) for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for c in comms:
            c.close()
        for e in errors:
            if e is not None:
                raise e
        return results


@pytest.mark.parametrize("grind", [4, 0])
@pytest.mark.parametrize("n,R,B,r", FRI_CASES)
def test_fri_cases_exchange_counts(ctx, rank_ctxs, n, R, B, r, grind):
    """The proof bytes again, over HostComm, and the all_to_all calls of every rank: each
    sharded FRI layer adds its tree's leaf exchange (sharded_cases.all_to_all_calls)."""
    opts = options(20, B, grind, r)
    air, trace, pub_el = inputs_of("mimc", n)
    grp = CountingGroup(R)
    res = grp.prove(rank_ctxs[:R], air, trace.data, pub_el, opts)
    check_ranks(res, single_proof(ctx, "mimc", n, opts))
    expected = S.FRI_SHAPES[(n, R, B, r)][3]
    assert [c["all_to_all"] for c in grp.calls] == [expected] * R
    assert len({c["all_gather"] for c in grp.calls}) == 1  # the same program on every rank
