"""Independent contexts proving at once from several host threads.

INTEGRATION.md §2a: calls on different contexts may run on different threads at once, and
the bytes are those of the sequential calls. Every other GPU test that uses threads drives
the ranks of one sharded proof; here each thread owns a context that it created itself and
the threads meet at a barrier before every step, so step i of every thread starts together.
What the contexts share is process-wide: the stream pool a closed context feeds
(csrc/prover.cpp), the once-per-device attribute block of launch_ntt and the lazy load of
the code objects (csrc/ntt.hip), the registry of AIR programs (csrc/air_program.hpp), and
the allocator under zkp_ctx_destroy / zkp_ctx_trim. What they must not share is per
context: the named device buffers, the pinned staging block and upload ring, the cached
program image, the statistics table and the last-error text.

Every step is one of the existing steps of test_gpu_context_reuse.py, test_gpu_wide_programs.py
and test_gpu_session_challenges.py, or an entry compared as its own test compares it, against
the same reference: the CPU oracle's bytes, stage_reference.py, the bound program's proof, the
host trace check. Exact comparisons only. Every reference is computed on the main thread
before the threads start (Step.prepare): the lru_cache'd makers are not entered concurrently
and the CPU oracle does not run beside the GPU steps. Rounds are fixed; nothing is retried.

Not covered, because not promised: one context, or sessions of one parent context, used from
two threads at once."""
import collections
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import oracle_ref as O
from air_params_cases import ZKP_ERR_UNSUPPORTED_AIR, pub_strided_instance, pub_strided_program
from air_program_cases import mimc_program, power_program, power_trace, trace_array
from challenge_cases import SHAPES, layers as shape_layers
from concurrent_cold import COLD_PROOFS
from folding_cases import options
from test_gpu_air_params import bound_proof
from test_gpu_context_reuse import (ZKP_ERR_INVALID_OPTIONS, ZKP_ERR_TRACE_SHAPE, builtin, mimc_strided_step,
                                    options_key, oracle_proof, power_reference, power_step, wide)
from test_gpu_options import gu_inputs, mimc_inputs
from test_gpu_parity import gu_prover, rand_trace
from test_gpu_session_challenges import felts, reference as session_reference, run_session as oracle_session, shape_inputs
from test_gpu_training_traces_batch import make_provers
from test_gpu_wide_programs import check_program_proof, fresh_context, structured_reference
from wide_program_cases import CASES, case_inputs, case_options, case_reference
from zk_stark_project_amd import (AIR_GLOBAL_UPDATE, AIR_MIMC, AIR_TRAINING_UPDATE, InvalidTrace, TrainingUpdateProver,
                                  _native)
from zk_stark_project_amd._native import ZkpError, verify_status
from zk_stark_project_amd.field import P, to_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFY_PUB_INPUTS = 35

# A barrier wait ends after this many seconds. Measured on an MI355X: the whole list of 23 step
# kinds takes 1.3 s on four threads, so no step takes more than a few tenths of a second alone
# or beside seven others; ten times that lies below the floor of 60 s.
BARRIER_TIMEOUT = 60.0

# A step: run(ctx) proves and compares; prepare() computes its references (main thread, once).
Step = collections.namedtuple("Step", "name run prepare")
_prepared = set()


def prepare(steps):
    for s in steps:
        if s is not None and s.name not in _prepared:
            s.prepare()
            _prepared.add(s.name)


def run_lockstep(sequences, timeout=BARRIER_TIMEOUT):
    """One thread per sequence, each with a fresh Context created inside the thread; a barrier
    before every step index. None in a sequence: the thread only waits at that barrier.
    A step that raises aborts the barrier, so the other threads stop at their next one.
    Every exception is re-raised here, on the main thread, with its thread and step number."""
    count = len(sequences[0])
    assert all(len(s) == count for s in sequences)
    prepare([s for seq in sequences for s in seq])
    barrier = threading.Barrier(len(sequences))
    errors, lock = [], threading.Lock()

    def worker(t, steps):
        ctx, i = None, -1
        try:
            ctx = _native.Context(0)
            for i, step in enumerate(steps):
                barrier.wait(timeout)
                if step is not None:
                    step.run(ctx)
        except threading.BrokenBarrierError:
            pass  # another thread failed (or a wait ran out: reported below)
        except BaseException as e:  # noqa: BLE001 — re-raised on the main thread
            with lock:
                errors.append((t, i, steps[i].name if 0 <= i < count and steps[i] else "context", e))
            barrier.abort()
        finally:
            if ctx is not None:
                ctx.close()

    threads = [threading.Thread(target=worker, args=(t, seq), daemon=True) for t, seq in enumerate(sequences)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout * (count + 1))
    alive = [t for t, th in enumerate(threads) if th.is_alive()]
    assert not alive, f"threads {alive} did not finish"
    if errors:
        text = "; ".join(f"thread {t}, step {i + 1} of {count} ({name}): {type(e).__name__}: {e}"
                         for t, i, name, e in sorted(errors, key=lambda x: x[:2]))
        raise AssertionError(text) from errors[0][3]
    assert not barrier.broken, "a barrier wait ran out of time"


# ---------------------------------------------------------------- step kinds
def proof_step(name, kind, *args, opts):
    return Step(name, builtin(kind, *args, opts=opts), lambda: oracle_proof(kind, args, options_key(opts)))


def case(w, d, n, blowup):
    return next(c for c in CASES if (c.w, c.d, c.n, c.blowup) == (w, d, n, blowup))


def wide_step(name, w, d, n, blowup, session=False):
    c = case(w, d, n, blowup)

    def ready():
        case_inputs(c)
        case_reference(c)
        if session:
            structured_reference(c)
    return Step(name, wide(w, d, n, blowup, session=session), ready)


def gu_device_step(ndev, n, opts):
    """build_global_update_trace on the device, prove_device of it: the host trace's oracle bytes."""
    def run(ctx):
        p = gu_prover(ndev, n, options(20, 16, 4), seed=ndev)  # gu_inputs' prover, made again: it keeps state
        d = p.build_trace_device(ctx)
        try:
            pub = tuple(p.get_pub_inputs().to_elements())
            assert pub == gu_inputs(ndev, n)[2]
            gpu, _ = ctx.prove_device(AIR_GLOBAL_UPDATE, d, 120, n, pub, opts)
        finally:
            ctx.free(d)
        assert gpu == oracle_proof("global_update", (ndev, n), options_key(opts))
    return Step(f"gu_device_{ndev}_{n}", run, lambda: oracle_proof("global_update", (ndev, n), options_key(opts)))


TU_BATCH = dict(bs=1, n=128, count=2, seed0=7000)
_tu_batch_refs = []


def tu_batch_step(opts):
    """build_training_update_traces for two clients, then prove_device of each: the oracle's
    bytes for each client's host trace."""
    bs, n, count, seed0 = (TU_BATCH[k] for k in ("bs", "n", "count", "seed0"))

    def ready():
        for p in make_provers(bs, n, count, seed0, options=opts):
            t = p.build_trace()
            pub = tuple(p.get_pub_inputs(t).to_elements())
            _tu_batch_refs.append((pub, O.prove(AIR_TRAINING_UPDATE, t.to_bytes(), 240, n, to_bytes(pub), opts)[0]))

    def run(ctx):
        provers = make_provers(bs, n, count, seed0, options=opts)  # made again: they keep the device rows
        ptrs = TrainingUpdateProver.build_traces_device(provers, ctx)
        try:
            for k, (p, d) in enumerate(zip(provers, ptrs)):
                pub = tuple(p.get_pub_inputs().to_elements())
                assert pub == _tu_batch_refs[k][0], f"client {k} public inputs"
                gpu, _ = ctx.prove_device(AIR_TRAINING_UPDATE, d, 240, n, pub, opts)
                assert gpu == _tu_batch_refs[k][1], f"client {k}"
        finally:
            ctx.free(ptrs[0])
    return Step("tu_batch_2_clients", run, ready)


PUB_N, PUB_CONSTANTS = 16, (5, 300)
_pub_refs = []


def pub_program():
    return pub_strided_program(PUB_N, [(0, 1, 4), (1, 0, 2)], [(2, 1, 2)])


def pub_instances_step():
    """One program with public inputs, two instances under one id, and the first again: each the
    proof of the instance's bound program (test_gpu_air_params.bound_proof, made beforehand)."""
    opts = options(20, 4, 4)

    def ready():
        p = pub_program()
        with fresh_context() as ctx:
            for c in PUB_CONSTANTS:
                cols, pub = pub_strided_instance(p, PUB_N, c)
                _pub_refs.append((trace_array(cols), pub, bound_proof(ctx, p, trace_array(cols), pub, opts)[0]))
        assert _pub_refs[0][2] != _pub_refs[1][2]

    def run(ctx):
        with pub_program().register() as air:
            for data, pub, want in _pub_refs + _pub_refs[:1]:
                gpu, _ = ctx.prove(air, data, pub, opts)
                assert gpu == want
                assert verify_status(air, gpu, pub, opts) == 0
    return Step("pub_two_instances", run, ready)


_session_refs = {}


def channel_replay(name, st, sec):
    """The host channel over the session's commitments draws what the oracle's coin drew."""
    air, _, pub_el, opts, sp = shape_inputs(name)
    com, L = sec["commitments"], shape_layers(sp)
    ch = _native.Channel(air, sp.w, sp.n, list(pub_el), opts)
    try:
        ch.commit(com[0:32])
        assert ch.draw_coeffs(opts.batching_constraints, sp.num_t + sp.num_a) == felts(st["coeffs"])
        ch.commit(com[32:64])
        assert ch.draw() == st["z"]
        ch.commit_felts(felts(sec["ood_trace"]))
        ch.commit_felts(felts(sec["ood_comp"]))
        assert ch.draw_coeffs(opts.batching_deep, sp.w + sp.C) == felts(st["deep_coeffs"])
        alphas = felts(st["alphas"])
        for layer in range(L):
            ch.commit(com[64 + 32 * layer:96 + 32 * layer])
            assert ch.draw() == alphas[layer]
        ch.commit(com[-32:])
        assert ch.query_positions(sec["nonce"]) == st["positions"]
    finally:
        ch.close()


def session_step(name):
    """A stage session of SHAPES[name] driven with the oracle's own challenges, every stage
    against the oracle; then the host channel replayed over what the session committed."""
    assert name in SHAPES

    def ready():
        shape_inputs(name)
        _session_refs[name] = session_reference(name)

    def run(ctx):
        _, st, sec = oracle_session(ctx, name, {}, ref=_session_refs[name])
        channel_replay(name, st, sec)
    return Step(f"session_{name}", run, ready)


_small_refs = {}
LDE_SHAPE, ROWS_SHAPE, GRIND_BITS = (3, 256, 4), (65, 16), 8
GRIND_SEED = bytes(range(32))


def lde_commit_step():
    w, n, blowup = LDE_SHAPE
    tr = rand_trace(w, n, seed=w * 1000 + n)

    def run(ctx):
        lde, root = ctx.trace_lde_commit(tr, blowup)
        assert lde.tobytes() == _small_refs["lde"][0] and root == _small_refs["lde"][1]
    return Step("trace_lde_commit", run, lambda: _small_refs.update(lde=O.trace_lde(tr.tobytes(), w, n, blowup)))


def merkle_rows_step():
    w, rows = ROWS_SHAPE
    m = rand_trace(w, rows, seed=rows + w)

    def run(ctx):
        assert ctx.merkle_commit_rows(m) == _small_refs["rows"]
    return Step("merkle_commit_rows", run, lambda: _small_refs.update(rows=O.merkle_rows(m.tobytes(), w, rows)))


def grind_step():
    def run(ctx):
        assert ctx.grind(GRIND_SEED, GRIND_BITS) == _small_refs["grind"]
    return Step("grind_8_bits", run, lambda: _small_refs.update(grind=O.grind(GRIND_SEED, GRIND_BITS)))


def check_trace_step():
    """check_trace_device on a valid and on an invalid trace of a registered program: the host check's tuple."""
    d, n = 5, 64
    good = trace_array(power_trace(d, n))
    bad = np.array(good, copy=True)
    bad[1, 37, 0] ^= np.uint64(1)

    def ready():
        with power_program(d, n).register() as prog:
            _small_refs["check"] = (prog.check_trace(good), prog.check_trace(bad))
        assert _small_refs["check"][0] is None and _small_refs["check"][1] is not None

    def run(ctx):
        with power_program(d, n).register() as prog:
            assert (ctx.check_trace(prog, good), ctx.check_trace(prog, bad)) == _small_refs["check"]
    return Step("check_trace_device", run, ready)


O8, O16 = options(20, 8, 4), options(20, 16, 4)
MIMC_64 = proof_step("mimc_64", "mimc", 64, opts=O8)                                   # radix-2 NTT (logn < 11)
MIMC_2K = proof_step("mimc_2^11", "mimc", 1 << 11, opts=O8)                            # the smallest k_ntt8 shape
MIMC_16K_FUSED = proof_step("mimc_2^14_fused_tail", "mimc", 1 << 14, opts=options(20, 16, 4, 7, 4))
MIMC_16K_UNFUSED = proof_step("mimc_2^14_host_tail", "mimc", 1 << 14, opts=options(20, 16, 0, 7, 4))
GU_6_64 = proof_step("gu_6_64", "global_update", 6, 64, opts=O8)
GU_30_256 = proof_step("gu_30_256", "global_update", 30, 256, opts=O16)
TU_1 = proof_step("tu_bs1", "training_update", 1, opts=O8)
TU_3 = proof_step("tu_bs3", "training_update", 3, opts=O8)
WIDE_A = wide_step("wide_16_5_8_8", 16, 5, 8, 8)
WIDE_B = wide_step("wide_33_9_16_16", 33, 9, 16, 16)
SESSION_MIMC = session_step("mimc_f2")

KINDS = [
    MIMC_64, MIMC_2K, MIMC_16K_FUSED, MIMC_16K_UNFUSED, GU_6_64, GU_30_256, gu_device_step(6, 64, O8), TU_1, TU_3,
    tu_batch_step(O8), WIDE_A, WIDE_B, wide_step("wide_16_5_8_8_session", 16, 5, 8, 8, session=True),
    Step("power_5", power_step(5, 64, 8), lambda: power_reference(5, 64, 8)),
    Step("power_3", power_step(3, 64, 8), lambda: power_reference(3, 64, 8)),
    Step("mimc_strided", mimc_strided_step(64, 8), lambda: oracle_proof("mimc", (64,), options_key(O8))),
    pub_instances_step(), SESSION_MIMC, session_step("global_update"), lde_commit_step(), merkle_rows_step(),
    grind_step(), check_trace_step(),
]


# ---------------------------------------------------------------- 1. every kind beside every other
def rotation(kinds, threads, reverse):
    """Thread t starts at offset t * K / threads and walks the list forwards (or backwards)."""
    K = len(kinds)
    return [[kinds[(t * K // threads + (-i if reverse else i)) % K] for i in range(K)] for t in range(threads)]


@pytest.mark.parametrize("reverse", [False, True], ids=["forwards", "reversed"])
def test_every_kind_beside_every_other(reverse):
    K = len(KINDS)
    assert K >= 8 and len({s.name for s in KINDS}) == K
    sequences = rotation(KINDS, 4, reverse)
    beside = collections.defaultdict(set)
    for i in range(K):
        at_barrier = [seq[i].name for seq in sequences]
        assert len(set(at_barrier)) == 4, f"barrier {i}: {at_barrier}"  # four different kinds at every barrier
        for name in at_barrier:
            beside[name] |= set(at_barrier) - {name}
    for seq in sequences:
        assert sorted(s.name for s in seq) == sorted(s.name for s in KINDS)  # every thread runs every kind once
    assert all(len(beside[s.name]) >= 3 for s in KINDS)
    run_lockstep(sequences)


# ---------------------------------------------------------------- 2. the same step on every context
@pytest.mark.parametrize("contexts", [4, 8])
def test_same_step_on_every_context(contexts):
    """Equal table keys, shapes and one registered id on every context at every barrier."""
    c = case(16, 5, 8, 8)
    program, cols, pub = case_inputs(c)
    with program.register() as prog:
        shared_wide = Step("wide_16_5_8_8_one_id",
                           lambda ctx: check_program_proof(ctx, prog, case_reference(c), trace_array(cols), pub,
                                                           case_options(c)),
                           lambda: case_reference(c))
        run_lockstep([[MIMC_2K, GU_30_256, shared_wide, SESSION_MIMC]] * contexts)


# ---------------------------------------------------------------- 3. context churn
CHURN_ROUNDS, BURST_ROUNDS, TRIM_ROUND = 12, (3, 9), 6


def test_context_churn():
    """Two threads prove; a third opens a context, proves on it and closes it, twelve times.
    The pool keeps at most STREAM_POOL_MAX = 4 idle stream sets per device: it is filled before
    the threads start, so a context opened while the others prove takes a pooled set; in two
    rounds the third thread holds four more contexts and closes all five, so the closes find
    the pool both with room (the set is kept) and full (the streams are destroyed) while the
    neighbours have work queued. Once it proves, trims and proves on its live context, with an
    idle stage-session context to free. Eight contexts at the most are open at once."""
    prepare([MIMC_64, GU_6_64, SESSION_MIMC])
    for c in [_native.Context(0) for _ in range(5)]:
        c.close()

    def churn(i):
        def run(ctx):
            extra = [_native.Context(0) for _ in range(4)] if i in BURST_ROUNDS else []
            try:
                with fresh_context() as own:
                    MIMC_64.run(own)
                    if i in BURST_ROUNDS:
                        GU_6_64.run(extra[-1])
            finally:
                for c in extra:
                    c.close()
            if i == TRIM_ROUND:
                SESSION_MIMC.run(ctx)  # leaves an idle session context on ctx
                MIMC_64.run(ctx)
                ctx.trim()
                MIMC_64.run(ctx)
        return Step(f"churn_{i}", run, lambda: None)
    provers = [[(MIMC_64, GU_6_64)[(i + t) % 2] for i in range(CHURN_ROUNDS)] for t in range(2)]
    run_lockstep(provers + [[churn(i) for i in range(CHURN_ROUNDS)]])


# ---------------------------------------------------------------- 4. registry churn
REGISTRY_PROGRAMS = [(d, n) for n in (16, 32) for d in (2, 3, 4, 5, 6)]  # ten distinct programs, blowup 8


def test_registry_churn():
    """One thread registers a program, proves with it, verifies and unregisters, ten times,
    while two others prove under ids registered before the start."""
    opts = options(20, 8, 4)
    for d, n in REGISTRY_PROGRAMS:
        power_reference(d, n, 8)
    power_reference(5, 64, 8)
    c = case(16, 5, 8, 8)
    program, wcols, wpub = case_inputs(c)
    case_reference(c)
    ids = []

    def program_proof(ctx, prog, d, n):
        cols = power_trace(d, n)
        return check_program_proof(ctx, prog, power_reference(d, n, 8), trace_array(cols),
                                   (cols[0][0], cols[1][n - 1]), opts)[0]

    def churn(d, n):
        def run(ctx):
            cols = power_trace(d, n)
            pub = (cols[0][0], cols[1][n - 1])
            prog = power_program(d, n).register()
            try:
                ids.append(prog.AIR_ID)
                proof = program_proof(ctx, prog, d, n)  # the verifier accepts it (check_program_proof)
            finally:
                prog.close()
            # the context has this id's image cached: the freed id is refused all the same
            assert verify_status(ids[-1], proof, pub, opts) == VERIFY_PUB_INPUTS
            with pytest.raises(ZkpError) as e:
                ctx.prove(ids[-1], trace_array(cols), pub, opts)
            assert e.value.code == ZKP_ERR_UNSUPPORTED_AIR
        return Step(f"register_power_{d}_{n}", run, lambda: None)

    with power_program(5, 64).register() as live, program.register() as wide_prog:
        first_id = max(live.AIR_ID, wide_prog.AIR_ID)
        power = Step("power_5_live_id", lambda ctx: program_proof(ctx, live, 5, 64), lambda: None)
        wide_live = Step("wide_live_id",
                         lambda ctx: check_program_proof(ctx, wide_prog, case_reference(c), trace_array(wcols), wpub,
                                                         case_options(c)), lambda: None)
        rounds = len(REGISTRY_PROGRAMS)
        # the churning context's own next proof under a live id, after the last refusal
        run_lockstep([[churn(d, n) for d, n in REGISTRY_PROGRAMS] + [power],
                      [power] * (rounds + 1), [wide_live] * (rounds + 1)])
    assert len(ids) == rounds and ids[0] > first_id
    assert all(b > a for a, b in zip(ids, ids[1:])), ids  # strictly increasing: never handed out twice


# ---------------------------------------------------------------- 5. failures beside successes
MIMC_EDITS = ["transition", "last_row", "wrong_result", "wrong_start"]  # test_gpu_parity's invalid MiMC traces
_refusal_refs = {}


def invalid_mimc(edit, n=64):
    """-> (the MiMC program's pub, the trace) of one of test_gpu_parity's invalid-trace edits."""
    _, trace, pub = mimc_inputs(n)
    pub, data = list(pub), np.array(trace.data, copy=True)
    if edit == "transition":
        data[0, 5, 0] ^= np.uint64(0x5A5A)
    elif edit == "last_row":
        data[0, n - 1, 0] ^= np.uint64(0x5A5A)
    elif edit == "wrong_result":
        pub[1] = (pub[1] + 1) % P
    else:
        pub[0] = (pub[0] + 7) % P
    return pub, data


def refusals():
    """name -> callable(ctx) that makes one refused call and returns what identifies the refusal."""
    def invalid(edit):
        def call(ctx):
            pub, data = invalid_mimc(edit)
            with mimc_program(64, pub).register() as prog, pytest.raises(InvalidTrace) as e:
                ctx.prove(prog, data, pub, O8, validate=True)
            return (e.value.row, e.value.constraint, e.value.assertion)
        return call

    def bad_options(ctx):
        _, trace, pub = mimc_inputs(64)
        with pytest.raises(ZkpError) as e:  # blowup 4 below MiMC's ce = 8
            ctx.prove(AIR_MIMC, trace.data, pub, options(20, 4, 4))
        assert e.value.code == ZKP_ERR_INVALID_OPTIONS
        return str(e.value)

    def bad_shape(ctx):
        with pytest.raises(ZkpError) as e:  # 256 columns
            ctx.trace_lde_commit(np.zeros((256, 8, 2), dtype=np.uint64), 2, want_lde=False)
        assert e.value.code == ZKP_ERR_TRACE_SHAPE
        return str(e.value)
    out = {f"invalid_{edit}": invalid(edit) for edit in MIMC_EDITS}
    out.update(bad_options=bad_options, bad_shape=bad_shape)
    return out


def refusal_step(name):
    call = refusals()[name]

    def run(ctx):
        assert call(ctx) == _refusal_refs[name]
    return Step(name, run, lambda: None)


def unpaired_gu_step():
    """GlobalUpdate (30, 256) with a paired column broken at row 5: prove_impl finds the pairing
    check failed and proves again unpaired; the bytes are the oracle's for that trace."""
    _, trace, pub = gu_inputs(30, 256)
    data = np.array(trace.data, copy=True)
    data[61, 5, 0] ^= np.uint64(0x5A5A)

    def ready():
        _refusal_refs["unpaired"] = O.prove(AIR_GLOBAL_UPDATE, data.tobytes(), 120, 256, to_bytes(pub), O16)[0]
        assert O.verify(AIR_GLOBAL_UPDATE, _refusal_refs["unpaired"], to_bytes(pub), O16) != 0

    def run(ctx):
        assert ctx.prove(AIR_GLOBAL_UPDATE, data, pub, O16)[0] == _refusal_refs["unpaired"]
    return Step("gu_unpaired_retry", run, ready)


def test_failures_beside_successes():
    """Two threads alternate refused calls with valid proofs, in different orders, so that at a
    barrier where both are refused they are refused for different reasons; two neighbours prove
    throughout. Every refusal gives what the same call gives alone on a fresh context: the
    InvalidTrace position, or the status with that context's own zkp_last_error text."""
    prepare([MIMC_64, MIMC_2K, GU_6_64, GU_30_256])
    with fresh_context() as ctx:
        for name, call in refusals().items():
            _refusal_refs[name] = call(ctx)
        assert _refusal_refs["bad_options"] != _refusal_refs["bad_shape"]
        # the ABI's text, not only the binding's prefix
        for name in ("bad_options", "bad_shape"):
            assert _refusal_refs[name].split(": ", 2)[2], _refusal_refs[name]
    # bad_shape came after bad_options on that context; alone on another its text is the same
    # (this file found the entries of csrc/abi.cpp reporting the text an earlier refused call left)
    with fresh_context() as ctx:
        assert refusals()["bad_shape"](ctx) == _refusal_refs["bad_shape"]
    assert len({_refusal_refs[f"invalid_{e}"] for e in MIMC_EDITS}) >= 3
    R = {name: refusal_step(name) for name in refusals()}
    unpaired = unpaired_gu_step()
    first = [R["bad_options"], MIMC_64, R["invalid_transition"], MIMC_64, R["bad_shape"], GU_6_64, unpaired, GU_6_64,
             R["invalid_last_row"], MIMC_64, R["invalid_wrong_result"], MIMC_2K, R["invalid_wrong_start"], MIMC_64]
    second = [R["bad_shape"], GU_6_64, R["bad_options"], MIMC_2K, R["invalid_wrong_start"], MIMC_64, R["bad_options"],
              unpaired, R["invalid_transition"], GU_6_64, R["bad_shape"], MIMC_64, R["invalid_last_row"], GU_6_64]
    assert len(first) == len(second)
    assert all(a.name != b.name for a, b in zip(first, second))
    rounds = len(first)
    run_lockstep([first, second, [(MIMC_2K, GU_30_256)[i % 2] for i in range(rounds)],
                  [(GU_30_256, MIMC_2K)[i % 2] for i in range(rounds)]])


# ---------------------------------------------------------------- 6. profiling stays per context
def test_profiling_stays_per_context():
    """The launch counts of MiMC 2^11 on a profiled context beside three proving neighbours equal
    those of the same proof alone on a fresh context. Counts only, never times."""
    counts = {}

    def profiled(key):
        def run(ctx):
            ctx.set_profiling(True)
            ctx.reset_stats()
            MIMC_2K.run(ctx)
            counts[key] = {k: v["launches"] for k, v in ctx.stats_table().items()}
            ctx.set_profiling(False)
        return Step(f"profiled_{key}", run, lambda: None)
    prepare([MIMC_2K, GU_30_256, WIDE_A, TU_1])
    with fresh_context() as ctx:
        profiled("alone").run(ctx)
    run_lockstep([[profiled("beside")], [GU_30_256], [WIDE_A], [TU_1]])
    assert counts["alone"] and sum(counts["alone"].values()) > 10
    assert counts["beside"] == counts["alone"]


# ---------------------------------------------------------------- 7. cold start in a fresh process
MEASURED_S = 0.72  # python tests/concurrent_cold.py DIR --sequential on an MI355X, wall time of the process
COLD_TIMEOUT_S = max(60.0, 10 * MEASURED_S)


def test_cold_start_in_a_fresh_process(tmp_path):
    """A child process (tests/concurrent_cold.py) creates four contexts on four threads; each
    context's first call is a different MiMC proof with logn >= 11, so the process's first NTT
    launches meet in launch_ntt's attribute block and in the lazy load of the code objects.
    The oracle's bytes are computed before the child starts; the parent does not touch the
    GPU while it runs. The child's time limit: the same four proofs one after another in a
    fresh process, start-up included, took 0.72 s (MEASURED_S; the child itself takes 0.67 s);
    times ten, and at least 60 s, gives 60 s."""
    want = [oracle_proof("mimc", (n,), options_key(options(20, blowup, 4))) for n, blowup in COLD_PROOFS]
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "concurrent_cold.py"), str(tmp_path)],
                       capture_output=True, text=True, timeout=COLD_TIMEOUT_S)
    print(f"cold child: {time.perf_counter() - t0:.2f} s")
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    for i, ref in enumerate(want):
        got = (tmp_path / f"proof_{i}.bin").read_bytes()
        assert got == ref, f"proof {i} {COLD_PROOFS[i]}"

