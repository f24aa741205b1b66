"""zkp_air_constraint_degrees_device: every transition constraint's actual degree on a trace,
measured on the GPU (k_program_columns, the composition's interpolation route, k_column_degrees).

Every expected degree is the big-int reference's (constraint_degree_cases.reference_degrees);
the closed forms are asserted beside it, here and on the reference alone in
test_constraint_degrees_abi.py. The other report fields follow from the degrees by the header's
formulas (expected_report)."""
import os
import subprocess
import threading

import pytest

import constraint_degree_cases as C
from air_program_cases import trace_array
from test_gpu_wide_programs import run_session
from wide_program_cases import CASES, case_inputs, case_options, deep_cases
from zk_stark_project_amd import (AIR_GLOBAL_UPDATE, AIR_MIMC, AIR_TRAINING_UPDATE, DegreeMismatch, ProofOptions,
                                  _native)
from zk_stark_project_amd._native import ZkpError, verify_status

pytestmark = pytest.mark.gpu
NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
ZKP_ERR_TRACE_SHAPE, ZKP_ERR_PUB_INPUTS, ZKP_ERR_UNSUPPORTED_AIR, ZKP_ERR_ARGUMENT = 3, 4, 8, 9
OPTS = ProofOptions(20, 8, 4)


def fields(rep):
    return {"eval_blowup": rep.eval_blowup, "columns": rep.columns, "columns_needed": rep.columns_needed,
            "max_degree": rep.max_degree, "first_under": rep.first_under, "proof_fits": rep.proof_fits}


def measure(ctx, kind, *args):
    """The case's DegreeReport on the GPU, checked against the reference; -> (report, program, cols)."""
    program, cols, want = C.reference(kind, *args)
    pub = list(args[-1]) if kind == "pub" else None
    n = len(cols[0])
    rep = program.constraint_degrees(ctx, trace_array(cols), pub)
    print(kind, args[:2], "actual", rep.actual[:8], fields(rep))
    assert rep.actual == want
    assert rep.declared == [d for _, d in program.constraints]
    assert fields(rep) == C.expected_report(program, n, want)
    assert rep.minimal == [1 if a is None else max(1, -(-a // (n - 1))) for a in want]
    return rep, program, cols


# ---------------------------------------------------------------- 1. powers
@pytest.mark.parametrize("n", C.POWER_LENGTHS)
@pytest.mark.parametrize("d", C.POWERS)
def test_powers(ctx, d, n):
    """next - cur^d on its valid trace: d (n - 1), E = 2 .. 32 on both sides of each power of two.
    d = 1: the valid trace is constant and the constraint the zero polynomial (power_closed_form);
    its random column gives n - 1. n dividing d - 1 (d = 9, 17 at n = 8): no proof of the shape
    exists and the entry returns ZKP_ERR_PUB_INPUTS like every other entry."""
    if C.no_proof_shape(d, n):
        program, cols = C.power_case(d, n)
        with pytest.raises(ZkpError) as e:
            program.constraint_degrees(ctx, trace_array(cols))
        assert e.value.code == ZKP_ERR_PUB_INPUTS
        return
    rep, _, _ = measure(ctx, "power", d, n)
    assert rep.actual == C.power_closed_form(d, n) and rep.eval_blowup == C.domain_factor(d)
    assert rep.proof_fits and rep.first_under is None and rep.under == []
    if d * (n - 1) - (n - 1) + 1 > (rep.columns - 1) * n:
        assert rep.columns_needed == rep.columns
    assert measure(ctx, "power", d, n, True)[0].actual == [d * (n - 1)]


# ---------------------------------------------------------------- 2. a periodic multiplier
@pytest.mark.parametrize("c", [2, 16])
def test_periodic_multiplier(ctx, c):
    """P_c cur^2 - next at n = 16: degree 2 (n - 1) + n - n / c whatever is declared. Declared 2 the
    proof has one column and the quotient needs two; declared 3 it fits."""
    n = 16
    rep2, _, _ = measure(ctx, "periodic", c, n, 2)
    rep3, _, _ = measure(ctx, "periodic", c, n, 3)
    assert rep2.actual == rep3.actual == [2 * (n - 1) + n - n // c]
    assert (rep2.first_under, rep2.proof_fits, rep2.columns, rep2.columns_needed) == (0, False, 1, 2)
    assert rep2.under == [0] and rep2.minimal == [3]
    assert (rep3.first_under, rep3.proof_fits, rep3.columns_needed) == (None, True, 2)
    assert rep3.under == rep3.over == []


def test_periodic_multiplier_proofs(ctx):
    """The pair with c = 2 through Context.prove and verify. Declared 3: the proof verifies, and
    check_degrees=True proves the same bytes. Declared 2, as observed on an MI355X: zkp_prove
    returns ZKP_OK and a proof that the verifier rejects with status 36
    (InconsistentOodConstraintEvaluations): the quotient's second segment of n coefficients is
    dropped, so the composition columns' value at z is not the constraints'. check_degrees=True
    raises DegreeMismatch instead, before any proving work."""
    n = 16
    p3, cols = C.periodic_case(2, n, 3)
    pub = [cols[0][0], cols[0][n - 1]]
    data = trace_array(cols)
    with p3.register() as air:
        proof, _ = ctx.prove(air, data, pub, OPTS)
        assert verify_status(air, proof, pub, OPTS) == 0
        assert ctx.prove(air, data, pub, OPTS, check_degrees=True)[0] == proof
        d = ctx.alloc(data.nbytes)
        try:
            ctx.to_device(d, data)
            assert ctx.prove_device(air, d, 1, n, pub, OPTS, check_degrees=True)[0] == proof
        finally:
            ctx.free(d)
    p2, _ = C.periodic_case(2, n, 2)
    with p2.register() as air:
        try:
            bad, _ = ctx.prove(air, data, pub, OPTS)
            outcome = ("proof", verify_status(air, bad, pub, OPTS))
        except ZkpError as e:
            outcome = ("error", e.code)
        print("declared 2:", outcome)
        assert outcome == ("proof", 36)
        with pytest.raises(DegreeMismatch) as e:
            ctx.prove(air, data, pub, OPTS, check_degrees=True)
        rep = e.value.report
        assert (rep.actual, rep.under, rep.minimal, rep.proof_fits) == ([2 * (n - 1) + n - n // 2], [0], [3], False)
        assert ctx.constraint_degrees(air, data).proof_fits is False  # the context is as usable as before


# ---------------------------------------------------------------- 3. cancellation, public inputs, zero
def test_cancellation_and_zero(ctx):
    n = 16
    rep, _, _ = measure(ctx, "cancel", n)
    assert rep.actual == [n - 1] and rep.over == [0] and rep.minimal == [1] and rep.under == []
    rep, _, _ = measure(ctx, "zero", n, False)
    assert rep.actual == [None, 2 * (n - 1)] and rep.max_degree == 2 * (n - 1)
    rep, _, _ = measure(ctx, "zero", n, True)
    assert rep.actual == [None, None]
    assert (rep.max_degree, rep.columns_needed, rep.proof_fits, rep.first_under) == (None, 1, True, None)


def test_public_inputs_one_id_two_instances(ctx):
    n = 16
    program, cols = C.pub_case(n)
    want0, want1 = C.reference("pub", n, (0,))[2], C.reference("pub", n, (1,))[2]
    assert (want0, want1) == ([n - 1], [3 * (n - 1)])
    data = trace_array(cols)
    d = ctx.alloc(data.nbytes)
    try:
        ctx.to_device(d, data)
        with program.register() as air:
            for _ in range(2):
                r0 = air.constraint_degrees_device(ctx, d, n, [0])
                r1 = air.constraint_degrees_device(ctx, d, n, [1])
                assert (r0.actual, r0.over, r0.minimal) == (want0, [0], [1])
                assert (r1.actual, r1.over, r1.proof_fits) == (want1, [], True)
            # the C entry's sentinels, as the header states them
            deg = (_native.ctypes.c_uint64 * 1)()
            rep = _native.AirDegreeReportC()
            rc = ctx.lib.zkp_air_constraint_degrees_device(ctx.ptr, air.AIR_ID, (0).to_bytes(16, "little"), 1, d, 1,
                                                           n, deg, 1, _native.ctypes.byref(rep))
            assert (rc, deg[0], rep.first_under, rep.num_constraints) == (0, n - 1, C.NONE32, 1)
    finally:
        ctx.free(d)
    with C.zero_case(n, True)[0].register() as air:
        deg = (_native.ctypes.c_uint64 * 2)()
        rep = _native.AirDegreeReportC()
        data = trace_array(C.zero_case(n, True)[1])
        d = ctx.alloc(data.nbytes)
        try:
            ctx.to_device(d, data)
            rc = ctx.lib.zkp_air_constraint_degrees_device(ctx.ptr, air.AIR_ID, None, 0, d, 2, n, deg, 2,
                                                           _native.ctypes.byref(rep))
        finally:
            ctx.free(d)
        assert (rc, list(deg), rep.max_degree) == (0, [C.DEGREE_ZERO] * 2, C.DEGREE_ZERO)
        assert (rep.columns_needed, rep.proof_fits, rep.first_under) == (1, 1, C.NONE32)


# ---------------------------------------------------------------- 4. an invalid trace
def test_invalid_trace(ctx):
    n = 32
    rep, program, cols = measure(ctx, "invalid", n)
    assert rep.actual == [3 * (n - 1)] * 2
    bad = program.check_trace_device(ctx, trace_array(cols))
    assert bad == program.check_trace(trace_array(cols)) and bad is not None and bad[0] == 0


# ---------------------------------------------------------------- 5. chunks
@pytest.mark.parametrize("count", [300, 1024])
def test_chunks(ctx, count):
    """More constraints than one chunk holds (K = 128 at E n = 64), 300 no multiple of it, zero
    constraints on both sides of every chunk edge and at the very end."""
    program, cols = C.chunk_case(count, C.chunk_zeros(count, 128))
    with program.register() as air:
        E, K = _native.air_constraint_degrees_shape(air, 4, 8)
    assert (E, K) == (8, 128) and count > K
    zeros = C.chunk_zeros(count, K)
    rep, _, _ = measure(ctx, "chunk", count, zeros)
    assert rep.actual == [None if i in zeros else (1 + i % 5) * 7 for i in range(count)]


# ---------------------------------------------------------------- 6. width and length
def test_width_255(ctx):
    rep, _, _ = measure(ctx, "wide")
    assert rep.actual == [14] * 128 and rep.eval_blowup == 2


@pytest.mark.parametrize("logn", [11, 12])
def test_both_sides_of_the_single_pass_ntt(ctx, logn):
    n = 1 << logn
    rep, _, _ = measure(ctx, "invalid", n)
    assert rep.actual == [3 * (n - 1)] * 2 and rep.eval_blowup == 4


# ---------------------------------------------------------------- 7. k_column_degrees alone
def test_column_degrees_kernel():
    path = os.path.join(NATIVE, "column_degrees_check")
    assert os.path.exists(path), f"{path} not built (run __graft_entry__.build())"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "20 cases, 0 mismatches" in r.stdout, r.stdout


# ---------------------------------------------------------------- 8. nothing else moves
def test_interleaved_with_proofs_checks_and_sessions(ctx):
    """One context: a proof, a trace check and a stage session give the same results before and
    after degrees calls of their own program and of one with another width and E."""
    c = CASES[2]
    program, cols, pub = case_inputs(c)
    opts, data = case_options(c), trace_array(cols)
    want = C.reference_degrees(program, cols, c.n)
    other, ocols, owant = C.reference("power", 5, 8)
    with program.register() as prog, other.register() as oprog:
        proof, _ = ctx.prove(prog, data, list(pub), opts)
        assert verify_status(prog, proof, list(pub), opts) == 0
        assert ctx.constraint_degrees(prog, data).actual == want
        assert ctx.prove(prog, data, list(pub), opts)[0] == proof
        broken = [list(col) for col in cols]
        broken[3][5] ^= 1
        bad = ctx.check_trace(prog, trace_array(broken))
        assert bad is not None and ctx.check_trace(prog, data) is None
        assert ctx.constraint_degrees(prog, data).actual == want
        assert ctx.check_trace(prog, trace_array(broken)) == bad and ctx.check_trace(prog, data) is None
        orep = ctx.constraint_degrees(oprog, trace_array(ocols))
        assert orep.actual == owant and orep.eval_blowup == 8
        assert ctx.prove(prog, data, list(pub), opts)[0] == proof
        gamma = deep_cases(c)["small"]
        run_session(ctx, prog, c, gamma)
        assert ctx.constraint_degrees(prog, data).actual == want
        assert ctx.constraint_degrees(oprog, trace_array(ocols)).actual == owant
        run_session(ctx, prog, c, gamma)
        assert ctx.prove(prog, data, list(pub), opts)[0] == proof


# ---------------------------------------------------------------- 9. threads
def test_four_contexts_on_four_threads(ctx):
    n = 16
    p3, cols = C.periodic_case(2, n, 3)
    pub, data = [cols[0][0], cols[0][n - 1]], trace_array(cols)
    inv_prog, inv_cols, inv_want = C.reference("invalid", 32)
    inv_data = trace_array(inv_cols)
    with p3.register() as air, inv_prog.register() as inv_air:
        proof = ctx.prove(air, data, pub, OPTS)[0]
        single = ctx.constraint_degrees(inv_air, inv_data)
        assert single.actual == inv_want
        ctxs = [_native.Context(0) for _ in range(4)]
        results, errors = [None] * 4, []

        def degrees(k):
            results[k] = [fields(r) | {"actual": r.actual}
                          for r in (ctxs[k].constraint_degrees(inv_air, inv_data) for _ in range(8))]

        def proofs(k):
            results[k] = [ctxs[k].prove(air, data, pub, OPTS)[0] for _ in range(8)]

        def guard(f, k):
            try:
                f(k)
            except Exception as e:  # noqa: BLE001 (reported below, from the main thread)
                errors.append((k, repr(e)))
        try:
            threads = [threading.Thread(target=guard, args=(degrees if k < 2 else proofs, k)) for k in range(4)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            for c in ctxs:
                c.close()
        assert not errors, errors
        for k in (0, 1):
            assert results[k] == [fields(single) | {"actual": single.actual}] * 8
        for k in (2, 3):
            assert results[k] == [proof] * 8


# ---------------------------------------------------------------- 10. refusals on a live context
def test_refusals_leave_the_context_usable(ctx):
    n = 16
    p3, cols = C.periodic_case(2, n, 3)
    pub, data = [cols[0][0], cols[0][n - 1]], trace_array(cols)
    want = C.reference("periodic", 2, n, 3)[2]
    L = ctx.lib
    d = ctx.alloc(data.nbytes)
    ctx.to_device(d, data)
    deg = (_native.ctypes.c_uint64 * 4)()
    rep = _native.AirDegreeReportC()
    rp = _native.ctypes.byref(rep)
    zero_pub = (0).to_bytes(16, "little")
    with p3.register() as air, C.pub_case(n)[0].register() as pair, \
            C.power_case(9, 8)[0].register() as nine, C.bound_33_program().register() as b33:
        proof = ctx.prove(air, data, pub, OPTS)[0]
        a = air.AIR_ID

        def call(ctx_ptr=ctx.ptr, air_id=a, pub_elems=None, n_pub=0, trace=d, width=1, rows=n, degrees=deg,
                 capacity=4, report=rp):
            return L.zkp_air_constraint_degrees_device(ctx_ptr, air_id, pub_elems, n_pub, trace, width, rows,
                                                       degrees, capacity, report)
        table = [
            (dict(trace=None), ZKP_ERR_ARGUMENT), (dict(degrees=None), ZKP_ERR_ARGUMENT),
            (dict(report=None), ZKP_ERR_ARGUMENT), (dict(n_pub=1), ZKP_ERR_ARGUMENT),
            (dict(ctx_ptr=None), ZKP_ERR_ARGUMENT), (dict(capacity=0), ZKP_ERR_ARGUMENT),
            (dict(air_id=AIR_MIMC), ZKP_ERR_UNSUPPORTED_AIR), (dict(air_id=AIR_GLOBAL_UPDATE), ZKP_ERR_UNSUPPORTED_AIR),
            (dict(air_id=AIR_TRAINING_UPDATE), ZKP_ERR_UNSUPPORTED_AIR), (dict(air_id=1 << 20), ZKP_ERR_UNSUPPORTED_AIR),
            (dict(rows=12), ZKP_ERR_TRACE_SHAPE), (dict(rows=4), ZKP_ERR_TRACE_SHAPE),
            (dict(width=0), ZKP_ERR_TRACE_SHAPE), (dict(width=256), ZKP_ERR_TRACE_SHAPE),
            (dict(rows=1 << 24), ZKP_ERR_TRACE_SHAPE),               # also every n with n E > 2^28
            (dict(width=2), ZKP_ERR_PUB_INPUTS),                     # not the program's width
            (dict(pub_elems=zero_pub, n_pub=1), ZKP_ERR_PUB_INPUTS),  # the id takes no public inputs
            (dict(air_id=pair.AIR_ID), ZKP_ERR_PUB_INPUTS),          # the id takes one
            (dict(air_id=nine.AIR_ID, rows=8), ZKP_ERR_PUB_INPUTS),  # n divides d - 1
            (dict(air_id=b33.AIR_ID, rows=64), ZKP_ERR_UNSUPPORTED_AIR),  # E > 32
        ]
        for kwargs, status in table:
            assert call(**kwargs) == status, kwargs
            if "ctx_ptr" not in kwargs:  # the successful call below clears it, so this is the refusal's own
                assert L.zkp_last_error(ctx.ptr), kwargs
            assert call() == 0 and [deg[0]] == want and rep.proof_fits == 1, kwargs
            assert ctx.prove(air, data, pub, OPTS)[0] == proof, kwargs
    ctx.free(d)
