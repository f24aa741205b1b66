"""Trace validation on the GPU (k_check_program, zkp_air_check_trace_device).

The yardstick everywhere is the host check (zkp_air_check_trace) on the same array:
exact tuple equality. Shapes are the smallest that reach each path: n = 8 (a wave
with 7 live lanes), 64 (lane 63 idle), 128 (frame 63 reads its next row from the
second wave's range), 4096 (many blocks; width-1 programs only)."""
import functools
import random

import numpy as np
import pytest

from air_program_cases import (global_update_program, mimc_program, power_periodic, power_program, power_trace,
                               trace_array, trace_columns)
from option_cases import ALGEBRAIC
from test_gpu_options import gu_inputs, mimc_inputs
from zk_stark_project_amd import AIR_MIMC, AirProgram, InvalidTrace, ProofOptions, _native
from zk_stark_project_amd._native import ZkpError, verify_status
from zk_stark_project_amd.field import P, inv

pytestmark = pytest.mark.gpu

ERR_TRACE_SHAPE, ERR_PUB_INPUTS, ERR_UNSUPPORTED_AIR = 3, 4, 8
OPTS = ProofOptions(20, 8, 4, 1, 16, 7, ALGEBRAIC, ALGEBRAIC)


def both(ctx, prog, data):
    """The device result on `data` (uploaded by Context.check_trace), equal to the host's."""
    want = prog.check_trace(data)
    got = ctx.check_trace(prog, data)
    assert got == want, (got, want)
    return got


def wrap_fails(p, cols):
    """Frame (n-1 -> 0) breaks a constraint: a check that wrapped would not return None."""
    n = len(cols[0])
    return any(p.evaluate([c[n - 1] for c in cols], [c[0] for c in cols], n - 1))


@functools.lru_cache(maxsize=None)
def mimc_cols(n):
    _, trace, pub = mimc_inputs(n)
    return trace_columns(trace.data), pub


def mimc_like(n, rows):
    """The MiMC program with column 0 asserted at `rows` (values of the valid trace)."""
    cols, _ = mimc_cols(n)
    p = AirProgram(1)
    K = p.periodic([(j + 1) * 10**6 for j in range(64)])
    p.constraint(p.next[0] - (p.cur[0] + K) ** 7, degree=7)
    for r in rows:
        p.assertion(0, r, cols[0][r])
    return p


def power_air(d, n, assertions):
    """power_program's constraints with the given (column, step, value) assertions, in that order."""
    p1, p2 = power_periodic(n)
    p = AirProgram(2)
    P1, P2 = p.periodic(p1), p.periodic(p2)
    p.constraint(p.next[0] - (p.cur[0] ** d + P1), degree=d)
    p.constraint(p.next[1] - (p.cur[1] + p.cur[0] * P2), degree=1)
    for a in assertions:
        p.assertion(*a)
    return p


@functools.lru_cache(maxsize=None)
def power_cols(d, n):
    return power_trace(d, n)


# ---------------------------------------------------------------- valid traces
@pytest.mark.parametrize("n", [64, 256])
def test_valid_mimc(ctx, n):
    """n = 64: the cycle is the trace; n = 256: the periodic column wraps."""
    cols, pub = mimc_cols(n)
    p = mimc_program(n, pub)
    assert wrap_fails(p, cols)
    with p.register() as prog:
        assert both(ctx, prog, trace_array(cols)) is None


@pytest.mark.parametrize("d,n", [(2, 8), (3, 8), (9, 16), (17, 32)])
def test_valid_power(ctx, d, n):
    cols = power_cols(d, n)
    p = power_program(d, n)
    assert wrap_fails(p, cols)
    with p.register() as prog:
        assert both(ctx, prog, trace_array(cols)) is None


def test_valid_global_update(ctx):
    _, trace, pub = gu_inputs(3, 16)
    p = global_update_program(pub, 16)
    assert wrap_fails(p, trace_columns(trace.data))
    with p.register() as prog:
        assert both(ctx, prog, trace.data) is None


# ---------------------------------------------------------------- single-cell corruption
@pytest.mark.parametrize("asserted", [False, True])
@pytest.mark.parametrize("n", [128, 4096])
def test_single_cell(ctx, n, asserted):
    """One cell changed at each of the rows where the lane, wave or block changes, in a cell
    that the program asserts and in one it does not (at most 4 steps may be asserted, so the
    asserted rows come in three sets)."""
    cols, _ = mimc_cols(n)
    sets = [(0, n - 1), (1, 62, 63, 64), (0, n - 2)]
    for row in (0, 1, 62, 63, 64, n - 2, n - 1):
        rows = next(s for s in sets if (row in s) == asserted)
        bad = list(cols[0])
        bad[row] = (bad[row] + 1) % P
        with mimc_like(n, rows).register() as prog:
            got = both(ctx, prog, trace_array([bad]))
        assert got == (max(row - 1, 0), 0, None)


# ---------------------------------------------------------------- ordering
def test_first_row_and_first_constraint(ctx):
    n = 128
    cols, pub = mimc_cols(n)
    bad = list(cols[0])
    bad[100] ^= 1
    bad[71] ^= 1
    with mimc_program(n, pub).register() as prog:
        assert both(ctx, prog, trace_array([bad])) == (70, 0, None)
    pc = power_cols(3, n)
    with power_program(3, n).register() as prog:
        two = [list(c) for c in pc]
        two[0][41] ^= 1
        two[1][41] ^= 1
        assert both(ctx, prog, trace_array(two)) == (40, 0, None)
        one = [list(c) for c in pc]
        one[1][41] ^= 1
        assert both(ctx, prog, trace_array(one)) == (40, 1, None)
        rnd = random.Random(5)
        noise = [[rnd.randrange(P) for _ in range(n)] for _ in range(2)]
        assert both(ctx, prog, trace_array(noise)) == (0, 0, None)


# ---------------------------------------------------------------- assertions
def test_assertions(ctx):
    """Assertions registered out of order over 4 steps; stored order is (step, column)."""
    n = 16
    cols = power_cols(2, n)
    data = trace_array(cols)
    cells = [(1, n - 1), (0, 3), (1, 0), (0, n // 2), (0, 0), (1, 3), (0, n - 1)]   # as registered
    stored = sorted(cells, key=lambda a: (a[1], a[0]))

    def program(wrong):
        return power_air(2, n, [(c, s, cols[c][s] + (1 if (c, s) in wrong else 0)) for c, s in cells])
    with program([]).register() as prog:
        assert both(ctx, prog, data) is None
    with program([(0, n // 2)]).register() as prog:
        assert both(ctx, prog, data) == (n // 2, None, stored.index((0, n // 2)))
    with program([(1, n - 1), (1, 3), (0, n - 1)]).register() as prog:
        assert both(ctx, prog, data) == (3, None, stored.index((1, 3)))
        broken = [list(c) for c in cols]
        broken[1][10] ^= 1  # a transition failure wins over the assertions
        assert both(ctx, prog, trace_array(broken)) == (9, 1, None)


# ---------------------------------------------------------------- limits
def wide_case(wrong_last=False):
    w, n = 255, 8
    p = AirProgram(w)
    for i in range(w):
        p.constraint(p.next[i] - (p.cur[i] + p.cur[(i + 1) % w] * p.const(i + 2)), degree=1)
    rows = [[(1 + 3 * i) % P for i in range(w)]]
    for _ in range(n - 1):
        r = rows[-1]
        rows.append([(r[i] + r[(i + 1) % w] * (i + 2)) % P for i in range(w)])
    cols = [[rows[t][i] for t in range(n)] for i in range(w)]
    for t in (0, 1, 2, 7):
        for i in range(w):
            p.assertion(i, t, cols[i][t] + (1 if wrong_last and (i, t) == (w - 1, 7) else 0))
    return p, cols


def test_width_255_and_1020_assertions(ctx):
    """n = 8: 7 live lanes, the allocation ends at width * n * 16 bytes; a constraint on
    column 254; 1020 assertions with the wrong value at the last stored index."""
    p, cols = wide_case()
    with p.register() as prog:
        assert both(ctx, prog, trace_array(cols)) is None
        bad = [list(c) for c in cols]
        bad[254][7] ^= 1
        assert both(ctx, prog, trace_array(bad)) == (6, 254, None)
    p, cols = wide_case(wrong_last=True)
    assert len(p.assertions) == 1020
    with p.register() as prog:
        assert both(ctx, prog, trace_array(cols)) == (7, None, 1019)


def test_32_registers(ctx):
    """31 products kept live under a multiply-add chain: 32 registers (32 KiB of LDS per block)."""
    n = 128
    p = AirProgram(1)
    v = [p.cur[0] * p.const(1000 + 7 * i) for i in range(31)]
    acc = p.next[0]
    for j in range(62):
        acc = acc * p.const(3 + j % 5) + v[j % 31]
    p.constraint(acc, degree=1)
    assert p.compile().num_registers == 32
    a, b = p.evaluate([0], [1], 0)[0], p.evaluate([1], [0], 0)[0]  # constraint = a * next + b * cur
    col = [12345]
    for _ in range(n - 1):
        col.append(-b * col[-1] % P * inv(a) % P)
    p.assertion(0, 0, col[0])
    p.assertion(0, n - 1, col[n - 1])
    with p.register() as prog:
        assert both(ctx, prog, trace_array([col])) is None
        col[65] ^= 1
        assert both(ctx, prog, trace_array([col])) == (64, 0, None)


def test_eight_periodic_columns(ctx):
    """Cycles 2, 4, ..., 256 = n."""
    n = 256
    vals = [[(11 * j + 5 * k + 1) % P for k in range(2 << j)] for j in range(8)]
    p = AirProgram(1)
    per = [p.periodic(v) for v in vals]
    expr = p.cur[0] * per[0]
    for q in per[1:]:
        expr = expr + q
    p.constraint(p.next[0] - expr, degree=1)
    col = [7]
    for r in range(n - 1):
        col.append((col[r] * vals[0][r % 2] + sum(v[r % len(v)] for v in vals[1:])) % P)
    p.assertion(0, 0, col[0])
    p.assertion(0, n - 1, col[n - 1])
    with p.register() as prog:
        assert both(ctx, prog, trace_array([col])) is None
        col[200] ^= 1
        assert both(ctx, prog, trace_array([col])) == (199, 0, None)


# ---------------------------------------------------------------- seeded sweep
SWEEP_SEED, SWEEP_CASES = 2024, 320


def sweep_cases(seed=SWEEP_SEED, count=SWEEP_CASES):
    """(program, data) pairs: power_program's constraints for d in {2, 3, 5} or MiMC (n >= 64),
    n in {8, 16, 64, 128, 512}, 0-3 corrupted cells, and on half of the cases 1-2 wrong
    asserted values (a trace cell of these programs always sits in a transition, so only a
    wrong asserted value gives an assertion failure)."""
    rnd = random.Random(seed)
    for _ in range(count):
        n = rnd.choice([8, 16, 64, 128, 512])
        kind = rnd.choice(["mimc", 2, 3, 5]) if n >= 64 else rnd.choice([2, 3, 5])
        cols = mimc_cols(n)[0] if kind == "mimc" else power_cols(kind, n)
        w = len(cols)
        steps = rnd.sample(range(n), 4)
        cells = [(rnd.randrange(w), s) for s in steps for _ in range(rnd.randint(1, 2))]
        cells = list(dict.fromkeys(cells))
        rnd.shuffle(cells)
        wrong = set(rnd.sample(cells, min(len(cells), rnd.randint(1, 2)))) if rnd.random() < 0.5 else set()
        asserts = [(c, s, cols[c][s] + (1 if (c, s) in wrong else 0)) for c, s in cells]
        if kind == "mimc":
            p = mimc_like(n, ())
            for a in asserts:
                p.assertion(*a)
        else:
            p = power_air(kind, n, asserts)
        bad = [list(c) for c in cols]
        for _ in range(rnd.randint(0, 3)):
            c, r = rnd.randrange(w), rnd.randrange(n)
            bad[c][r] = (bad[c][r] + 1 + rnd.randrange(P - 1)) % P
        yield p, trace_array(bad)


def test_seeded_sweep(ctx):
    valid = transition = assertion = 0
    for p, data in sweep_cases():
        with p.register() as prog:
            got = both(ctx, prog, data)
        want = p.check_trace(data)  # the counts are the host's judgement
        valid += want is None
        transition += want is not None and want[1] is not None
        assertion += want is not None and want[2] is not None
    assert valid + transition + assertion == SWEEP_CASES >= 200
    assert valid >= 20 and transition >= 50 and assertion >= 20, (valid, transition, assertion)


# ---------------------------------------------------------------- error parity
def test_error_parity(ctx):
    """Both entry points return the same status, decided before any launch; the context
    proves afterwards."""
    n = 64
    cols, pub = mimc_cols(n)
    d = ctx.alloc(255 * 64 * 16)

    def codes(air, width, rows):
        out = []
        for call in (lambda: _native.air_check_trace(air, np.zeros((width, rows, 2), dtype=np.uint64)),
                     lambda: ctx.check_trace_device(air, d, width, rows)):
            with pytest.raises(ZkpError) as e:
                call()
            out.append(e.value.code)
        return out
    try:
        gone = mimc_program(n, pub).register()
        gone_id = gone.AIR_ID
        gone.close()
        with mimc_program(n, pub).register() as prog, power_program(2, 64).register() as pw:
            assert codes(AIR_MIMC, 1, n) == [ERR_UNSUPPORTED_AIR] * 2           # a built-in id
            assert codes(gone_id, 1, n) == [ERR_UNSUPPORTED_AIR] * 2            # an unregistered id
            assert codes(prog, 2, n) == [ERR_PUB_INPUTS] * 2                    # another width
            assert codes(prog, 1, 48) == [ERR_TRACE_SHAPE] * 2                  # n no power of two
            assert codes(pw, 2, 32) == [ERR_PUB_INPUTS] * 2                     # an assertion step >= n
            assert codes(prog, 1, 32) == [ERR_PUB_INPUTS] * 2                   # a cycle > n
            data = trace_array(cols)
            proof, _ = ctx.prove(prog, data, pub, OPTS, validate=True)
            assert verify_status(prog, proof, pub, OPTS) == 0
    finally:
        ctx.free(d)


# ---------------------------------------------------------------- validate=
def test_validate(ctx):
    n = 64
    cols, pub = mimc_cols(n)
    data = trace_array(cols)
    bad = np.array(data, copy=True)
    bad[0, 5, 0] ^= np.uint64(0x5A5A)
    d = ctx.alloc(data.nbytes)
    try:
        with mimc_program(n, pub).register() as prog:
            want = prog.check_trace(bad)
            assert want == (4, 0, None)
            with pytest.raises(InvalidTrace) as e:
                ctx.prove(prog, bad, pub, OPTS, validate=True)
            assert (e.value.row, e.value.constraint, e.value.assertion) == want
            ctx.to_device(d, bad)
            assert ctx.check_trace_device(prog, d, 1, n) == prog.check_trace_device(ctx, d, n) == want
            assert ctx.check_trace(prog, bad) == want
            with pytest.raises(InvalidTrace) as e:
                ctx.prove_device(prog, d, 1, n, pub, OPTS, validate=True)
            assert (e.value.row, e.value.constraint, e.value.assertion) == want
            ctx.to_device(d, data)
            assert prog.check_trace_device(ctx, d, n) is None
            checked, _ = ctx.prove(prog, data, pub, OPTS, validate=True)
            resident, _ = ctx.prove_device(prog, d, 1, n, pub, OPTS, validate=True)
            plain, _ = ctx.prove(prog, data, pub, OPTS)
            builtin, _ = ctx.prove(AIR_MIMC, data, pub, OPTS)
            assert checked == resident == plain == builtin
        for call in (lambda: ctx.prove(AIR_MIMC, data, pub, OPTS, validate=True),
                     lambda: ctx.prove_device(AIR_MIMC, d, 1, n, pub, OPTS, validate=True)):
            with pytest.raises(ZkpError) as e:
                call()
            assert e.value.code == ERR_UNSUPPORTED_AIR
    finally:
        ctx.free(d)
