"""Constraint programs (zkp_air_register, include/zkp.h) on the host: registration
rules, the verifier under a program id, and zkp_air_check_trace. No GPU.

The verifier cases take proofs made by the CPU oracle under the built-in ids and
verify them under the three built-in AIRs restated as programs (air_program_cases):
the program path of zkp_verify must accept exactly those proofs."""
import functools

import numpy as np
import pytest

import oracle_ref as O
from air_program_cases import (VERIFY_INCONSISTENT_OOD, VERIFY_PUB_INPUTS, ZKP_ERR_ARGUMENT, ZKP_ERR_UNSUPPORTED_AIR,
                               global_update_program, mimc_program, power_program, power_trace, trace_array,
                               training_update_program)
from test_training import tu_prover
from test_verifier import felts, gu
from zk_stark_project_amd import AIR_GLOBAL_UPDATE, AIR_MIMC, AIR_TRAINING_UPDATE, AirProgram, ProofOptions, _native
from zk_stark_project_amd._native import ZkpError, verify_status
from zk_stark_project_amd.air import OP_ADD, OP_EMIT, OP_MUL, OP_SUB, SRC_CONST, SRC_CUR, SRC_PERIODIC, SRC_REG
from zk_stark_project_amd.field import P, to_bytes


def src(kind, index):
    return (kind << 13) | index


def op(code, dst, a, b=0):
    return code | (dst << 8) | (a << 16) | (b << 32)


# a small valid program: r0 = cur0 + const0; emit r0
BASE = dict(width=1, degrees=[1], constants=[1], periodic=[[1, 2]], assertions=[(0, 0, 5)], num_registers=1,
            ops=[op(OP_ADD, 0, src(SRC_CUR, 0), src(SRC_CONST, 0)), op(OP_EMIT, 0, src(SRC_REG, 0))])
ADD0 = BASE["ops"][0]
EMIT0 = BASE["ops"][1]

REFUSED = [
    ("width", dict(width=0)),
    ("width", dict(width=256)),
    ("num_constraints", dict(degrees=[], ops=[ADD0])),
    ("num_constraints", dict(degrees=[1] * 1025, ops=[ADD0] + [EMIT0] * 1025)),
    ("degrees[0]", dict(degrees=[0])),
    ("degrees[0]", dict(degrees=[18])),
    ("degrees[0]", dict(degrees=[33])),
    ("num_constants", dict(constants=[1] * 257)),
    ("constants[0]", dict(constants=[P])),
    ("num_periodic", dict(periodic=[[1, 2]] * 9)),
    ("periodic_cycles[0]", dict(periodic=[[1, 2, 3]])),
    ("periodic_cycles[0]", dict(periodic=[[1]])),
    ("periodic_cycles[1]", dict(periodic=[[1, 2], [1] * 2048])),
    ("periodic_values[1]", dict(periodic=[[1, P]])),
    ("num_assertions", dict(assertions=[(0, s, 1) for s in range(1025)])),
    ("assertions[4]", dict(assertions=[(0, s, 1) for s in (0, 1, 2, 3, 4)])),
    ("assertions[1]", dict(assertions=[(0, 3, 1), (0, 3, 2)])),
    ("assertions[0]", dict(assertions=[(1, 0, 1)])),
    ("assertions[0]", dict(assertions=[(0, 0, P)])),
    ("num_registers", dict(num_registers=0)),
    ("num_registers", dict(num_registers=33)),
    ("num_ops", dict(ops=[])),
    ("num_ops", dict(ops=[ADD0] * 8192 + [EMIT0])),
    ("ops[0]", dict(ops=[op(7, 0, src(SRC_CUR, 0), src(SRC_CONST, 0)), EMIT0])),                  # opcode
    ("ops[0]", dict(ops=[op(OP_ADD, 0, src(5, 0), src(SRC_CONST, 0)), EMIT0])),                   # operand kind
    ("ops[0]", dict(ops=[op(OP_ADD, 1, src(SRC_CUR, 0), src(SRC_CONST, 0)), EMIT0])),             # dst register
    ("ops[0]", dict(ops=[op(OP_ADD, 0, src(SRC_REG, 1), src(SRC_CONST, 0)), EMIT0])),             # register operand
    ("ops[0]", dict(ops=[op(OP_ADD, 0, src(SRC_CUR, 1), src(SRC_CONST, 0)), EMIT0])),             # trace column
    ("ops[0]", dict(ops=[op(OP_ADD, 0, src(SRC_CUR, 0), src(SRC_CONST, 1)), EMIT0])),             # constant
    ("ops[0]", dict(ops=[op(OP_ADD, 0, src(SRC_CUR, 0), src(SRC_PERIODIC, 1)), EMIT0])),          # periodic column
    ("ops[0]", dict(ops=[op(OP_ADD, 0, src(SRC_REG, 0), src(SRC_CONST, 0)), EMIT0])),             # read before write
    ("ops[0]", dict(ops=[ADD0 | (1 << 48), EMIT0])),                                              # reserved bits
    ("ops[2]", dict(ops=[ADD0, EMIT0, EMIT0])),                                                   # too many EMITs
    ("ops", dict(ops=[ADD0])),                                                                    # too few EMITs
    ("degrees[0]", dict(ops=[op(OP_MUL, 0, src(SRC_CUR, 0), src(SRC_CUR, 0)), EMIT0])),           # x^2 declared 1
]


def test_base_program_round_trips():
    """An accepted program registers, unregisters and registers again under a new id
    (ids start at 16 and are never reused); a freed id cannot be freed twice."""
    a = _native.air_register(**BASE)
    assert a >= 16
    _native.air_unregister(a)
    with pytest.raises(ZkpError) as e:
        _native.air_unregister(a)
    assert e.value.code == ZKP_ERR_ARGUMENT
    b = _native.air_register(**BASE)
    assert b > a
    _native.air_unregister(b)
    for builtin in (AIR_MIMC, AIR_GLOBAL_UPDATE, AIR_TRAINING_UPDATE, 0, -1):
        with pytest.raises(ZkpError):
            _native.air_unregister(builtin)


@pytest.mark.parametrize("field,change", REFUSED, ids=[f"{i}-{f}" for i, (f, _) in enumerate(REFUSED)])
def test_registration_refusals(field, change):
    """Every rule of zkp_air_program that does not depend on n: ZKP_ERR_ARGUMENT, and
    zkp_air_last_error names the failing field."""
    with pytest.raises(ZkpError) as e:
        _native.air_unregister(_native.air_register(**{**BASE, **change}))
    assert e.value.code == ZKP_ERR_ARGUMENT
    assert f"zkp_air_register: {field}" in str(e.value), str(e.value)


def test_limits_are_accepted():
    """The largest program of each kind registers: 1024 constraints of degree 17, 256
    constants, 8 periodic columns of cycle 1024, every cell of 4 rows of a 255-column
    trace asserted (1020 assertions over 4 steps), 32 registers, 8192 ops."""
    big = dict(width=255, degrees=[17] * 1024, constants=list(range(256)), periodic=[[1] * 1024] * 8,
               assertions=[(c, s, 1) for s in (0, 1, 2, 10**12) for c in range(255)], num_registers=32,
               ops=[op(OP_ADD, 31, src(SRC_CUR, 254), src(SRC_CONST, 255))] * (8192 - 1024) +
               [op(OP_EMIT, 0, src(SRC_REG, 31))] * 1024)
    assert len(big["ops"]) == 8192
    _native.air_unregister(_native.air_register(**big))


def test_builder_shares_subexpressions_and_reuses_registers():
    p = mimc_program(64, [1, 2])
    cp = p.compile()
    # u = cur + K; u^7 by square and multiply: u2, u4, u3 = u*u2, u7 = u3*u4; next - u7; emit
    assert len(cp.ops) == 7 and cp.num_registers <= 3
    assert [o & 0xff for o in cp.ops] == [OP_ADD, OP_MUL, OP_MUL, OP_MUL, OP_MUL, OP_SUB, OP_EMIT]
    q = AirProgram(2)
    e = q.cur[0] * q.cur[1]
    assert e is q.cur[1] * q.cur[0]  # commutative operands share a node
    with pytest.raises(ValueError):
        q.cur[0] + p.cur[0]  # two programs


# ---------------------------------------------------------------- verifier parity (no GPU)
@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """-> (built-in id, proof, pub, options, n) of an oracle-made proof."""
    if name.startswith("mimc"):
        n = int(name[4:])
        opts = ProofOptions(24, 8, 4)
        vals = felts(O.mimc_trace(42 * 10**6, n))
        pub = (vals[0], vals[-1])
        proof, _ = O.prove(AIR_MIMC, to_bytes(vals), 1, n, to_bytes(pub), opts)
        return AIR_MIMC, proof, pub, opts, n
    if name == "gu16":
        n, opts = 16, ProofOptions(20, 16, 4)
        g = gu(3, n, 2, opts)
        t = g.build_trace()
        pub = tuple(g.get_pub_inputs(t).to_elements())
        proof, _ = O.prove(AIR_GLOBAL_UPDATE, t.to_bytes(), 120, n, to_bytes(pub), opts)
        return AIR_GLOBAL_UPDATE, proof, pub, opts, n
    opts = ProofOptions(20, 8, 4)
    tp = tu_prover(0, seed=5, options=opts)
    t = tp.build_trace()
    assert t.length() == 16
    pub = tuple(tp.get_pub_inputs(t).to_elements())
    proof, _ = O.prove(AIR_TRAINING_UPDATE, t.to_bytes(), 240, 16, to_bytes(pub), opts)
    return AIR_TRAINING_UPDATE, proof, pub, opts, 16


def build_program(air, pub, n):
    if air == AIR_MIMC:
        return mimc_program(n, pub)
    return global_update_program(pub, n) if air == AIR_GLOBAL_UPDATE else training_update_program(pub, n)


def register_with(p, ops=None):
    """register() with the compiled op stream replaced."""
    cp = p.compile()
    return _native.air_register(p.width, [d for _, d in p.constraints], p.constants, p.periodic_columns,
                                p.assertions, cp.num_registers, ops or cp.ops)


CASES = ["mimc64", "mimc256", "gu16", "tu16"]


@pytest.mark.parametrize("name", CASES)
def test_verifier_accepts_oracle_proofs_under_program_ids(name):
    air, proof, pub, opts, n = oracle_case(name)
    assert verify_status(air, proof, pub, opts) == 0
    with build_program(air, pub, n).register() as prog:
        assert verify_status(prog, proof, pub, opts) == 0
        assert verify_status(prog.AIR_ID, proof, pub, opts) == 0
        aid = prog.AIR_ID
    assert verify_status(aid, proof, pub, opts) == VERIFY_PUB_INPUTS  # freed: no such AIR


@pytest.mark.parametrize("name", CASES)
def test_verifier_rejects_a_changed_constant_or_op(name):
    air, proof, pub, opts, n = oracle_case(name)
    # one constant changed
    if air == AIR_MIMC:
        rc = list(range(10**6, 65 * 10**6, 10**6))
        rc[17] += 1
        changed = mimc_program(n, pub, constants=rc)
    elif air == AIR_GLOBAL_UPDATE:
        changed = global_update_program(pub, n, k=(pub[120] + 1) % P)
    else:
        changed = training_update_program(pub, n)
        changed.constants[0] = 1
    with changed.register() as prog:
        assert verify_status(prog, proof, pub, opts) == VERIFY_INCONSISTENT_OOD
    # one op changed
    p = build_program(air, pub, n)
    ops = list(p.compile().ops)
    if air == AIR_MIMC:
        assert ops[0] & 0xff == OP_ADD
        ops[0] = ops[0] & ~0xff | OP_SUB           # (K - cur)^7
    elif air == AIR_GLOBAL_UPDATE:
        assert ops[0] & 0xff == OP_MUL
        ops[0] = ops[0] & ~0xff | OP_ADD           # k + next_0
    else:
        assert ops[5] & 0xff == OP_EMIT
        ops[5] = op(OP_EMIT, 0, src(SRC_CUR, 5))   # constraint 5 = cur_5
    aid = register_with(p, ops)
    try:
        assert verify_status(aid, proof, pub, opts) == VERIFY_INCONSISTENT_OOD
    finally:
        _native.air_unregister(aid)


@pytest.mark.parametrize("name", CASES)
def test_verifier_changed_assertion_matches_changed_public_input(name):
    """One assertion value changed in the program: the status the built-in id gives for
    the same change to its public inputs."""
    air, proof, pub, opts, n = oracle_case(name)
    wrong = list(pub)
    at = {AIR_MIMC: 1, AIR_GLOBAL_UPDATE: 60, AIR_TRAINING_UPDATE: 0}[air]
    wrong[at] = (wrong[at] + 1) % P
    want = verify_status(air, proof, wrong, opts)
    assert want != 0
    with build_program(air, wrong, n).register() as prog:
        assert verify_status(prog, proof, pub, opts) == want


def test_shape_mismatches_are_public_input_errors():
    """A width other than the program's, an assertion step >= n and a cycle > n."""
    air, proof, pub, opts, n = oracle_case("mimc64")
    with mimc_program(128, pub).register() as prog:      # assertion at row 127 of a 64-row trace
        assert verify_status(prog, proof, pub, opts) == VERIFY_PUB_INPUTS
    with global_update_program(oracle_case("gu16")[2], 16).register() as prog:  # width 120
        assert verify_status(prog, proof, pub, opts) == VERIFY_PUB_INPUTS
    p = AirProgram(1)
    p.constraint(p.next[0] - p.cur[0] - p.periodic(list(range(128))), 1)  # cycle 128 > n = 64
    with p.register() as prog:
        assert verify_status(prog, proof, pub, opts) == VERIFY_PUB_INPUTS
        with pytest.raises(ZkpError) as e:
            _native.Channel(prog, 1, 64, pub, opts)
        assert e.value.code == 4  # ZKP_ERR_PUB_INPUTS
        _native.Channel(prog, 1, 128, pub, opts).close()
    # a trace length that divides (degree - 1): the quotient does not fit the composition columns
    with power_program(9, 8).register() as prog:
        for n, want in [(8, 4), (16, 0)]:
            try:
                _native.Channel(prog, 2, n, pub, ProofOptions(20, 8, 4)).close()
                got = 0
            except ZkpError as e:
                got = e.code
            assert got == want, n


# ---------------------------------------------------------------- zkp_air_check_trace
def spec_check(p, cols):
    """AirProgram.evaluate over every frame, then the assertions in (step, column) order."""
    n = len(cols[0])
    for r in range(n - 1):
        vals = p.evaluate([c[r] for c in cols], [c[r + 1] for c in cols], r)
        for i, v in enumerate(vals):
            if v:
                return (r, i, None)
    for k, (c, s, v) in enumerate(p.sorted_assertions()):
        if cols[c][s] != v:
            return (s, None, k)
    return None


def test_check_trace_power_program():
    n = 16
    cols = power_trace(3, n)
    p = power_program(3, n)
    assert spec_check(p, cols) is None
    assert p.check_trace(trace_array(cols)) is None
    with p.register() as prog:
        for c, r in [(0, 5), (1, 9), (0, 0), (1, n - 1), (0, n - 1)]:
            bad = [list(col) for col in cols]
            bad[c][r] = (bad[c][r] + 1) % P
            got = prog.check_trace(trace_array(bad))
            assert got is not None and got == spec_check(p, bad), (c, r)
        # the corrupted cell (0, 5) first breaks the frame of rows 4 and 5, constraint 0
        bad = [list(col) for col in cols]
        bad[0][5] += 1
        assert prog.check_trace(trace_array(bad)) == (4, 0, None)
        bad = [list(col) for col in cols]
        bad[1][9] += 1
        assert prog.check_trace(trace_array(bad)) == (8, 1, None)
    # a broken assertion: every transition holds, assertion 2 = (column 1, row n/2)
    q = power_program(3, n)
    q.assertions[2] = (1, n // 2, (cols[1][n // 2] + 1) % P)
    assert q.check_trace(trace_array(cols)) == (n // 2, None, 2)
    assert spec_check(q, cols) == (n // 2, None, 2)


def test_check_trace_mimc_program():
    n = 128
    t = _native.mimc_trace(42 * 10**6, n)
    cols = [felts(t.tobytes())]
    p = mimc_program(n, [cols[0][0], cols[0][-1]])
    with p.register() as prog:
        assert prog.check_trace(t.reshape(1, n, 2)) is None
        bad = np.array(t.reshape(1, n, 2), copy=True)
        bad[0, 77, 0] ^= np.uint64(1)
        assert prog.check_trace(bad) == (76, 0, None)
        assert spec_check(p, [felts(bad.tobytes())]) == (76, 0, None)
        last = np.array(t.reshape(1, n, 2), copy=True)
        last[0, n - 1, 0] ^= np.uint64(1)  # breaks the last frame first
        assert prog.check_trace(last) == (n - 2, 0, None)
    with mimc_program(n, [cols[0][0], (cols[0][-1] + 1) % P]).register() as prog:
        assert prog.check_trace(t.reshape(1, n, 2)) == (n - 1, None, 1)


def test_check_trace_refuses_builtin_ids_and_bad_shapes():
    t = _native.mimc_trace(1, 64).reshape(1, 64, 2)
    for air in (AIR_MIMC, AIR_GLOBAL_UPDATE, AIR_TRAINING_UPDATE):
        with pytest.raises(ZkpError) as e:
            _native.air_check_trace(air, t)
        assert e.value.code == ZKP_ERR_UNSUPPORTED_AIR
    with pytest.raises(ZkpError) as e:
        _native.air_check_trace(10**6, t)  # not registered
    assert e.value.code == ZKP_ERR_UNSUPPORTED_AIR
    with mimc_program(64, [1, 2]).register() as prog:
        with pytest.raises(ZkpError) as e:
            prog.check_trace(np.zeros((2, 64, 2), dtype=np.uint64))  # width
        assert e.value.code == 4
        with pytest.raises(ZkpError) as e:
            prog.check_trace(np.zeros((1, 48, 2), dtype=np.uint64))  # not a power of two
        assert e.value.code == 3
