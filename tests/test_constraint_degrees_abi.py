"""zkp_air_degree_bounds and the host-decided refusals of zkp_air_constraint_degrees_device,
without a GPU; and the closed-form degrees of every case of test_gpu_constraint_degrees.py,
asserted on the big-int reference (constraint_degree_cases.py), which shows the cases' traces
are generic.

The device entry's null-pointer refusals come before the context is touched and are called
directly. Its other host-decided statuses come from one host function (degrees_plan), which the
host-only zkp_air_constraint_degrees_shape exposes with the same arguments: that is what runs
here. test_gpu_constraint_degrees.py runs the same table through the device entry on a live context."""
import ctypes
import inspect

import pytest

import constraint_degree_cases as C
from zk_stark_project_amd import (AIR_GLOBAL_UPDATE, AIR_MIMC, AIR_TRAINING_UPDATE, AirProgram, DegreeMismatch,
                                  DegreeReport, RegisteredAir, _native)
from zk_stark_project_amd._native import ZkpError

ZKP_ERR_TRACE_SHAPE, ZKP_ERR_PUB_INPUTS, ZKP_ERR_UNSUPPORTED_AIR, ZKP_ERR_ARGUMENT = 3, 4, 8, 9


def one_constraint(width, build, degree, periodic=()):
    p = AirProgram(width)
    cols = [p.periodic(list(v)) for v in periodic]
    p.constraint(build(p, cols), degree=degree)
    p.assertion(0, 0, 0)
    return p


# ---------------------------------------------------------------- zkp_air_degree_bounds
@pytest.mark.parametrize("d", [1, 2, 9, 17])
def test_bounds_of_powers(d):
    assert C.power_case(d, 64)[0].degree_bounds() == [d]


def test_bounds_count_periodic_operands_and_nothing_else():
    per = [[3, 5], [1, 2, 3, 4]]
    assert one_constraint(1, lambda p, k: k[0] * p.cur[0] * p.cur[0] - p.next[0], 2, per[:1]).degree_bounds() == [3]
    assert one_constraint(1, lambda p, k: k[0] * k[1] * p.cur[0] - p.next[0], 1, per).degree_bounds() == [3]
    # a constant factor adds 0, and so does a pub one
    assert one_constraint(1, lambda p, k: p.const(7) * p.cur[0] * p.cur[0] - p.next[0], 2).degree_bounds() == [2]
    assert one_constraint(1, lambda p, k: p.pub(0) * p.cur[0] * p.cur[0] - p.next[0], 2).degree_bounds() == [2]
    # a sum takes the larger side
    assert one_constraint(2, lambda p, k: p.cur[0] ** 3 + p.cur[1] * k[0], 3, per[:1]).degree_bounds() == [3]


def test_bounds_per_constraint_and_against_the_graph():
    p, _ = C.invalid_case(8)
    assert p.degree_bounds() == [3, 3] == C.product_bounds(p)
    p = AirProgram(2)
    k = p.periodic([3, 5])
    p.constraint(p.cur[0] ** 5 - p.next[0], degree=5)
    p.constraint(p.next[1] - p.cur[1] * k, degree=1)
    p.assertion(0, 0, 0)
    assert p.degree_bounds() == [5, 2] == C.product_bounds(p)
    with p.register() as air:
        assert air.degree_bounds() == [5, 2] == _native.air_degree_bounds(air.AIR_ID)
    p, _ = C.chunk_case(300, C.chunk_zeros(300, 128))
    assert p.degree_bounds() == C.product_bounds(p)


def test_bounds_refusals():
    L = _native.load()
    cnt = ctypes.c_uint32(77)
    buf = (ctypes.c_uint8 * 4)()
    for builtin in (AIR_MIMC, AIR_GLOBAL_UPDATE, AIR_TRAINING_UPDATE, 15, 1 << 20):
        assert L.zkp_air_degree_bounds(builtin, buf, 4, ctypes.byref(cnt)) == ZKP_ERR_UNSUPPORTED_AIR
    with C.invalid_case(8)[0].register() as air:
        assert L.zkp_air_degree_bounds(air.AIR_ID, None, 4, ctypes.byref(cnt)) == ZKP_ERR_ARGUMENT
        assert L.zkp_air_degree_bounds(air.AIR_ID, buf, 4, None) == ZKP_ERR_ARGUMENT
        assert L.zkp_air_degree_bounds(air.AIR_ID, buf, 1, ctypes.byref(cnt)) == ZKP_ERR_ARGUMENT
        assert cnt.value == 2 and b"capacity" in L.zkp_air_last_error()
        assert L.zkp_air_degree_bounds(air.AIR_ID, buf, 2, ctypes.byref(cnt)) == 0 and list(buf[:2]) == [3, 3]
        freed = air.AIR_ID
    assert L.zkp_air_degree_bounds(freed, buf, 4, ctypes.byref(cnt)) == ZKP_ERR_UNSUPPORTED_AIR


# ---------------------------------------------------------------- the device entry's host-decided refusals
def test_device_entry_null_arguments():
    """Without a context only the null ctx can be shown: the other null pointers leave their
    message in the context (test_gpu_constraint_degrees.py runs them on a live one)."""
    L = _native.load()
    some = ctypes.create_string_buffer(64)  # stands for a non-null device pointer: the null ctx returns first
    ptr = ctypes.addressof(some)
    deg = (ctypes.c_uint64 * 4)()
    rep = _native.AirDegreeReportC()
    call = L.zkp_air_constraint_degrees_device
    assert call(None, 4096, None, 0, ptr, 1, 8, deg, 4, ctypes.byref(rep)) == ZKP_ERR_ARGUMENT
    assert call(None, 4096, None, 1, None, 1, 8, None, 4, None) == ZKP_ERR_ARGUMENT
    assert L.zkp_air_constraint_degrees_shape(4096, None, 1, 1, 8, None, None) == ZKP_ERR_ARGUMENT  # n_pub, no pub_elems


def shape_status(air, width, n, pub=None):
    try:
        return _native.air_constraint_degrees_shape(air, width, n, pub)
    except ZkpError as e:
        return e.code


def test_device_entry_host_refusals():
    for builtin in (AIR_MIMC, AIR_GLOBAL_UPDATE, AIR_TRAINING_UPDATE):
        assert shape_status(builtin, 1, 64) == ZKP_ERR_UNSUPPORTED_AIR
    assert shape_status(1 << 20, 1, 64) == ZKP_ERR_UNSUPPORTED_AIR  # not registered
    with C.invalid_case(8)[0].register() as air:
        assert shape_status(air, 2, 8) == (4, 128)
        for n in (0, 4, 12, 1 << 24):
            assert shape_status(air, 2, n) == ZKP_ERR_TRACE_SHAPE
        assert shape_status(air, 0, 8) == shape_status(air, 256, 8) == ZKP_ERR_TRACE_SHAPE
        assert shape_status(air, 3, 8) == ZKP_ERR_PUB_INPUTS   # not the program's width
        assert shape_status(air, 2, 8, [1]) == ZKP_ERR_PUB_INPUTS  # an id without public inputs takes none
        assert b"public inputs" in _native.load().zkp_air_last_error()
        # the chunk: 2^22 felts over E n, at least 1, at most 128
        assert shape_status(air, 2, 1 << 12) == (4, 128)
        assert shape_status(air, 2, 1 << 16) == (4, 16)
        assert shape_status(air, 2, 1 << 23) == (4, 1)
    with C.pub_case(8)[0].register() as air:
        assert shape_status(air, 1, 8, [1]) == (4, 128)
        assert shape_status(air, 1, 8) == shape_status(air, 1, 8, [1, 2]) == ZKP_ERR_PUB_INPUTS
        assert shape_status(air, 1, 8, [C.P]) == ZKP_ERR_PUB_INPUTS  # not canonical
    with C.power_case(9, 8)[0].register() as air:  # n divides d - 1: no proof of this shape exists
        assert shape_status(air, 1, 8) == ZKP_ERR_PUB_INPUTS
        assert shape_status(air, 1, 16) == (16, 128)
    with C.bound_33_program().register() as air:
        assert air.degree_bounds() == [33]
        assert shape_status(air, 1, 64) == ZKP_ERR_UNSUPPORTED_AIR
        assert b"33" in _native.load().zkp_air_last_error()
    # n * E > 2^28: with n <= 2^23 and E <= 32 the product stops at 2^28, so the longer traces that
    # reach it are refused for their length first; the status is the same
    with C.power_case(17, 64)[0].register() as air:
        assert shape_status(air, 1, 1 << 23) == (32, 1)
        assert shape_status(air, 1, 1 << 24) == ZKP_ERR_TRACE_SHAPE


def test_python_surface():
    for name in ("zkp_air_constraint_degrees_device", "zkp_air_degree_bounds", "zkp_air_constraint_degrees_shape"):
        assert name in _native.EXPORTED
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(_native.Context.constraint_degrees_device) == ["self", "air", "d_trace", "width", "n", "pub"]
    assert params(_native.Context.constraint_degrees) == ["self", "air", "trace", "pub"]
    assert params(RegisteredAir.constraint_degrees_device) == ["self", "ctx", "d_trace", "n", "pub"]
    assert params(AirProgram.constraint_degrees) == ["self", "ctx", "trace", "pub"]
    for f in (_native.Context.prove, _native.Context.prove_device):
        assert inspect.signature(f).parameters["check_degrees"].default is False
        assert inspect.signature(f).parameters["validate"].default is False
    r = DegreeReport(16, [38, None, 15], [2, 2, 2], 4, 1, 2, 38, 0, False)
    assert r.minimal == [3, 1, 1] and r.under == [0] and r.over == [1, 2]
    e = DegreeMismatch(r)
    assert e.report is r and isinstance(e, ValueError)


# ---------------------------------------------------------------- the closed forms, on the reference
@pytest.mark.parametrize("n", C.POWER_LENGTHS)
@pytest.mark.parametrize("d", C.POWERS)
def test_reference_powers(d, n):
    program, _, actual = C.reference("power", d, n)
    assert actual == C.power_closed_form(d, n)
    assert C.reference("power", d, n, True)[2] == [d * (n - 1)]  # and on a random column, d = 1 included
    rep = C.expected_report(program, n, actual)
    assert rep["eval_blowup"] == C.domain_factor(d) and rep["first_under"] is None
    if not C.no_proof_shape(d, n):
        assert rep["proof_fits"] and rep["columns_needed"] <= rep["columns"]
        if d * (n - 1) - (n - 1) + 1 > (rep["columns"] - 1) * n:
            assert rep["columns_needed"] == rep["columns"]


@pytest.mark.parametrize("declared", [2, 3])
@pytest.mark.parametrize("c", [2, 16])
def test_reference_periodic_multiplier(c, declared):
    n = 16
    program, _, actual = C.reference("periodic", c, n, declared)
    assert actual == [2 * (n - 1) + n - n // c]
    rep = C.expected_report(program, n, actual)
    assert rep["eval_blowup"] == 4 and rep["columns_needed"] == 2
    assert (rep["columns"], rep["proof_fits"], rep["first_under"]) == ((1, False, 0) if declared == 2 else (2, True, None))


def test_reference_cancellation_pub_and_zero():
    n = 16
    assert C.reference("cancel", n)[2] == [n - 1]
    assert C.reference("pub", n, (0,))[2] == [n - 1]
    assert C.reference("pub", n, (1,))[2] == [3 * (n - 1)]
    assert C.reference("zero", n, False)[2] == [None, 2 * (n - 1)]
    program, _, actual = C.reference("zero", n, True)
    assert actual == [None, None]
    rep = C.expected_report(program, n, actual)
    assert (rep["max_degree"], rep["columns_needed"], rep["proof_fits"]) == (None, 1, True)


def test_reference_invalid_wide_and_long():
    assert C.reference("invalid", 32)[2] == [3 * 31, 3 * 31]
    assert C.reference("wide")[2] == [2 * 7] * 128
    assert C.reference("invalid", 1 << 11)[2] == [3 * ((1 << 11) - 1)] * 2


@pytest.mark.parametrize("count", [300, 1024])
def test_reference_chunks(count):
    zeros = C.chunk_zeros(count, 128)
    assert len(zeros) == 2 * ((count - 1) // 128) + 1
    _, _, actual = C.reference("chunk", count, zeros)
    assert actual == [None if i in zeros else (1 + i % 5) * 7 for i in range(count)]
