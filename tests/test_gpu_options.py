"""The accepted proof-option space on the GPU, against the CPU oracle.

check_options (csrc/host_stark.hpp) accepts 1..255 queries, blowup 2..128, grinding
0..32, remainder degrees 0..255 and three batching methods for each coefficient
draw; several device paths are selected by those options alone:

- dcoin_draw_coeffs_block (csrc/merkle.hip): a LINEAR branch (parallel candidates)
  and a HORNER branch (out[ncoef - 1 - i] across blockDim strides), called with 3,
  180 and 480 constraint coefficients and 7, 121 and 241 DEEP coefficients;
- the FRI tail of ProofRun::fri_layers (csrc/prover.cpp): the fused device tail
  (k_fri_tail), the device remainder, grinding and query gather for a last layer of
  at most 256 values with grinding, and the host remainder / grinding / openings
  otherwise; remainders of 1 to 256 coefficients; proofs without a FRI layer;
- the blowup edges 2, 4, 64, 128 and query counts 1, 2 and 255 (on a 512-point
  domain most of 255 draws repeat: the dedupe and the batch openings do real work).

Every proving case asserts what test_gpu_parity.py asserts: GPU bytes == oracle
bytes, equal trace root, constraint root and nonce, and both verifiers accept.
The arithmetic is integer: no tolerance. Shapes are the smallest that still reach
the branch (option_cases.py).

Not covered: the rejection redo of the LINEAR draw needs a coin candidate >= p,
about 2^-88 per draw, which no real seed reaches.

The last test is the host-side refusal of FRI shapes whose layers do not fit the
trace (check_fri_shape): it only ever shows that nothing was launched."""
import functools

import numpy as np
import pytest

import oracle_ref as O
from proof_format import sections
from option_cases import HORNER, LINEAR, METHOD_PAIRS, MIMC_REMAINDER_SHAPES, REFUSED_SHAPES, fri_layers, options
from test_gpu_parity import felts_of, gu_prover, mimc_case
from test_gpu_stages import check_by_stages, run_stages
from test_training import tu_prover
from zk_stark_project_amd import AIR_GLOBAL_UPDATE, AIR_MIMC, AIR_TRAINING_UPDATE, _native
from zk_stark_project_amd._native import ZkpError, verify_status
from zk_stark_project_amd.field import to_bytes

pytestmark = pytest.mark.gpu

ZKP_ERR_INVALID_OPTIONS = 1


# ---------------------------------------------------------------- inputs (built once per shape)
# the trace and public inputs do not depend on the proof options
@functools.lru_cache(maxsize=None)
def mimc_inputs(n):
    p, trace = mimc_case(n, options(20, 8, 4))
    return AIR_MIMC, trace, tuple(p.get_pub_inputs(trace).to_elements())


@functools.lru_cache(maxsize=None)
def gu_inputs(ndev, n):
    p = gu_prover(ndev, n, options(20, 16, 4), seed=ndev)
    trace = p.build_trace()
    return AIR_GLOBAL_UPDATE, trace, tuple(p.get_pub_inputs(trace).to_elements())


@functools.lru_cache(maxsize=None)
def tu_inputs(bs):
    p = tu_prover(bs, seed=100 + bs, options=options(20, 16, 4))
    trace = p.build_trace()
    return AIR_TRAINING_UPDATE, trace, tuple(p.get_pub_inputs(trace).to_elements())


def check_proof(ctx, inputs, opts, layers=None):
    """One proof on the GPU and on the oracle: the assertions of test_gpu_parity.py."""
    air, trace, pub_el = inputs
    pub = to_bytes(pub_el)
    w, n = trace.data.shape[0], trace.data.shape[1]
    gpu, gtr = ctx.prove(air, trace.data, pub_el, opts)
    ref, otr = O.prove(air, trace.to_bytes(), w, n, pub, opts)
    if layers is not None:  # the case reaches the FRI depth it is listed for
        assert otr.num_fri_layers == layers == gtr.num_fri_layers
    assert bytes(gtr.trace_root) == bytes(otr.trace_root)
    assert bytes(gtr.constraint_root) == bytes(otr.constraint_root)
    assert gtr.pow_nonce == otr.pow_nonce
    assert gpu == ref
    assert O.verify(air, gpu, pub, opts) == 0
    assert verify_status(air, gpu, felts_of(pub), opts) == 0  # product verifier
    return gpu, gtr


# ---------------------------------------------------------------- a. batching methods
@pytest.mark.parametrize("constraints,deep", METHOD_PAIRS)
def test_batching_methods_mimc(ctx, constraints, deep):
    """3 constraint and 7 DEEP coefficients."""
    check_proof(ctx, mimc_inputs(256), options(20, 8, 4, 7, constraints, deep))


@pytest.mark.parametrize("constraints,deep", METHOD_PAIRS)
def test_batching_methods_global_update(ctx, constraints, deep):
    """180 constraint coefficients (one 256-thread stride) and 121 DEEP coefficients
    (two strides of the 64-thread DEEP block)."""
    check_proof(ctx, gu_inputs(6, 64), options(20, 16, 4, 7, constraints, deep))


@pytest.mark.parametrize("constraints,deep", METHOD_PAIRS)
def test_batching_methods_training_update(ctx, constraints, deep):
    """480 constraint and 241 DEEP coefficients: the HORNER reversal spans several
    blockDim strides in both draws."""
    inputs = tu_inputs(2)
    assert inputs[1].data.shape[1] == 256
    check_proof(ctx, inputs, options(20, 16, 4, 7, constraints, deep))


# ---------------------------------------------------------------- b. remainder degree, tail selection
@pytest.mark.parametrize("grind", [4, 0])
@pytest.mark.parametrize("n,blowup,r", MIMC_REMAINDER_SHAPES)
def test_remainder_degree_and_tail(ctx, n, blowup, r, grind):
    """Each (n, B, r) with grinding (device tail where the last layer has <= 256
    values, host tail above) and without (host remainder throughout)."""
    layers = fri_layers(n, blowup, r)
    gpu, _ = check_proof(ctx, mimc_inputs(n), options(20, blowup, grind, r), layers=layers)
    assert len(sections(gpu)["remainder"]) == 16 * (n // 16 ** layers)  # coefficients: remainder domain / B


@pytest.mark.parametrize("grind", [4, 0])
@pytest.mark.parametrize("blowup", [2, 16])
def test_no_fri_layer_global_update(ctx, blowup, grind):
    """GlobalUpdate n = 8: L = 0, a device tail without layers (16- and 128-point remainder domain)."""
    check_proof(ctx, gu_inputs(2, 8), options(20, blowup, grind), layers=0)


# ---------------------------------------------------------------- c. blowup edges
@pytest.mark.parametrize("blowup", [2, 4, 128])
def test_blowup_edges_global_update(ctx, blowup):
    check_proof(ctx, gu_inputs(6, 64), options(20, blowup, 4))


@pytest.mark.parametrize("blowup", [2, 4, 128])
def test_blowup_edges_training_update(ctx, blowup):
    check_proof(ctx, tu_inputs(2), options(20, blowup, 4))


def test_blowup_64_global_update(ctx):
    check_proof(ctx, gu_inputs(6, 1024), options(20, 64, 4))


@pytest.mark.parametrize("blowup", [2, 4])
def test_blowup_below_constraint_degree_is_refused(ctx, blowup):
    """MiMC's constraint evaluation domain needs blowup 8."""
    air, trace, pub_el = mimc_inputs(256)
    with pytest.raises(ZkpError) as e:
        ctx.prove(air, trace.data, pub_el, options(20, blowup, 4))
    assert e.value.code == ZKP_ERR_INVALID_OPTIONS


# ---------------------------------------------------------------- d. query count
@pytest.mark.parametrize("grind", [0, 3])
@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("q", [1, 2, 255])
def test_query_count_mimc(ctx, q, n, grind):
    _, tr = check_proof(ctx, mimc_inputs(n), options(q, 8, grind))
    assert 1 <= tr.num_unique_queries <= min(q, 8 * n)
    if q == 255 and n == 64:  # 255 draws over 512 positions: a run without repeats has probability ~2e-34
        assert tr.num_unique_queries < 255


def test_query_count_255_global_update(ctx):
    check_proof(ctx, gu_inputs(6, 256), options(255, 16, 4))


def test_query_count_255_training_update(ctx):
    inputs = tu_inputs(1)
    assert inputs[1].data.shape[1] == 128
    check_proof(ctx, inputs, options(255, 8, 4, 15), layers=1)


# ---------------------------------------------------------------- e. stage API, non-default options
STAGE_CASES = {
    "mimc": (lambda: mimc_inputs(4096), 8, 3, 8, 6),
    "global_update": (lambda: gu_inputs(6, 64), 16, 15, 2, 1),
    "training_update": (lambda: tu_inputs(2), 16, 15, 2, 1),
}


@pytest.mark.parametrize("name", list(STAGE_CASES))
def test_stages_linear_horner(ctx, name):
    """The session stages driven by the oracle's LINEAR constraint and HORNER DEEP
    coefficients, with a short remainder (MiMC: r = 3, three FRI layers)."""
    get, blowup, r, ce, C = STAGE_CASES[name]
    air, trace, pub_el = get()
    run_stages(ctx, air, trace, list(pub_el), options(20, blowup, 4, r, LINEAR, HORNER), ce, C)


CHANNEL_CASES = {
    "mimc": (lambda: mimc_inputs(256), 8),
    "global_update": (lambda: gu_inputs(6, 64), 16),
    "training_update": (lambda: tu_inputs(2), 16),
}


@pytest.mark.parametrize("name", list(CHANNEL_CASES))
def test_channel_stages_horner_linear(ctx, name):
    """The host channel (zkp_channel_draw) draws HORNER constraint and LINEAR DEEP
    coefficients: commitments, z, nonce, positions and openings equal zkp_prove's,
    whose bytes equal the oracle's."""
    get, blowup = CHANNEL_CASES[name]
    air, trace, pub_el = get()
    opts = options(20, blowup, 4, 7, HORNER, LINEAR)
    gpu = check_by_stages(ctx, air, trace.data, list(pub_el), opts)
    ref, _ = O.prove(air, trace.to_bytes(), trace.data.shape[0], trace.data.shape[1], to_bytes(pub_el), opts)
    assert gpu == ref


# ---------------------------------------------------------------- f. refusals
def test_fri_layers_past_the_trace_are_refused(ctx):
    """16^L > n (the last FRI layer would have no rows): zkp_prove, zkp_prove_device and
    zkp_session_create return ZKP_ERR_INVALID_OPTIONS from the host-side shape check. With
    profiling on, every launch and every finished host stage adds a row to the
    statistics table: it stays empty. The context then proves a normal case."""
    ctx.set_profiling(True)
    try:
        for air, n, blowup, r in REFUSED_SHAPES:
            assert 16 ** fri_layers(n, blowup, r) > n
            opts = options(20, blowup, 4, r)
            _, trace, pub_el = mimc_inputs(n) if air == AIR_MIMC else gu_inputs(2, n)
            w = trace.data.shape[0]
            d = ctx.alloc(trace.data.nbytes)
            try:
                ctx.to_device(d, np.ascontiguousarray(trace.data))
                calls = {"zkp_prove": lambda: ctx.prove(air, trace.data, pub_el, opts),
                         "zkp_prove_device": lambda: ctx.prove_device(air, d, w, n, pub_el, opts),
                         "zkp_session_create": lambda: _native.Session(ctx, air, w, n, list(pub_el), opts)}
                for name, call in calls.items():
                    ctx.reset_stats()
                    with pytest.raises(ZkpError) as e:
                        call()
                    assert e.value.code == ZKP_ERR_INVALID_OPTIONS, name
                    assert ctx.stats_table() == {}, name
            finally:
                ctx.free(d)
        # still usable, and the table does fill when a proof runs
        ctx.reset_stats()
        check_proof(ctx, mimc_inputs(256), options(20, 8, 4))
        assert ctx.stats_table()["host_0_setup"]["launches"] == 1
    finally:
        ctx.set_profiling(False)
        ctx.reset_stats()
