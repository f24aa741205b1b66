"""FRI folding factors 2, 4 and 8 on the GPU, against the CPU oracle.

The factor selects device code of its own: the fold kernels (k_fri_fold<F>,
csrc/merkle.hip), rows of 2, 4 and 8 values in the layer trees (one or two BLAKE3
blocks; the LDS-fused tree up to 2^16 rows, the lane-subtree pass above), trees of
2 and 4 leaves, up to 16 layers, the fused tail (k_fri_tail<F>) with up to 7 small
layers, and 4 * F words per row in the device query gather. One F = 16 case sits with
them (b.): k_fri_fold<16> above 2^15 rows, which the fast F = 16 tests do not reach.

Every proving case asserts what check_proof of test_gpu_options.py asserts: GPU
bytes == oracle bytes, equal trace root, constraint root and nonce, the listed
layer count, and both verifiers accept. The arithmetic is integer: no tolerance.
Shapes are the smallest that reach each branch (folding_cases.py)."""
import threading

import numpy as np
import pytest

import oracle_ref as O
from folding_cases import (DEPTH_CASES, FACTORS, FOLD16_LANE_CASE, MAX_FRI_LAYERS, PAST_TRACE, TOO_DEEP,
                           WIDE_LAYER_CASES, fri_layers, options)
from proof_format import sections
from test_gpu_options import check_proof, gu_inputs, mimc_inputs, tu_inputs
from test_gpu_stages import check_by_stages
from zk_stark_project_amd import AIR_MIMC, _native
from zk_stark_project_amd._native import ZkpError
from zk_stark_project_amd.field import to_bytes

pytestmark = pytest.mark.gpu

ZKP_ERR_INVALID_OPTIONS = 1


# ---------------------------------------------------------------- a. depth and remainder
@pytest.mark.parametrize("fold,n,blowup,r,layers,grind",
                         [(f, n, b, r, L, g) for f, n, b, r, L, grinds in DEPTH_CASES for g in grinds])
def test_depth_and_remainder(ctx, fold, n, blowup, r, layers, grind):
    """With grinding: the fused device tail (last layer of <= 256 values) or the host
    tail; without: the host remainder, grinding and openings."""
    assert fri_layers(n, blowup, r, fold) == layers <= MAX_FRI_LAYERS
    gpu, _ = check_proof(ctx, mimc_inputs(n), options(20, blowup, grind, r, fold), layers=layers)
    # coefficients = remainder domain / B, the remainder domain being N / F^L
    assert len(sections(gpu)["remainder"]) == 16 * (n * blowup // fold ** layers // blowup)


# ---------------------------------------------------------------- b. layer 0 above 2^16 rows
@pytest.mark.parametrize("fold,n,layers", WIDE_LAYER_CASES)
def test_first_layer_above_65536_rows(ctx, fold, n, layers):
    """The smallest n whose first layer has more than 2^16 rows (N / F = 2^17)."""
    assert n * 8 // fold == 1 << 17
    check_proof(ctx, mimc_inputs(n), options(20, 8, 4, 7, fold), layers=layers)


def test_fold16_above_32768_rows(ctx):
    """F = 16 at the smallest n whose first layer (N / 16 = 2^16 rows) is past the quad
    fold's 2^15 rows, so k_fri_fold<16> folds it; the next layer (2^12 rows) takes the
    quad fold. Only slow tests reached the one-lane fold-16 before."""
    n, layers = FOLD16_LANE_CASE
    assert n * 8 // 16 == 1 << 16 and n * 8 // 16 ** 2 == 1 << 12
    check_proof(ctx, mimc_inputs(n), options(20, 8, 4, 7, 16), layers=layers)


# ---------------------------------------------------------------- c. wide AIRs, tiny trees
@pytest.mark.parametrize("fold,layers", [(2, 3), (4, 2), (8, 1)])
def test_global_update(ctx, fold, layers):
    check_proof(ctx, gu_inputs(6, 64), options(20, 16, 4, 7, fold), layers=layers)


@pytest.mark.parametrize("fold,layers", [(2, 5), (4, 3), (8, 2)])
def test_training_update(ctx, fold, layers):
    inputs = tu_inputs(2)
    assert inputs[1].data.shape[1] == 256
    check_proof(ctx, inputs, options(20, 16, 4, 7, fold), layers=layers)


def test_two_row_last_layer(ctx):
    """GlobalUpdate n = 64, B = 2, r = 0, F = 2: six layers of 64 .. 2 rows, all of them
    in the fused tail; the last tree has two leaves."""
    check_proof(ctx, gu_inputs(6, 64), options(20, 2, 4, 0, 2), layers=6)


def test_255_queries(ctx):
    """255 draws over 512 positions, folded six times (256 .. 8 rows): the dedupe of
    every layer's positions and the batch openings do real work."""
    _, tr = check_proof(ctx, mimc_inputs(64), options(255, 8, 4, 0, 2), layers=6)
    assert tr.num_unique_queries < 255


# ---------------------------------------------------------------- d. stage API
@pytest.mark.parametrize("fold", FACTORS)
def test_stages(ctx, fold):
    """The session stages with the host channel == zkp_prove == the oracle."""
    air, trace, pub_el = mimc_inputs(256)
    opts = options(20, 8, 4, 7, fold)
    s = _native.Session(ctx, air, 1, 256, list(pub_el), opts)
    try:
        assert s.fri_layers == fri_layers(256, 8, 7, fold)
    finally:
        s.close()
    gpu = check_by_stages(ctx, air, trace.data, list(pub_el), opts)
    ref, _ = O.prove(air, trace.to_bytes(), 1, 256, to_bytes(pub_el), opts)
    assert gpu == ref


# ---------------------------------------------------------------- e. fused tail
@pytest.mark.parametrize("fold,large_layers", [(2, 3), (4, 1), (8, 1), (16, 0)])
def test_fused_tail(ctx, fold, large_layers):
    """MiMC n = 256, B = 8, r = 7: the layers of <= 128 rows, their coin steps and the
    remainder are one k_fri_tail launch; the fold kernel runs for the larger layers
    only. F = 16 (one layer of 128 rows) is the proof and the launch count it was."""
    ctx.set_profiling(True)
    try:
        ctx.reset_stats()
        check_proof(ctx, mimc_inputs(256), options(20, 8, 4, 7, fold))
        table = ctx.stats_table()
        assert table["fri_tail"]["launches"] == 1
        assert table.get(f"fri_fold{fold}", {"launches": 0})["launches"] == large_layers
        for other in (2, 4, 8, 16):
            assert other == fold or f"fri_fold{other}" not in table
    finally:
        ctx.set_profiling(False)
        ctx.reset_stats()


# ---------------------------------------------------------------- f. refusals
@pytest.mark.parametrize("fold,n,blowup,r", [PAST_TRACE, TOO_DEEP])
def test_refused_on_the_host(ctx, fold, n, blowup, r):
    """F^L > n, and L > 16: zkp_prove, zkp_prove_device and zkp_session_create return
    ZKP_ERR_INVALID_OPTIONS before anything is launched (the statistics table of a
    profiling context stays empty)."""
    layers = fri_layers(n, blowup, r, fold)
    assert fold ** layers > n or layers > MAX_FRI_LAYERS
    opts = options(20, blowup, 4, r, fold)
    air, pub_el = AIR_MIMC, (1, 2)
    trace = np.zeros((1, n, 2), dtype=np.uint64)  # never read: the options are refused first
    ctx.set_profiling(True)
    d = ctx.alloc(trace.nbytes)
    try:
        calls = {"zkp_prove": lambda: ctx.prove(air, trace, pub_el, opts),
                 "zkp_prove_device": lambda: ctx.prove_device(air, d, 1, n, pub_el, opts),
                 "zkp_session_create": lambda: _native.Session(ctx, air, 1, n, list(pub_el), opts)}
        for name, call in calls.items():
            ctx.reset_stats()
            with pytest.raises(ZkpError) as e:
                call()
            assert e.value.code == ZKP_ERR_INVALID_OPTIONS, name
            assert ctx.stats_table() == {}, name
    finally:
        ctx.free(d)
        ctx.set_profiling(False)
        ctx.reset_stats()


def test_sharded_group_refuses_other_factors(ctx):
    """A group of two ranks keeps folding factor 16: at F = 4 both ranks get
    ZKP_ERR_INVALID_OPTIONS from the arguments alone (no collective, none blocks), and
    the same group then proves the F = 16 case; a group of one takes every factor."""
    air, trace, pub_el = mimc_inputs(1 << 11)
    comms = _native.local_group(2)
    ctxs = [_native.Context(0) for _ in range(2)]

    def run_group(opts):
        out = [None, None]

        def run(r):
            try:
                out[r] = ctxs[r].prove_sharded(comms[r], air, trace.data, pub_el, opts)
            except ZkpError as e:
                out[r] = e
        threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        return out
    try:
        for res in run_group(options(20, 8, 4, 7, 4)):
            assert isinstance(res, ZkpError) and res.code == ZKP_ERR_INVALID_OPTIONS
        opts = options(20, 8, 4)
        ref, _ = O.prove(air, trace.to_bytes(), 1, 1 << 11, to_bytes(pub_el), opts)
        for res in run_group(opts):
            assert not isinstance(res, ZkpError), res
            assert res[0] == ref
    finally:
        for c in comms:
            c.close()
        for c in ctxs:
            c.close()
    one = _native.local_group(1)[0]
    try:
        opts = options(20, 8, 4, 7, 4)
        got, _ = ctx.prove_sharded(one, air, trace.data, pub_el, opts)
        ref, _ = O.prove(air, trace.to_bytes(), 1, 1 << 11, to_bytes(pub_el), opts)
        assert got == ref
    finally:
        one.close()
