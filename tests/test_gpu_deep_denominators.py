"""The DEEP inverse table: one inversion per LDE point, built beside the OOD frame.

k_deep reads 1 / (x - z) of every LDE point from a table and takes 1 / (x - z w_n)
from the previous row of the same coset, times w_n^-1. The table comes from the
batch inverses of z^8 - y over the 8th powers y of the points (1/8 of them),
expanded 8 points per thread (kernels.hip k_deep_inv_expand).

 * tests/native/deep_inv_check.hip builds the table through launch_deep_denominators
   and compares both denominators of every point with Fermat inverses: n = 8, 16, 64
   and 2^11 over 2, 8 and 32 cosets, the row t = 0 of every coset included.
 * Whole proofs, byte for byte against the CPU oracle. The FRI layer-0 root covers
   every DEEP value, so equal bytes check every point, not only the queried ones.
   MiMC accepts no trace below 64 rows (build_air), so its lengths are 64 and 2^10 at
   blowups 8, 16 and 32; the lengths 8 and 16 (one and two groups of 8 per coset) run
   through GlobalUpdate, whose 120 columns also take the combined-column DEEP path,
   and TrainingUpdate runs at its smallest shape. Sharded over 2 and 8 in-process
   ranks each rank's table covers its own cosets only; a rank needs 256 rows per
   coset of its Merkle range (ProofRun::init), so 8 ranks prove 2^11 rows, the
   smallest length they accept, and 2 ranks 2^10.
"""
import os
import subprocess

import pytest

import oracle_ref as O
from test_gpu_options import gu_inputs, mimc_inputs, tu_inputs
from zk_stark_project_amd import ProofOptions, _native
from zk_stark_project_amd.field import to_bytes
from zk_stark_project_amd.sharded import prove_local_group

pytestmark = pytest.mark.gpu
NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_inverse_table_matches_fermat_inverses():
    path = os.path.join(NATIVE, "deep_inv_check")
    assert os.path.exists(path), f"{path} not built (run __graft_entry__.build())"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "12 cases, 0 mismatches" in r.stdout, r.stdout


def oracle_bytes(inputs, opts):
    air, trace, pub_el = inputs
    w, n = trace.data.shape[:2]
    return O.prove(air, trace.to_bytes(), w, n, to_bytes(pub_el), opts)[0]


def check_bytes(ctx, inputs, opts):
    air, trace, pub_el = inputs
    gpu, _ = ctx.prove(air, trace.data, pub_el, opts)
    assert gpu == oracle_bytes(inputs, opts)


@pytest.mark.parametrize("blowup", [8, 16, 32])
@pytest.mark.parametrize("n", [64, 1 << 10])
def test_mimc_proof_bytes(ctx, n, blowup):
    check_bytes(ctx, mimc_inputs(n), ProofOptions(20, blowup, 4))


@pytest.mark.parametrize("n", [8, 16])
def test_global_update_combined_column_proof_bytes(ctx, n):
    inputs = gu_inputs(2, n)
    assert inputs[1].data.shape[0] == 120
    check_bytes(ctx, inputs, ProofOptions(20, 16, 4))


def test_training_update_smallest_proof_bytes(ctx):
    check_bytes(ctx, tu_inputs(0), ProofOptions(20, 16, 4))


@pytest.fixture(scope="module")
def rank_ctxs():
    cs = [_native.Context(0) for _ in range(8)]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.parametrize("n,R", [(1 << 10, 2), (1 << 11, 8)])
def test_mimc_sharded_proof_bytes(rank_ctxs, n, R):
    opts = ProofOptions(20, 8, 4)
    inputs = mimc_inputs(n)
    air, trace, pub_el = inputs
    ref = oracle_bytes(inputs, opts)
    res = prove_local_group(R, air, trace.data, pub_el, opts, contexts=rank_ctxs[:R])
    for r, (data, _) in enumerate(res):
        assert data == ref, f"rank {r} proof differs from the oracle"
