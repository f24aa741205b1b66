"""CPU: the case tables of challenge_cases.py against the oracle alone. The grinding
nonces recorded there are the oracle's minimum nonces and meet the conditions the GPU
tests rely on (a minimum inside k_grind_all's first pass, past it, past two passes;
proofs whose nonce lies past k_grind's first chunk), and no listed OOD point lies on
the LDE coset."""
import pytest

import oracle_ref as O
from challenge_cases import (GRIND_CHUNK, GRIND_NONCES, GRIND_PASS, GRIND_PROOFS, SHAPES, coset_points,
                             grind_proof_options, grind_seed, lde_size, on_lde_coset, z_cases)
from zk_stark_project_amd import AIR_MIMC, MimcProver
from zk_stark_project_amd.field import P, to_bytes


@pytest.mark.parametrize("bits", sorted(GRIND_NONCES))
def test_grind_seed_table(bits):
    got = [O.grind(O.blake3(grind_seed(i)), bits) for i in range(len(GRIND_NONCES[bits]))]
    assert got == GRIND_NONCES[bits]
    if bits == 20:
        assert sum(v > GRIND_PASS for v in got) >= 2
        assert any(v > 2 * GRIND_PASS for v in got)
        assert any(v < GRIND_PASS for v in got)


@pytest.mark.parametrize("name", list(GRIND_PROOFS))
def test_grind_proof_table(name):
    g = GRIND_PROOFS[name]
    opts = grind_proof_options(g)
    p = MimcProver(opts)
    trace = p.build_trace(g.start, g.n)
    _, tr = O.prove(AIR_MIMC, trace.to_bytes(), 1, g.n, to_bytes(p.get_pub_inputs(trace).to_elements()), opts)
    assert tr.pow_nonce == g.nonce
    assert g.nonce > (GRIND_PASS if name == "device_tail" else GRIND_CHUNK + 1)


@pytest.mark.parametrize("name", list(SHAPES))
def test_ood_points_off_the_lde_coset(name):
    sp = SHAPES[name]
    N = lde_size(sp)
    for z in z_cases(sp).values():
        assert pow(z, N, P) != pow(3, N, P) and not on_lde_coset(z, sp)
    for z in coset_points(sp):
        assert pow(z, N, P) == pow(3, N, P) and on_lde_coset(z, sp)
