"""Shapes and challenge values of test_gpu_session_challenges.py, and the grinding
tables it shares with test_challenge_cases.py (CPU).

A stage session (include/zkp.h `zkp_session_*`) takes every Fiat-Shamir challenge as
an argument, so its caller may pass values no coin ever draws: 0, 1, p - 1, one-hot
vectors, an OOD point inside the trace domain, dense or adjacent query positions.
The tables below are those values per shape; the CPU oracle computes the reference
for each of them in coefficient form (oracle_prove_stages_with).

Notation: n trace rows, B blowup, N = n * B, F folding factor, r remainder degree,
L FRI layers, w trace width, C composition columns, ce constraint-evaluation blowup.
Everything here is checked when the module is imported, so a wrong row fails before
anything is launched."""
from collections import namedtuple

from air_strided_cases import root_of_unity
from folding_cases import fri_layers, options
from zk_stark_project_amd.field import P

Shape = namedtuple("Shape", "kind n blowup fold r w ce C num_t num_a")

# The smallest shapes at which each path still exists, with N >= 512 so that 255
# positions fit. MiMC (1 transition, 2 assertions) at every folding factor, the
# remainder degrees those of folding_cases.DEPTH_CASES with at least 2 layers for
# F <= 4; GlobalUpdate at the shape with lazily filled paired columns; TrainingUpdate
# at batch size 2 (256 rows, its smallest trace for that batch); "program": MiMC as
# a registered program with its periodic column and one strided assertion group
# (air_strided_cases.mimc_strided_program, "periodic" form), whose proof is the
# built-in AIR's, so the oracle's MiMC is its reference.
SHAPES = {
    "mimc_f2": Shape("mimc", 64, 8, 2, 7, 1, 8, 6, 1, 2),
    "mimc_f4": Shape("mimc", 64, 8, 4, 0, 1, 8, 6, 1, 2),
    "mimc_f8": Shape("mimc", 64, 8, 8, 0, 1, 8, 6, 1, 2),
    "mimc_f16": Shape("mimc", 64, 8, 16, 7, 1, 8, 6, 1, 2),
    "global_update": Shape("global_update", 64, 16, 16, 7, 120, 2, 1, 60, 120),
    "training_update": Shape("training_update", 256, 16, 16, 7, 240, 2, 1, 240, 240),
    "program": Shape("program", 64, 8, 16, 7, 1, 8, 6, 1, 2),
}
GU_DEVICES, TU_BATCH = 6, 2
QUERIES = 20  # the coin's draw where the positions are not overridden


def shape_options(sp):
    return options(QUERIES, sp.blowup, 4, sp.r, sp.fold)


def lde_size(sp):
    return sp.n * sp.blowup


def layers(sp):
    return fri_layers(sp.n, sp.blowup, sp.r, sp.fold)


for _sp in SHAPES.values():
    assert lde_size(_sp) >= 512 and _sp.fold ** layers(_sp) <= _sp.n
assert [layers(SHAPES[k]) for k in ("mimc_f2", "mimc_f4", "mimc_f8", "mimc_f16")] == [3, 3, 2, 1]
assert layers(SHAPES["global_update"]) == 1 and layers(SHAPES["training_update"]) == 2


def one_hot(k, i):
    return [int(j == i) for j in range(k)]


# ---------------------------------------------------------------- challenge sets
def coeff_cases(sp):
    """Composition coefficients: num_t transition coefficients, then one per assertion."""
    k = sp.num_t + sp.num_a
    return {"zero": [0] * k, "one": [1] * k, "minus_one": [P - 1] * k,
            "first_transition": one_hot(k, 0), "last_transition": one_hot(k, sp.num_t - 1),
            "first_assertion": one_hot(k, sp.num_t), "last_assertion": one_hot(k, k - 1)}


def z_trace_rows(sp):
    """The OOD points inside the trace domain: name -> k with z = w_n^k."""
    return {"one": 0, "omega_1": 1, "omega_half": sp.n // 2, "omega_last": sp.n - 1}


def z_cases(sp):
    wn = root_of_unity(sp.n.bit_length() - 1)
    out = {"zero": 0, "two": 2, "p_minus_two": P - 2}
    out.update({name: pow(wn, k, P) for name, k in z_trace_rows(sp).items()})
    return out


def on_lde_coset(z, sp):
    """z or z * w_n on the LDE coset 3 * <w_N> (x is on it iff x^N = 3^N): zkp_ood_frame refuses it."""
    N = lde_size(sp)
    zg = z * root_of_unity(sp.n.bit_length() - 1) % P
    return pow(z, N, P) == pow(3, N, P) or pow(zg, N, P) == pow(3, N, P)


def coset_points(sp):
    """Refused OOD points: 3 and 3 * w_N^5."""
    return [3, 3 * pow(root_of_unity(lde_size(sp).bit_length() - 1), 5, P) % P]


def deep_cases(sp):
    """DEEP coefficients: w trace columns, then C composition columns."""
    k = sp.w + sp.C
    return {"zero": [0] * k, "minus_one": [P - 1] * k, "first_trace": one_hot(k, 0),
            "last_trace": one_hot(k, sp.w - 1), "last_composition": one_hot(k, k - 1)}


def alpha_cases(sp):
    L = layers(sp)
    return {"zero": [0] * L, "one": [1] * L, "minus_one": [P - 1] * L, "small": [2 + l for l in range(L)],
            "zero_last": [7 + l for l in range(L - 1)] + [0]}


def position_cases(sp):
    """Sorted unique LDE positions; `fold_row`: the F positions of one first-layer row."""
    N, F = lde_size(sp), sp.fold
    return {"first": [0], "last": [N - 1], "both_ends": [0, N - 1], "siblings": [N // 4 + 2, N // 4 + 3],
            "fold_row": [5 + j * (N // F) for j in range(F)], "dense_low": list(range(255)),
            "dense_high": list(range(N - 255, N)), "every_second": list(range(0, N, 2))[:255]}


def requery_sets(sp):
    """Two disjoint position sets for A, B, A on one session."""
    N = lde_size(sp)
    return list(range(1, N, 7))[:60], list(range(3, N, 7))[:60]


def combined_case(sp):
    """Every site overridden in one run."""
    return {"coeffs": coeff_cases(sp)["minus_one"], "z": z_cases(sp)["omega_last"],
            "deep_coeffs": deep_cases(sp)["last_composition"], "alphas": alpha_cases(sp)["zero_last"],
            "positions": position_cases(sp)["dense_high"]}


for _sp in SHAPES.values():
    # 3 generates the full multiplicative group, so none of the chosen points is on 3 * <w_N>
    assert not any(on_lde_coset(z, _sp) for z in z_cases(_sp).values())
    assert all(on_lde_coset(z, _sp) for z in coset_points(_sp))
    assert all(0 <= v < P for c in (coeff_cases, deep_cases, alpha_cases) for vec in c(_sp).values() for v in vec)
    for _pos in list(position_cases(_sp).values()) + list(requery_sets(_sp)):
        assert 1 <= len(_pos) <= 255 and _pos == sorted(set(_pos)) and _pos[-1] < lde_size(_sp)
    assert len(position_cases(_sp)["every_second"]) == 255
    assert position_cases(_sp)["siblings"][0] % 2 == 0
    assert len({p % (lde_size(_sp) // _sp.fold) for p in position_cases(_sp)["fold_row"]}) == 1
    assert not set(requery_sets(_sp)[0]) & set(requery_sets(_sp)[1])

# ---------------------------------------------------------------- grinding
GRIND_PASS = 1024 * 256        # nonces per grid-stride pass of k_grind_all (csrc/merkle.hip)
GRIND_CHUNK = 1 << 22          # ProofRun::grind_chunk: nonces per k_grind launch (csrc/prover_internal.hpp)


def grind_seed(i):
    """Seed i of the sweep: BLAKE3(b"grind-<i>") (hashed by the caller's oracle binding)."""
    return b"grind-%d" % i


# minimum nonce of seed i at 20 and 22 bits, from the oracle (test_challenge_cases.py derives them again)
GRIND_NONCES = {
    20: [223633, 44119, 1118189, 377689, 473953, 575998, 5105856, 251420],
    22: [4296426, 627102, 5885652, 10768023, 5157970, 7158228, 5602748, 1379642],
}
for _bits, _row in GRIND_NONCES.items():
    assert len(_row) == 8
assert sum(v > GRIND_PASS for v in GRIND_NONCES[20]) >= 2      # past the first pass
assert any(v > 2 * GRIND_PASS for v in GRIND_NONCES[20])       # past the second
assert any(v < GRIND_PASS for v in GRIND_NONCES[20])           # inside the first
assert any(v > 2 * GRIND_CHUNK for v in GRIND_NONCES[22])

# MiMC proofs whose nonce lies past the first unit of each grinding kernel; the start value
# (MimcProver.build_trace's seed) was searched on the CPU with the oracle.
#   host_tail:   remainder domain 512 > 256 points, so no device tail: ProofRun::grind_stage
#                runs k_grind chunk by chunk from nonce 1 (F = 8: at F = 16 the last layer
#                of this n, B, r has 128 points and takes the device tail)
#   two_ranks:   an in-process group of two (F = 16, default remainder): the first chunk on
#                the device coin, the following ones from grind_stage
#   device_tail: world 1 with the device query tail: k_grind_all to completion
GrindProof = namedtuple("GrindProof", "n start blowup grind r fold world nonce")
GRIND_PROOFS = {
    "host_tail": GrindProof(4096, 2, 8, 22, 63, 8, 1, 12727370),
    "two_ranks": GrindProof(512, 8, 8, 22, 7, 16, 2, 8932330),
    "device_tail": GrindProof(64, 1, 8, 20, 7, 16, 1, 809716),
}


def grind_proof_options(g):
    return options(QUERIES, g.blowup, g.grind, g.r, g.fold)


def last_domain(g):
    return g.n * g.blowup // g.fold ** fri_layers(g.n, g.blowup, g.r, g.fold)


assert last_domain(GRIND_PROOFS["host_tail"]) == 512 and last_domain(GRIND_PROOFS["device_tail"]) <= 256
assert GRIND_PROOFS["host_tail"].nonce > GRIND_CHUNK + 1 and GRIND_PROOFS["two_ranks"].nonce > GRIND_CHUNK + 1
assert GRIND_PROOFS["device_tail"].nonce > GRIND_PASS
