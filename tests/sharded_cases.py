"""Cases of the sharded option and shape sweep (test_gpu_sharded_options.py): the
smallest shapes at which a proof over R ranks takes each path that the options or
the shape select, with the thresholds of csrc/prover.cpp and csrc/prover_shard.cpp
restated in plain Python. Every table below is checked against those restatements
when this module is imported, so a wrong row fails before anything is launched.

Notation: n trace rows, B blowup, R ranks, r remainder degree, L FRI layers
(option_cases.fri_layers), F = 16 values per FRI row."""
from option_cases import HORNER, LINEAR, fri_layers


def ilog2(x):
    assert x > 0 and x & (x - 1) == 0, x
    return x.bit_length() - 1


def min_rows(R):
    """ProofRun::init: logn >= logR + 8 (256 rows per coset in every rank's Merkle range)."""
    return 256 * R


def accepted(n, B, R):
    """ProofRun::init's sharding checks: R <= B and n >= 256 R."""
    return R <= B and n >= min_rows(R)


def sharded_fri_layers(n, R, L):
    """ProofRun::fri_layers: layer l stays coset-sharded while every layer before it did
    and (m / 16) >> logR >= 16, m = n / 16^l (its tree has m / 16 rows per coset)."""
    k = 0
    while k < L and (n // 16 ** (k + 1)) // R >= 16:
        k += 1
    return k


def last_domain(n, B, L):
    """Points of the last FRI layer (the remainder's domain): at most 256 for the device remainder."""
    return B * n // 16 ** L


def tree_chunks(rows_per_coset, R):
    """commit_rows_sharded: the leaf exchange of a sharded tree runs in 4 chunks when each
    rank's range has 2^12 rows per coset (logrows - logR >= 12), else in 1."""
    return 4 if ilog2(rows_per_coset) - ilog2(R) >= 12 else 1


def all_to_all_calls(n, R, L):
    """all_to_all calls of one rank in one proof without a second attempt: 1 for the
    composition exchange (ProofRun::composition_exchange) and, for every sharded tree
    (trace, constraint, each sharded FRI layer), one per chunk of its leaf exchange.
    Every other collective of the proof is an all_gather."""
    fri = sum(tree_chunks(n // 16 ** (l + 1), R) for l in range(sharded_fri_layers(n, R, L)))
    return 1 + 2 * tree_chunks(n, R) + fri


def ood_split(n, R):
    """ood_launch: the OOD blocks (2048 coefficients each) are split over the ranks."""
    return (n >> min(ilog2(n), 11)) >= R


def tu_rows(bs):
    """TrainingUpdateProver.trace_length: 2 * 60 state cells per sample, padded to a power of two."""
    return max(1 << (120 * bs - 1).bit_length(), 16)


# ---------------------------------------------------------------- a. FRI replication, remainder, tail
# MiMC (n, R, B, r): L, sharded layers, last domain, all_to_all calls per rank
FRI_SHAPES = {
    (512, 2, 8, 7): (2, 1, 16, 4),        # smallest n at R = 2
    (2048, 8, 8, 7): (2, 1, 64, 4),       # smallest n at R = 8
    (512, 2, 8, 31): (1, 1, 256, 4),      # every layer sharded: replicate(L); device remainder at its limit
    (4096, 8, 8, 255): (1, 1, 2048, 4),   # replicate(L); host remainder of 256 coefficients
    (4096, 2, 8, 0): (3, 1, 8, 4),        # one-coefficient remainder, 16^L = n
    (4096, 8, 8, 0): (3, 1, 8, 4),
    (8192, 2, 8, 31): (2, 2, 256, 11),    # two sharded layers, then replicate(L); trace and constraint trees in 4 chunks
    (1 << 17, 2, 8, 7): (4, 3, 16, 15),   # three sharded layers; layer 0's tree (2^13 rows per coset) in 4 chunks
}
FRI_BIG = (1 << 17, 2, 8, 7)  # single-GPU comparison only, grinding 4 only, not in the counting run
DEVICE_TAIL_MAX = 256

for (n, R, B, r), (L, sh, last, calls) in FRI_SHAPES.items():
    assert accepted(n, B, R), (n, R, B)
    assert fri_layers(n, B, r) == L and 16 ** L <= n, (n, B, r)
    assert sharded_fri_layers(n, R, L) == sh, (n, R, L)
    assert last_domain(n, B, L) == last, (n, B, L)
    assert all_to_all_calls(n, R, L) == calls, (n, R, L)
assert not accepted(256, 8, 2) and not accepted(1024, 8, 8)  # the first two rows are the smallest accepted
assert all(sh == L for (n, R, B, r), (L, sh, _, _) in FRI_SHAPES.items() if r in (31, 255))  # replicate(L)
assert tree_chunks((1 << 17) // 16, 2) == 4 and tree_chunks(8192 // 16, 2) == 1
# the device remainder at its limit, and the host remainder above it
assert {last for (_, _, _, r), (_, _, last, _) in FRI_SHAPES.items() if r == 31} == {DEVICE_TAIL_MAX}
assert FRI_SHAPES[(4096, 8, 8, 255)][2] > DEVICE_TAIL_MAX

# the trace and constraint trees in 4 chunks at larger R (MiMC, default options): (n, R)
CHUNKED_TREES = [(1 << 14, 4), (1 << 15, 8)]
for n, R in CHUNKED_TREES:
    assert tree_chunks(n, R) == 4 and tree_chunks(n // 2, R) == 1

# ---------------------------------------------------------------- b. batching methods through k_shard_top
ASYMMETRIC_PAIRS = [(LINEAR, HORNER), (HORNER, LINEAR)]
GU_METHODS = (512, 16, 2)                  # (n, B, R): 180 coefficients
MIMC_METHODS = (512, 8, 2)                 # 3 coefficients
# TrainingUpdate, 480 coefficients: (batch size, n, B, R). 3 is the smallest batch with 512 rows; 512
# rows admit R = 2 only, so R = 8 runs at the smallest batch with 2048 rows
TU_METHODS = [(3, 512, 16, 2), (9, 2048, 16, 8)]
for bs, n, B, R in TU_METHODS:
    assert tu_rows(bs) == n and tu_rows(bs - 1) < n and accepted(n, B, R) and not accepted(n // 2, B, R)
assert accepted(*GU_METHODS) and accepted(*MIMC_METHODS)

# ---------------------------------------------------------------- c. query counts
QUERY_COUNTS = (1, 2, 255)
QUERY_GRINDS = (0, 3)
MIMC_QUERIES = [(2048, 8, 2), (2048, 8, 8)]  # (n, B, R)
GU_QUERIES = (512, 2, 2)                     # 1024-point domain, Bl = 1
GU_FILL = [(2048, 2), (2048, 8)]             # (n, R): device-resident paired trace, q = 255, reference blowup 16
assert GU_QUERIES[0] * GU_QUERIES[1] == 1024 and GU_QUERIES[1] // GU_QUERIES[2] == 1
assert all(accepted(n, B, R) for n, B, R in MIMC_QUERIES + [GU_QUERIES]) and all(accepted(n, 16, R) for n, R in GU_FILL)

# ---------------------------------------------------------------- d. blowup edges
# (n, B, R). B = R = 4 needs 1024 rows (n >= 256 R): both (4, 4) cases run there, not at 512
GU_BLOWUPS = [(512, 2, 2), (1024, 4, 4), (512, 4, 2), (512, 128, 2), (2048, 64, 8)]
MIMC_BLOWUPS = [(2048, 32, 2), (2048, 32, 4), (2048, 32, 8), (2048, 128, 8)]
TU_BLOWUPS = [(3, 512, 2, 2), (5, 1024, 4, 4)]  # (batch size, n, B, R)
for n, B, R in GU_BLOWUPS + MIMC_BLOWUPS + [t[1:] for t in TU_BLOWUPS]:
    assert accepted(n, B, R), (n, B, R)
assert not accepted(512, 4, 4) and all(tu_rows(bs) == n and tu_rows(bs - 1) < n for bs, n, _, _ in TU_BLOWUPS)
REFUSED_WORLD = (1024, 2, 4)  # GlobalUpdate (n, B, R): enough rows for R = 4, so R > B is the only reason
assert REFUSED_WORLD[0] >= min_rows(REFUSED_WORLD[2]) and not accepted(*REFUSED_WORLD)
ERR_ARGUMENT = 9  # ZKP_ERR_ARGUMENT (include/zkp.h)

# ---------------------------------------------------------------- e. OOD split at R = 8, traces from HBM
OOD_SPLIT_R8 = (1 << 14, 8)  # (n, R): the smallest n whose OOD is split over 8 ranks
assert ood_split(*OOD_SPLIT_R8) and not ood_split(OOD_SPLIT_R8[0] // 2, 8)
DEVICE_TRACES = {"mimc": (2048, 8, 2), "training_update": (3, 512, 16, 2)}  # (n, B, R) / (batch size, n, B, R)
