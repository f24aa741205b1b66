"""Proof-option cases shared by the option tests (test_gpu_options.py,
test_verifier.py, test_oracle_golden.py): the shapes are the smallest that reach
each option-selected code path. L below is the FRI layer count: the domain
N = n * B is divided by 16 while it exceeds (r + 1) * B."""
from zk_stark_project_amd import ProofOptions

LINEAR, ALGEBRAIC, HORNER = 0, 1, 2
METHOD_PAIRS = [(c, d) for c in (LINEAR, ALGEBRAIC, HORNER) for d in (LINEAR, ALGEBRAIC, HORNER)]


def options(q, blowup, grind, r=7, constraints=ALGEBRAIC, deep=ALGEBRAIC):
    return ProofOptions(q, blowup, grind, 1, 16, r, constraints, deep)


# MiMC (n, B, r): remainder degree and FRI tail selection
MIMC_REMAINDER_SHAPES = [
    (256, 8, 0), (256, 8, 1), (256, 8, 3),  # L = 2; remainder of 1, 2, 4 coefficients (fused tail, m = 1, 2, 4)
    (4096, 8, 0),                           # L = 3
    (256, 8, 15), (256, 8, 63),             # L = 1
    (256, 8, 255),                          # L = 0, remainder domain 2048: host tail
    (64, 8, 63),                            # L = 0 on a 512-point domain
    (4096, 8, 255),                         # L = 1, remainder domain 2048
    (64, 128, 7),                           # L = 1, remainder domain 512: host tail with grinding
    (64, 64, 7),                            # remainder domain 256: the largest the device tail takes
    (1024, 64, 31),
]

# shapes whose FRI layers do not fit the trace (16^L > n): no verifying proof exists.
# (air, n, B, r); air ids as include/zkp.h (1 = MiMC, 2 = GlobalUpdate)
REFUSED_SHAPES = [(1, 64, 8, 0), (1, 1024, 16, 1), (2, 8, 2, 0)]


def fri_layers(n, blowup, r):
    d, layers = n * blowup, 0
    while d > (r + 1) * blowup:
        d //= 16
        layers += 1
    return layers
