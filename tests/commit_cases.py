"""Matrix shapes and inputs of the device commitment sweeps (test_gpu_commit_shapes.py):
every row width the two matrix entry points accept, the widths at which the row hash
changes its BLAKE3 chunk or block count, and the tree sizes at which the tree builder
changes its launches. The shapes are the smallest that reach each path; the kernels
named here are those of launch_merkle_lde and merkle_upper (csrc/merkle.hip)."""
import numpy as np

P = 2**128 - 45 * 2**40 + 1

MIN_WIDTH, MAX_WIDTH = 1, 255
ALL_WIDTHS = tuple(range(MIN_WIDTH, MAX_WIDTH + 1))

# the ends of the narrow range (1..8), of each 64-felt chunk and of a 4-felt block beside them
W_EDGE = (1, 2, 3, 4, 5, 7, 8, 9, 16, 63, 64, 65, 66, 67, 68, 127, 128, 129, 130, 191, 192, 193, 194, 254, 255)

# a. zkp_merkle_commit_rows, every width
ROWS_SWEEP_ROWS = 16

# b. zkp_trace_lde_commit (n, blowup): logB = 1, 4 over every width; logB = 7, 2 over W_EDGE
LDE_FULL_SHAPES = ((8, 2), (8, 16))
LDE_EDGE_SHAPES = ((16, 128), (64, 4))
NO_LDE_SHAPE = (8, 2)
NO_LDE_WIDTHS = (4, 8, 65, 129, 193, 255)  # want_lde=False: the root alone

# c. widths checked against the pure-Python specification as well
SPEC_WIDTHS = (1, 4, 5, 8, 9, 64, 65, 128, 129, 192, 193, 255)
SPEC_ROWS = 4
SPEC_LDE_SHAPE = (8, 2)

# row-constant matrices (every felt 0, every felt p - 1)
CONST_WIDTHS = (4, 8, 64, 255)
CONST_VALUES = (0, P - 1)
CONST_ROWS = 16
CONST_LDE_SHAPE = (8, 2)

# d. tree sizes at width 1
ROW_LADDER = tuple(1 << k for k in range(1, 21))     # zkp_merkle_commit_rows rows
LDE_LADDER_BLOWUP = 8
LDE_LADDER = tuple(1 << k for k in range(3, 18))     # zkp_trace_lde_commit n
WIDE_TREES = ((65, 1 << 12), (255, 1 << 12))         # (width, rows): lane-pass grids of 8 blocks

# e. refused shapes: ZKP_ERR_TRACE_SHAPE (include/zkp.h)
ERR_TRACE_SHAPE = 3
REFUSED_WIDTHS = (0, 256)
REFUSED_ROWS = (1, 3)
REFUSED_N = (4, 12)


def rand_felts(width, rows, *shape_tag):
    """(width, rows, 2) uint64 column-major matrix of canonical felts over the whole range:
    low word uniform in [0, 2^64), high word uniform in [0, 2^64 - 1), which is always
    below p (p's high word is 2^64 - 1). Seeded by the shape (and shape_tag, e.g. the
    blowup), so that a failing width reproduces on its own."""
    rng = np.random.default_rng([width, rows, *shape_tag])
    a = np.empty((width, rows, 2), dtype=np.uint64)
    a[..., 0] = rng.integers(0, 2**64, size=(width, rows), dtype=np.uint64)
    a[..., 1] = rng.integers(0, 2**64 - 1, size=(width, rows), dtype=np.uint64)
    return a


def const_felts(width, rows, value):
    a = np.empty((width, rows, 2), dtype=np.uint64)
    a[..., 0] = np.uint64(value & (2**64 - 1))
    a[..., 1] = np.uint64(value >> 64)
    return a


def to_ints(a):
    """(..., 2) uint64 -> nested lists of Python ints."""
    lo, hi = a[..., 0].astype(object), a[..., 1].astype(object)
    return (lo + hi * 2**64).tolist()


def ranges(ws):
    """[129, 130, 131, 192, 200] -> '129..131, 192, 200' (a failing sweep shows its pattern)"""
    out, ws = [], sorted(ws)
    i = 0
    while i < len(ws):
        j = i
        while j + 1 < len(ws) and ws[j + 1] == ws[j] + 1:
            j += 1
        out.append(str(ws[i]) if i == j else f"{ws[i]}..{ws[j]}")
        i = j + 1
    return ", ".join(out)
