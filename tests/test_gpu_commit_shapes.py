"""Every row width and tree size through the two device entry points that commit a
matrix, zkp_merkle_commit_rows and zkp_trace_lde_commit, byte for byte against the CPU
oracle and, at the widths where the row hash changes shape, against the pure-Python
specification (tests/golden/spec.py), which shares no code with the oracle.

Both entry points pick their device code from (cols, logB, L) alone, L = leaves of the
tree (launch_merkle_lde and merkle_upper, csrc/merkle.hip). What each test reaches:

  leaf pass (launch_merkle_lde)            cols      logB   L        tests
  ---------------------------------------  --------  -----  -------  -----------------------------
  k_merkle_leaf2<cols>, hash_felts_c       1..8      any    any      rows_width_sweep, lde_width_sweep,
                                                                     both ladders (cols = 1)
  k_merkle_lane<0, 1>, hash_felts          9..255    0      any      rows_width_sweep (1..4 chunks),
    row i at src + i                                                 wide_trees (8 blocks)
  k_merkle_lane<0, 1>, hash_felts          9..64     >= 1   any      lde_width_sweep
    coset-major: j = i & (B - 1), t = i >> logB, stride n << logB
  k_merkle_wide, hash_chunk per lane       65..255   >= 1   <= 2^20  lde_width_sweep: 65..128 two chunks,
    a quad per row, an octet per row pair                            129..192 three, 193..255 four
  (k_merkle_lane<0, 1> for cols 65..255 with logB >= 1 and L > 2^20 is not reached:
   the smallest such matrix is 2 GiB)

  lde_width_sweep shapes (n, blowup): (8, 2) logB 1, one coset pair, 16 leaves, 64 of the
  wide kernel's 256 threads valid; (64, 4) logB 2, 256 leaves; (8, 16) logB 4, 128 leaves;
  (16, 128) logB 7, 64 coset pairs, 2048 leaves.

  levels above the leaf pass (merkle_upper over L / 2 nodes), by L:
  zkp_merkle_commit_rows passes no tail, so every k_merkle_fused<2> launch leaves one
  root per block of 512 nodes and the loop launches again    (test_rows_ladder)
    2                leaf pass only (its merge is the root)
    4 .. 1024        one k_merkle_fused<2> block (4 rows: its first merge is the root, no LDS level)
    2048 .. 2^18     k_merkle_fused<2> of 2 .. 256 blocks, then one block over their roots
    2^19, 2^20       k_merkle_lane<2, 2>, then k_merkle_fused<2> of 128 / 256 blocks, then one
  zkp_trace_lde_commit passes the tail counter: the last block of the first
  k_merkle_fused<2> launch of at most 512 blocks finishes the tree  (test_lde_ladder)
    16 .. 1024       one block, its tail a no-op (sweeps; ladder n = 8 .. 128 at blowup 8)
    2048 .. 2^18     2 .. 256 blocks, the last to finish builds the top (n = 256 .. 2^15)
    2^19, 2^20       k_merkle_lane<2, 2>, then 128 / 256 blocks with the tail (n = 2^16, 2^17)

Code that no accepted input reaches, so no test can: k_merkle_leaf2<CC, true> for CC other
than 6, k_leaf_hash_shard<0, CC> for CC other than 1, and k_leaf_hash_shard<0, CC, true>
for CC other than 6: the proofs reach these kernels at their AIRs' column counts only, and
neither entry point here derives a column or shards. A later simplification can remove them. Rows with a derived last column or lazy GlobalUpdate columns and FRI rows
are covered at their AIRs' widths by test_gpu_parity.py, test_gpu_sharded.py and
test_gpu_folding.py.
"""
import ctypes

import numpy as np
import pytest

import commit_cases as C
import oracle_ref as O
import spec

pytestmark = pytest.mark.gpu


def rows_mismatches(ctx, widths, rows):
    bad, seen = [], 0
    for w in widths:
        m = C.rand_felts(w, rows)
        if ctx.merkle_commit_rows(m) != O.merkle_rows(m.tobytes(), w, rows):
            bad.append(w)
        seen += 1
    return bad, seen


def lde_mismatches(ctx, widths, n, blowup):
    """widths whose LDE bytes differ, widths whose root differs, widths visited"""
    bad_lde, bad_root, seen = [], [], 0
    for w in widths:
        tr = C.rand_felts(w, n, blowup)
        lde, root = ctx.trace_lde_commit(tr, blowup)
        olde, oroot = O.trace_lde(tr.tobytes(), w, n, blowup)
        if lde.tobytes() != olde:
            bad_lde.append(w)
        if root != oroot:
            bad_root.append(w)
        seen += 1
    return bad_lde, bad_root, seen


# ---------------------------------------------------------------- a, b: every width
def test_rows_width_sweep(ctx):
    bad, seen = rows_mismatches(ctx, C.ALL_WIDTHS, C.ROWS_SWEEP_ROWS)
    assert seen == 255
    assert not bad, f"root differs from the oracle at widths {C.ranges(bad)}"


@pytest.mark.parametrize("n,blowup", C.LDE_FULL_SHAPES)
def test_lde_width_sweep(ctx, n, blowup):
    bad_lde, bad_root, seen = lde_mismatches(ctx, C.ALL_WIDTHS, n, blowup)
    assert seen == 255
    assert not bad_lde, f"LDE differs from the oracle at widths {C.ranges(bad_lde)}"
    assert not bad_root, f"root differs from the oracle at widths {C.ranges(bad_root)}"


@pytest.mark.parametrize("n,blowup", C.LDE_EDGE_SHAPES)
def test_lde_edge_width_sweep(ctx, n, blowup):
    bad_lde, bad_root, seen = lde_mismatches(ctx, C.W_EDGE, n, blowup)
    assert seen == len(C.W_EDGE) == 25
    assert not bad_lde, f"LDE differs from the oracle at widths {C.ranges(bad_lde)}"
    assert not bad_root, f"root differs from the oracle at widths {C.ranges(bad_root)}"


def test_lde_root_without_lde_output(ctx):
    n, blowup = C.NO_LDE_SHAPE
    bad = []
    for w in C.NO_LDE_WIDTHS:
        tr = C.rand_felts(w, n, blowup)
        lde, root = ctx.trace_lde_commit(tr, blowup, want_lde=False)
        assert lde is None
        if root != ctx.trace_lde_commit(tr, blowup)[1] or root != O.trace_lde(tr.tobytes(), w, n, blowup)[1]:
            bad.append(w)
    assert not bad, f"root without the LDE output differs at widths {C.ranges(bad)}"


# ---------------------------------------------------------------- row-constant matrices
@pytest.mark.parametrize("value", C.CONST_VALUES, ids=["zero", "p-1"])
def test_constant_rows(ctx, value):
    n, blowup = C.CONST_LDE_SHAPE
    bad = []
    for w in C.CONST_WIDTHS:
        m = C.const_felts(w, C.CONST_ROWS, value)
        if ctx.merkle_commit_rows(m) != O.merkle_rows(m.tobytes(), w, C.CONST_ROWS):
            bad.append(("rows", w))
        tr = C.const_felts(w, n, value)
        lde, root = ctx.trace_lde_commit(tr, blowup)
        olde, oroot = O.trace_lde(tr.tobytes(), w, n, blowup)
        # the extension of a constant column is that constant
        if lde.tobytes() != olde or lde.tobytes() != C.const_felts(w, n * blowup, value).tobytes():
            bad.append(("lde", w))
        if root != oroot:
            bad.append(("lde root", w))
    assert not bad, f"constant matrix of {value:#x} differs from the oracle: {bad}"


# ---------------------------------------------------------------- c: a second reference
def test_rows_match_python_spec(ctx):
    rows, bad = C.SPEC_ROWS, []
    for w in C.SPEC_WIDTHS:
        m = C.rand_felts(w, rows)
        cols = C.to_ints(m)
        want = spec.merkle_root([spec.hash_elements([cols[c][i] for c in range(w)]) for i in range(rows)])
        if ctx.merkle_commit_rows(m) != want or O.merkle_rows(m.tobytes(), w, rows) != want:
            bad.append(w)
    assert not bad, f"root differs from spec.py at widths {C.ranges(bad)}"


def test_lde_matches_python_spec(ctx):
    n, blowup = C.SPEC_LDE_SHAPE
    N, bad_lde, bad_root = n * blowup, [], []
    for w in C.SPEC_WIDTHS:
        tr = C.rand_felts(w, n, blowup)
        ext = [spec.naive_lde(col, blowup)[1] for col in C.to_ints(tr)]
        want_lde = b"".join(spec.felts_to_bytes(col) for col in ext)
        want_root = spec.merkle_root([spec.hash_elements([ext[c][i] for c in range(w)]) for i in range(N)])
        lde, root = ctx.trace_lde_commit(tr, blowup)
        olde, oroot = O.trace_lde(tr.tobytes(), w, n, blowup)
        if lde.tobytes() != want_lde or olde != want_lde:
            bad_lde.append(w)
        if root != want_root or oroot != want_root:
            bad_root.append(w)
    assert not bad_lde, f"LDE differs from spec.py at widths {C.ranges(bad_lde)}"
    assert not bad_root, f"root differs from spec.py at widths {C.ranges(bad_root)}"


# ---------------------------------------------------------------- d: tree sizes
def test_rows_ladder(ctx):
    bad = []
    for rows in C.ROW_LADDER:
        m = C.rand_felts(1, rows)
        if ctx.merkle_commit_rows(m) != O.merkle_rows(m.tobytes(), 1, rows):
            bad.append(rows.bit_length() - 1)
    assert len(C.ROW_LADDER) == 20
    assert not bad, f"root differs from the oracle at 2^k rows, k = {C.ranges(bad)}"


@pytest.mark.parametrize("n", C.LDE_LADDER, ids=lambda n: f"2^{n.bit_length() - 1}")
def test_lde_ladder(ctx, n):
    blowup = C.LDE_LADDER_BLOWUP
    tr = C.rand_felts(1, n, blowup)
    lde, root = ctx.trace_lde_commit(tr, blowup)
    olde, oroot = O.trace_lde(tr.tobytes(), 1, n, blowup)
    assert lde.tobytes() == olde
    assert root == oroot


@pytest.mark.parametrize("w,rows", C.WIDE_TREES)
def test_wide_trees(ctx, w, rows):
    m = C.rand_felts(w, rows)
    assert ctx.merkle_commit_rows(m) == O.merkle_rows(m.tobytes(), w, rows)


# ---------------------------------------------------------------- e: refusals
def raw_commit_rows(ctx, buf, w, rows):
    root = ctypes.create_string_buffer(32)
    return ctx.lib.zkp_merkle_commit_rows(ctx.ptr, buf.ctypes.data, w, rows, root)


def raw_lde_commit(ctx, buf, w, n, blowup):
    root = ctypes.create_string_buffer(32)
    return ctx.lib.zkp_trace_lde_commit(ctx.ptr, buf.ctypes.data, w, n, blowup, None, root)


def test_refused_shapes(ctx):
    """Widths 0 and 256, row counts that are not a power of two of at least 2, and trace
    lengths that are not a power of two of at least 8 return ZKP_ERR_TRACE_SHAPE; the
    context commits a small matrix correctly after each."""
    buf = C.rand_felts(256, 16)  # readable at every refused shape

    def still_commits():
        m = C.rand_felts(3, 8)
        assert ctx.merkle_commit_rows(m) == O.merkle_rows(m.tobytes(), 3, 8)
        lde, root = ctx.trace_lde_commit(m, 2)
        assert (lde.tobytes(), root) == O.trace_lde(m.tobytes(), 3, 8, 2)

    for w in C.REFUSED_WIDTHS:
        assert raw_commit_rows(ctx, buf, w, 16) == C.ERR_TRACE_SHAPE, f"width {w}"
        still_commits()
        assert raw_lde_commit(ctx, buf, w, 8, 2) == C.ERR_TRACE_SHAPE, f"width {w}"
        still_commits()
    for rows in C.REFUSED_ROWS:
        assert raw_commit_rows(ctx, buf, 1, rows) == C.ERR_TRACE_SHAPE, f"{rows} rows"
        still_commits()
    for n in C.REFUSED_N:
        assert raw_lde_commit(ctx, buf, 1, n, 2) == C.ERR_TRACE_SHAPE, f"n = {n}"
        still_commits()
