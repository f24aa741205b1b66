"""Field-op fast paths and the NTT rounds' exact recomputation on the GPU.

The product and sum forms skip the exact canonical select unless a lane needs it
(felt_dev.hpp canon_rare / add_sum, and the NTT rounds' deferred check that redoes
a round with the exact forms). Random data reaches those branches about once per
2^32 operations, so the proof-level parity tests never take them on purpose; these
native checks drive them (values at p - 1 against small values, sums in [p, 2^128) of
operands near 2^127, products whose residue sits at the top of the range or aliases past
2^128) and compare with the host's portable arithmetic and a host DFT.

tests/native/ntt_check.cpp is built twice: ntt_check with ntt.hip as the library compiles
it (the values), ntt_check_count with ZKP_COUNT_REDO, whose per-site wave counters show
that every case reached the redo it was built for. Its groups, one test function each:
  whole     45 cases, 2^11 .. 2^21, in place, patterns at the transform's input
  pass-*    every k_ntt8 instantiation launched alone, every stage of it crafted (751 cases
            over 6 DIT + 7 DIF passes; 28 thinned cases over the four 9-stage passes at 2^20):
            under the counter every register round of all 17 instantiations is redone
  lde       the prover's coset-LDE launch (60 cases: B = 2, 8, 16; 2^11 .. 2^17, both grid
            orders); the staged coset-scale reload and the first round both counted
  forms     interpolation, DIF with a scale, sequence launches (88 cases)
  radix2    2^1 .. 2^10 through k_ntt_pass (60 cases, values only)
  big       2^22 and 2^23, both directions (4 cases)
tests/test_gpu_ntt_forms.py drives the same data through the library's entry points.
Binaries built by __graft_entry__.build() (tests/native/Makefile)."""
import os
import re
import subprocess

import pytest

from test_ntt_plan import KERNELS

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
BINARIES = ("ntt_check", "ntt_check_count")


def run(binary, *args, timeout=240):
    path = os.path.join(HERE, binary)
    assert os.path.exists(path), f"{path} not built (run __graft_entry__.build())"
    r = subprocess.run([path, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def ntt_group(binary, group, cases):
    """One group of ntt_check / ntt_check_count: `cases` cases, none mismatching (the counting
    build also fails a case whose targeted redo site counted no wave)."""
    out = run(binary, group)
    assert out.strip().splitlines()[-1] == f"{binary}: {cases} cases, 0 mismatching", out[-2000:]
    return out


def redone_instantiations(out):
    """(dit, threads, K, small) of the TABLE lines of ntt_check_count whose every round was redone"""
    rows = re.findall(r"^TABLE k_ntt8<(DIT|DIF), (\d+), (\d+), (SMALL|-)> .*$", out, re.M)
    assert "NEVER" not in out
    return {(int(d == "DIT"), int(nt), int(k), int(s == "SMALL")) for d, nt, k, s in rows}


def test_field_op_edge_cases():
    out = run("ubench_bfly", "--check")
    assert "all equal to the host's portable arithmetic" in out


def test_ntt_exact_redo_rounds():
    ntt_group("ntt_check", "whole", 45)


def test_ntt_exact_redo_rounds_counted():
    """the dense and sparse patterns of the same 45 cases are counted in the first round"""
    ntt_group("ntt_check_count", "whole", 45)


@pytest.mark.parametrize("binary", BINARIES)
@pytest.mark.parametrize("group,dit,cases", [("pass-dit", 1, 224), ("pass-dif", 0, 257)])
def test_ntt_every_pass_every_round(binary, group, dit, cases):
    out = ntt_group(binary, group, cases)
    if binary == "ntt_check_count":
        assert redone_instantiations(out) == {k for k in KERNELS if k[0] == dit and k[2] != 9}


@pytest.mark.parametrize("binary", BINARIES)
def test_ntt_nine_stage_passes(binary):
    out = ntt_group(binary, "pass-9", 28)
    if binary == "ntt_check_count":
        assert redone_instantiations(out) == {k for k in KERNELS if k[2] == 9}


@pytest.mark.parametrize("binary", BINARIES)
def test_ntt_lde_launch(binary):
    out = ntt_group(binary, "lde", 60)
    # the launch condition of every case is on the side it was written for
    assert len(re.findall(r"tile_major=0", out)) == 36 and len(re.findall(r"tile_major=1", out)) == 24


@pytest.mark.parametrize("binary", BINARIES)
def test_ntt_interpolation_scale_sequence_launches(binary):
    ntt_group(binary, "forms", 88)


@pytest.mark.parametrize("binary", BINARIES)
def test_ntt_radix2_sizes(binary):
    ntt_group(binary, "radix2", 60)


@pytest.mark.parametrize("binary", BINARIES)
def test_ntt_largest_sizes(binary):
    ntt_group(binary, "big", 4)


def test_eval_mimc_exact_redo():
    """k_eval_mimc's exact recomputation, driven on purpose (tests/native/eval_check.cpp):
    every output equals the host's exact arithmetic and the redo branch was taken."""
    out = run("eval_check")
    assert ", 0 mismatching," in out, out
    redo = int(out.strip().splitlines()[-1].split(",")[-1].split()[0])
    assert redo > 0, out
