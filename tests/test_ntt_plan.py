"""The NTT pass plan (csrc/ntt_plan.hpp), checked on the CPU.

tests/native/plan_dump.cpp includes only that header; it is compiled with the host
compiler and its dump for logn 1..28 x {DIT, DIF} x {1, 8} batches is compared with
the plan written out below, which is the production plan the measurements in
DESIGN.md §4 were taken with. The set of k_ntt8 instantiations the plan can ask for
is the list ZKP_NTT8_KERNELS in csrc/ntt.hip: a plan change has to touch both."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# K of each pass, in stage order. Below 2^11 the radix-2 path; 2^17-2^20 below.
PLAN_K = {
    1: [1], 2: [2], 3: [3], 4: [4], 5: [5], 6: [6], 7: [7], 8: [8], 9: [3, 6], 10: [3, 7],
    11: [11],
    12: [6, 6], 13: [6, 7], 14: [6, 8], 15: [8, 7], 16: [8, 8],
    21: [6, 8, 7], 22: [6, 8, 8], 23: [8, 8, 7], 24: [8, 8, 8],
    25: [6, 6, 6, 7], 26: [6, 6, 6, 8], 27: [6, 6, 8, 7], 28: [6, 6, 8, 8],
}
# 2^17-2^20: the 11-stage pass is the one with lo = 0
PLAN_K_DIT = {17: [11, 6], 18: [11, 7], 19: [11, 8], 20: [11, 9]}
PLAN_K_DIF = {17: [6, 11], 18: [7, 11], 19: [8, 11], 20: [9, 11]}

# (dit, threads, K, small) of every k_ntt8 the plan launches
KERNELS = {
    (1, 256, 6, 1), (1, 256, 8, 1), (1, 256, 11, 1),
    (1, 256, 6, 0), (1, 256, 7, 0), (1, 256, 8, 0), (1, 256, 9, 0), (1, 512, 9, 0),
    (0, 256, 6, 1), (0, 256, 7, 1), (0, 256, 8, 1), (0, 256, 11, 1),
    (0, 256, 6, 0), (0, 256, 7, 0), (0, 256, 8, 0), (0, 256, 9, 0), (0, 512, 9, 0),
}


def expected():
    rows = []
    for logn in range(1, 29):
        for dit in (0, 1):
            for batches in (1, 8):
                ks = PLAN_K.get(logn) or (PLAN_K_DIT if dit else PLAN_K_DIF)[logn]
                s0 = 0
                for p, k in enumerate(ks):
                    lo = s0 if dit else logn - s0 - k
                    threads = 512 if k == 9 and batches >= 8 else 256
                    rows.append((logn, dit, batches, p, k, s0, lo, threads, int(lo == 0)))
                    s0 += k
    return rows


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(HERE, "native", "plan_dump.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return [tuple(int(x) for x in line.split()) for line in out.splitlines()]


def test_ntt_plan(dump):
    assert len(KERNELS) == 17
    assert dump == expected()
    plans = {}
    for logn, dit, batches, p, k, s0, lo, threads, small in dump:
        plans.setdefault((logn, dit, batches), []).append((k, lo, small))
    assert len(plans) == 28 * 2 * 2
    for (logn, dit, batches), passes in plans.items():
        assert sum(k for k, _, _ in passes) == logn
        if logn >= 11:
            zero = [i for i, (_, lo, small) in enumerate(passes) if lo == 0]
            assert zero == [0 if dit else len(passes) - 1], (logn, dit, passes)
            assert [small for _, _, small in passes] == [int(lo == 0) for _, lo, _ in passes]
    assert {(r[1], r[7], r[4], r[8]) for r in dump if r[0] >= 11} == KERNELS
