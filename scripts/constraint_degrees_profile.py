#!/usr/bin/env python3
"""What measuring every constraint's actual degree costs, beside a proof of the same shape.

Two workloads on one context, the trace resident in HBM:
  mimc:   the MiMC program of tests/air_program_cases.py at n = 2^16 (one degree-7 constraint with
          a periodic column: degree bound 7, E = 8);
  cols16: 16 columns, next_i = cur_i^3 + cur_{i+1}, at n = 2^14 (16 degree-3 constraints, E = 4).
For each: 5 warm-up and 20 timed calls of Context.constraint_degrees_device, then the same of
Context.prove_device (blowup 8, 40 queries, grinding 16); median and min wall time of both, and
from one more, event-bracketed call of each the per-kernel statistics rows.

Writes profiles/constraint_degrees.json (or --out).

    python scripts/constraint_degrees_profile.py [--warmup 5] [--calls 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from air_program_cases import mimc_program, trace_array  # noqa: E402
from zk_stark_project_amd import AirProgram, MimcProver, ProofOptions, _native  # noqa: E402
from zk_stark_project_amd.field import P  # noqa: E402


def cols16(n):
    w = 16
    rows = [[(3 + 5 * i) % P for i in range(w)]]
    for _ in range(n - 1):
        r = rows[-1]
        rows.append([(pow(r[i], 3, P) + r[(i + 1) % w]) % P for i in range(w)])
    cols = [[row[i] for row in rows] for i in range(w)]
    p = AirProgram(w)
    for i in range(w):
        p.constraint(p.next[i] - (p.cur[i] ** 3 + p.cur[(i + 1) % w]), degree=3)
        p.assertion(i, 0, cols[i][0])
    return p, trace_array(cols), [cols[0][0], cols[0][n - 1]]


def timed(f, warmup, calls):
    for _ in range(warmup):
        f()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


def kernel_rows(ctx, f):
    ctx.reset_stats()
    ctx.set_profiling(True)
    f()
    ctx.set_profiling(False)
    return {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in sorted(ctx.stats_table().items())
            if not k.startswith("host_")}


def run(ctx, program, data, pub, opts, warmup, calls):
    w, n = int(data.shape[0]), int(data.shape[1])
    d = ctx.alloc(data.nbytes)
    ctx.to_device(d, np.ascontiguousarray(data))
    try:
        with program.register() as air:
            degrees = lambda: air.constraint_degrees_device(ctx, d, n)  # noqa: E731
            prove = lambda: ctx.prove_device(air, d, w, n, pub, opts)  # noqa: E731
            rep = degrees()
            assert rep.proof_fits and not rep.under, rep
            assert _native.verify_status(air, prove()[0], pub, opts) == 0
            row = {"n": n, "width": w, "constraints": len(rep.actual), "eval_blowup": rep.eval_blowup,
                   "actual": rep.actual, "declared": rep.declared,
                   "constraint_degrees": timed(degrees, warmup, calls), "prove_device": timed(prove, warmup, calls)}
            row["degrees_over_proof_median"] = round(
                row["constraint_degrees"]["median_ms"] / row["prove_device"]["median_ms"], 3)
            row["constraint_degrees_kernels"] = kernel_rows(ctx, degrees)
            row["prove_device_kernels"] = kernel_rows(ctx, prove)
            return row
    finally:
        ctx.free(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constraint_degrees.json"))
    args = ap.parse_args()
    ctx = _native.Context(0)
    opts = ProofOptions(40, 8, 16)
    res = {"warmup": args.warmup, "calls": args.calls}
    try:
        n = 1 << 16
        builder = MimcProver(opts, ctx)
        tr = builder.build_trace(42 * 10**6, n)
        pub = [int(v) for v in builder.get_pub_inputs(tr).to_elements()]
        res["mimc_2^16"] = run(ctx, mimc_program(n, pub), tr.data, pub, opts, args.warmup, args.calls)
        print(json.dumps(res["mimc_2^16"]), flush=True)
        program, data, pub = cols16(1 << 14)
        res["cols16_degree3_2^14"] = run(ctx, program, data, pub, opts, args.warmup, args.calls)
        print(json.dumps(res["cols16_degree3_2^14"]), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
