#!/usr/bin/env python3
"""Proof time, proof size and FRI kernel time over the four FRI folding factors.

MiMC 2^20, blowup 8, 40 queries, grinding 21, the trace resident in HBM
(zkp_prove_device). F = 16, 8 and 4 run with remainder degree 7; F = 2 with 15,
because degree 7 gives 17 layers at this size, one more than a proof may have.
Each configuration gets 5 warm-up proofs and 20 timed ones, then a pass with every
launch bracketed by HIP events for the per-kernel table. The proofs are checked by
the library's own verifier (zkp_verify).

Writes profiles/fri_folding_factors.json (or --out). `--parent FILE` merges a JSON
object with the parent commit's figures for F = 16 under the key "parent".

    python scripts/fri_folding_profile.py [--log-n 20] [--steps 20] [--warmup 5] [--factors 16,8,4,2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zk_stark_project_amd import AIR_MIMC, MimcProver, ProofOptions, _native  # noqa: E402

CONFIGS = [(16, 7), (8, 7), (4, 7), (2, 15)]  # (folding factor, remainder max degree)
KERNELS = ("merkle_fri", "fri_tail", "coin", "gather")
PROFILED = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--factors", default="16,8,4,2", help="folding factors to run (comma-separated)")
    ap.add_argument("--parent", default=None, help="JSON file with the parent commit's F = 16 figures")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_folding_factors.json"))
    args = ap.parse_args()

    n = 1 << args.log_n
    wanted = {int(f) for f in args.factors.split(",")}
    ctx = _native.Context(0)
    builder = MimcProver(ProofOptions(40, 8, 21), ctx)
    trace = builder.build_trace(42 * 10**6, n)
    pub = builder.get_pub_inputs(trace).to_elements()
    d = ctx.alloc(trace.data.nbytes)
    rows = {}
    try:
        ctx.to_device(d, trace.data)
        for fold, r in CONFIGS:
            if fold not in wanted:
                continue
            opts = ProofOptions(40, 8, 21, 1, fold, r)

            def prove():
                return ctx.prove_device(AIR_MIMC, d, 1, n, pub, opts)
            for _ in range(args.warmup):
                proof, tr = prove()
            _native.verify(AIR_MIMC, proof, pub, opts)
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                prove()
                times.append((time.perf_counter() - t0) * 1e3)
            ctx.reset_stats()
            ctx.set_profiling(True)
            try:
                for _ in range(PROFILED):
                    prove()
                table = ctx.stats_table()
            finally:
                ctx.set_profiling(False)
                ctx.reset_stats()
            names = (f"fri_fold{fold}",) + KERNELS
            rows[str(fold)] = {
                "remainder_max_degree": r,
                "fri_layers": tr.num_fri_layers,
                "proof_bytes": len(proof),
                "median_ms": round(statistics.median(times), 4),
                "min_ms": round(min(times), 4),
                "kernel_ms_per_proof": {k: round(table.get(k, {"ms": 0.0})["ms"] / PROFILED, 4) for k in names},
                "launches_per_proof": {k: table.get(k, {"launches": 0})["launches"] / PROFILED for k in names},
            }
            print(f"F={fold:2d} r={r:2d}: {json.dumps(rows[str(fold)])}", flush=True)
    finally:
        ctx.free(d)
        ctx.close()
    out = {"workload": f"MiMC 2^{args.log_n}, blowup 8, 40 queries, grinding 21, trace resident (zkp_prove_device)",
           "steps": args.steps, "warmup": args.warmup, "profiled_proofs": PROFILED, "factors": rows}
    if args.parent:
        with open(args.parent) as f:
            out["parent"] = json.load(f)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
