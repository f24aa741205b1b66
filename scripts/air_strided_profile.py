#!/usr/bin/env python3
"""What strided assertions cost in a proof.

MiMC 2^20, blowup 8, 40 queries, grinding 21, the trace resident in HBM
(zkp_prove_device), under three registered programs:
  singles: the seed and the result as two single assertions (k_eval_program, the
           launch of a program without strided assertions);
  strided: the seed a single, the result a sequence of one value over the stride
           2^20, and a periodic assertion of stride 64 on top (k_eval_program_strided,
           k_strided_combine and the coset NTT of W). No row of a MiMC cycle holds one
           value in every cycle, so the periodic assertion states the first cycle's
           row 62 and the trace fails it: the kernels' times do not depend on that,
           but the proof does not verify and, at blowup 8 = ce, is made a second time
           without the derived last column (launches_per_proof = 2), so its whole-proof
           time is not a valid proof's;
  strided_valid: the same with row 62 of every cycle asserted by a sequence of 2^14
           values instead: a valid proof, and a second group that holds a sequence.
Each gets warm-up proofs and timed ones (whole-proof wall time), then one pass per
kernel with that kernel's launches bracketed by HIP events (Context.set_profiling).
--singles-only times the first program alone: the run to repeat on the commit before
this one, whose library has no zkp_air_register_strided.

Writes profiles/air_strided.json (or --out).

    python scripts/air_strided_profile.py [--log-n 20] [--steps 20] [--warmup 5] [--singles-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zk_stark_project_amd import AirProgram, MimcProver, ProofOptions, _native  # noqa: E402

PROFILED = 5


def mimc_program(n, pub, kind, row62) -> AirProgram:
    p = AirProgram(1)
    K = p.periodic([(j + 1) * 10**6 for j in range(64)])
    p.constraint(p.next[0] - (p.cur[0] + K) ** 7, degree=7)
    p.assertion(0, 0, pub[0])
    if kind == "singles":
        p.assertion(0, n - 1, pub[1])
        return p
    p.sequence_assertion(0, n - 1, n, [pub[1]])
    if kind == "strided":
        p.periodic_assertion(0, 62, 64, row62[0])
    else:
        p.sequence_assertion(0, 62, 64, row62)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--singles-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_strided.json"))
    args = ap.parse_args()

    n = 1 << args.log_n
    opts = ProofOptions(40, 8, 21)
    ctx = _native.Context(0)
    builder = MimcProver(opts, ctx)
    trace = builder.build_trace(42 * 10**6, n)
    pub = list(builder.get_pub_inputs(trace).to_elements())
    row62 = [int(lo) | (int(hi) << 64) for lo, hi in trace.data[0, 62::64]]
    cases = [("singles", ["eval_program", "ntt_dit"])]  # ntt_dit: every coset NTT of the proof, W's among them
    if not args.singles_only:
        new = ["eval_program_strided", "strided_combine", "ntt_dit"]
        cases += [("strided", new), ("strided_valid", new)]
    d = ctx.alloc(trace.data.nbytes)
    rows = {}
    try:
        ctx.to_device(d, trace.data)
        for name, kernels in cases:
            prog = mimc_program(n, pub, name, row62).register()
            try:
                def prove():
                    return ctx.prove_device(prog, d, 1, n, pub, opts)
                t0 = time.perf_counter()
                proof, _ = prove()
                first_ms = (time.perf_counter() - t0) * 1e3  # builds the tables and the image
                for _ in range(args.warmup):
                    proof, _ = prove()
                times = []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    prove()
                    times.append((time.perf_counter() - t0) * 1e3)
                row = {"verifies": _native.verify_status(prog, proof, pub, opts) == 0,
                       "first_proof_ms": round(first_ms, 4), "proof_median_ms": round(statistics.median(times), 4),
                       "proof_min_ms": round(min(times), 4), "kernels_ms_per_proof": {},
                       "launches_per_proof": {}}
                for kernel in kernels:
                    ctx.reset_stats()
                    ctx.set_profiling(True, kernel)
                    try:
                        for _ in range(PROFILED):
                            prove()
                        launches, ms = ctx.kernel_stats(kernel)
                    finally:
                        ctx.set_profiling(False)
                        ctx.reset_stats()
                    row["kernels_ms_per_proof"][kernel] = round(ms / PROFILED, 4)
                    row["launches_per_proof"][kernel] = launches / PROFILED
                rows[name] = row
                print(f"{name}: {json.dumps(row)}", flush=True)
            finally:
                prog.close()
    finally:
        ctx.free(d)
        ctx.close()
    out = {"workload": f"MiMC 2^{args.log_n}, blowup 8, 40 queries, grinding 21, trace resident (zkp_prove_device)",
           "steps": args.steps, "warmup": args.warmup, "profiled_proofs": PROFILED, **rows}
    if "strided_valid" in rows:
        s, b = rows["strided_valid"], rows["singles"]
        out["eval_kernel_ratio_strided_valid_over_singles"] = round(
            s["kernels_ms_per_proof"]["eval_program_strided"] / b["kernels_ms_per_proof"]["eval_program"], 3)
        out["proof_ratio_strided_valid_over_singles"] = round(s["proof_median_ms"] / b["proof_median_ms"], 3)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
