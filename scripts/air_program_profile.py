#!/usr/bin/env python3
"""Constraint evaluation of MiMC by the built-in kernel and by the program interpreter.

MiMC 2^20, blowup 8, 40 queries, grinding 21, the trace resident in HBM
(zkp_prove_device), once under the built-in id (k_eval_mimc) and once under the
same AIR registered as a constraint program (k_eval_program). Each gets warm-up
proofs and timed ones (whole-proof wall time), then a pass with the evaluation
kernel's launches bracketed by HIP events (Context.set_profiling). The two proofs
must be equal byte for byte. k_eval_mimc is the code of the commit before the
program path existed, unchanged, so its figure is that commit's.

Writes profiles/air_program.json (or --out).

    python scripts/air_program_profile.py [--log-n 20] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zk_stark_project_amd import AIR_MIMC, AirProgram, MimcProver, ProofOptions, _native  # noqa: E402

PROFILED = 5


def mimc_program(n, pub) -> AirProgram:
    p = AirProgram(1)
    K = p.periodic([(j + 1) * 10**6 for j in range(64)])
    p.constraint(p.next[0] - (p.cur[0] + K) ** 7, degree=7)
    p.assertion(0, 0, pub[0])
    p.assertion(0, n - 1, pub[1])
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_program.json"))
    args = ap.parse_args()

    n = 1 << args.log_n
    opts = ProofOptions(40, 8, 21)
    ctx = _native.Context(0)
    builder = MimcProver(opts, ctx)
    trace = builder.build_trace(42 * 10**6, n)
    pub = builder.get_pub_inputs(trace).to_elements()
    program = mimc_program(n, pub)
    compiled = program.compile()
    prog = program.register()
    d = ctx.alloc(trace.data.nbytes)
    rows, proofs = {}, {}
    try:
        ctx.to_device(d, trace.data)
        for name, air, kernel in (("builtin", AIR_MIMC, "eval_mimc"), ("program", prog, "eval_program")):
            def prove():
                return ctx.prove_device(air, d, 1, n, pub, opts)
            for _ in range(args.warmup):
                proofs[name], _ = prove()
            _native.verify(air, proofs[name], pub, opts)
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                prove()
                times.append((time.perf_counter() - t0) * 1e3)
            ctx.reset_stats()
            ctx.set_profiling(True, kernel)
            try:
                for _ in range(PROFILED):
                    prove()
                launches, ms = ctx.kernel_stats(kernel)
            finally:
                ctx.set_profiling(False)
                ctx.reset_stats()
            assert launches == PROFILED, (kernel, launches)
            rows[name] = {"kernel": kernel, "kernel_ms_per_proof": round(ms / PROFILED, 4),
                          "proof_median_ms": round(statistics.median(times), 4), "proof_min_ms": round(min(times), 4)}
            print(f"{name}: {json.dumps(rows[name])}", flush=True)
        assert proofs["builtin"] == proofs["program"], "the two ids' proofs differ"
    finally:
        ctx.free(d)
        prog.close()
        ctx.close()
    ratio = rows["program"]["kernel_ms_per_proof"] / rows["builtin"]["kernel_ms_per_proof"]
    out = {"workload": f"MiMC 2^{args.log_n}, blowup 8, 40 queries, grinding 21, trace resident (zkp_prove_device)",
           "steps": args.steps, "warmup": args.warmup, "profiled_proofs": PROFILED,
           "program": {"ops": len(compiled.ops), "registers": compiled.num_registers,
                       "lds_bytes_per_block": compiled.num_registers * 64 * 16},
           "proofs_equal": True, "builtin": rows["builtin"], "program_id": rows["program"],
           "eval_kernel_ratio_program_over_builtin": round(ratio, 3),
           "proof_ratio_program_over_builtin": round(rows["program"]["proof_median_ms"] /
                                                     rows["builtin"]["proof_median_ms"], 3)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
