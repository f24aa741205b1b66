"""The TrainingUpdate traces of a round built in one call, at the reference flow's shape
(bs = 50: n = 8192, w = 240, 8 clients), against one call per client, in one run on one
machine, the variants alternating:

  * 8 single build_trace_device() calls (numpy's mask draw, an upload and a chain each);
  * one build_traces_device() with numpy's masks sent through the batch call;
  * one build_traces_device() with the masks made on the device (median and min);
  * the per-kernel device ms of the statistics table for each of the three;
  * 8 traces built and proved, one call per client and batched;
  * the CLI's "Step 'proof' completed in" for --bs 50 over 8 devices.

Writes profiles/tu_batch_build.json (--out to change) with the figures recorded before
the batch call existed (profiles/tu_trace_build.json) beside the new ones. The one gate:
the device-mask batch is faster than the 8 single calls of the same run, and its traces
have the single calls' bytes."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from tu_trace_probe import BS, CLIENTS, cli_proof_step_ms, make_provers, ms_since, write_dataset  # noqa: E402

REPS = 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tu_batch_build.json"))
    args = ap.parse_args()
    from zk_stark_project_amd import AIR_TRAINING_UPDATE, _native
    from zk_stark_project_amd.prover import TrainingUpdateProver

    ctx = _native.Context(0)
    opts, provers = make_provers(CLIENTS, ctx)
    n = provers[0].trace_length
    stride = 240 * n * 16
    d = ctx.alloc(CLIENTS * stride)
    ptrs = [d + k * stride for k in range(CLIENTS)]
    out = {"shape": {"bs": BS, "n": n, "width": 240, "clients": CLIENTS}}

    variants = {
        "eight_single_calls": lambda: [p.build_trace_device(ctx, ptr) for p, ptr in zip(provers, ptrs)],
        "batch_host_masks": lambda: TrainingUpdateProver.build_traces_device(provers, ctx, d, device_masks=False),
        "batch_device_masks": lambda: TrainingUpdateProver.build_traces_device(provers, ctx, d),
    }

    # the same bytes from every variant
    traces = {}
    for name, fn in variants.items():
        fn()
        traces[name] = np.empty((CLIENTS, 240, n, 2), dtype=np.uint64)
        ctx.to_host(traces[name], d)
        ctx.to_device(d, np.zeros(CLIENTS * stride // 8, dtype=np.uint64))
    out["batch_traces_equal_single"] = bool(
        np.array_equal(traces["eight_single_calls"], traces["batch_host_masks"])
        and np.array_equal(traces["eight_single_calls"], traces["batch_device_masks"]))
    del traces

    # wall ms around calls that end in a synchronise; warm, the variants alternating
    times = {name: [] for name in variants}
    for rep in range(REPS + 3):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            if rep >= 3:
                times[name].append(ms_since(t0))
    out["eight_traces_build_ms"] = {name: {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                           "repeats": len(v)} for name, v in times.items()}

    # per-kernel device ms per build of 8, profiling on, in loops of their own
    out["kernels_ms_per_eight_traces"] = {}
    for name, fn in variants.items():
        ctx.reset_stats()
        ctx.set_profiling(True)
        for _ in range(10):
            fn()
        ctx.set_profiling(False)
        table = ctx.stats_table()
        out["kernels_ms_per_eight_traces"][name] = {
            k: {"ms": round(table[k]["ms"] / 10, 4), "launches": table[k]["launches"] // 10}
            for k in ("tu_states", "tu_trace") if k in table}
    ctx.reset_stats()

    # built and proved
    def single_and_prove():
        for p in provers:
            p.build_trace_device(ctx, d)
            ctx.prove_device(AIR_TRAINING_UPDATE, d, 240, n, p.get_pub_inputs().to_elements(), opts)

    def batch_and_prove():
        for p, ptr in zip(provers, TrainingUpdateProver.build_traces_device(provers, ctx, d)):
            ctx.prove_device(AIR_TRAINING_UPDATE, ptr, 240, n, p.get_pub_inputs().to_elements(), opts)

    both = {"one_call_per_client": single_and_prove, "batched": batch_and_prove}
    bp = {name: [] for name in both}
    for rep in range(7):
        for name, fn in both.items():
            t0 = time.perf_counter()
            fn()
            if rep >= 2:
                bp[name].append(ms_since(t0))
    out["eight_traces_build_and_prove_ms"] = {name: round(statistics.median(v), 2) for name, v in bp.items()}
    ctx.free(d)
    ctx.close()

    with tempfile.TemporaryDirectory() as data_dir:
        write_dataset(data_dir)
        runs = [cli_proof_step_ms(data_dir) for _ in range(4)]
    out["cli_proof_step_ms"] = {"runs": runs, "warm": min(runs[1:])}

    with open(os.path.join(ROOT, "profiles", "tu_trace_build.json")) as f:
        before = json.load(f)
    out["recorded_before_the_batch_call"] = {
        "eight_traces_build_ms": before["eight_traces_ms"]["build_median"],
        "eight_traces_build_and_prove_ms": before["eight_traces_ms"]["build_and_prove_median"],
        "cli_proof_step_ms": before["cli_proof_step_ms"]["device_traces_warm"]}
    single_ms = out["eight_traces_build_ms"]["eight_single_calls"]["median"]
    batch_ms = out["eight_traces_build_ms"]["batch_device_masks"]["median"]
    out["gate_batch_faster_than_single_calls"] = bool(batch_ms < single_ms)
    out["speedup"] = round(single_ms / batch_ms, 2)
    txt = json.dumps(out, indent=1)
    print(txt)
    with open(args.out, "w") as f:
        f.write(txt + "\n")
    if not (out["gate_batch_faster_than_single_calls"] and out["batch_traces_equal_single"]):
        raise SystemExit("gate failed: the batch must have the single calls' bytes and be faster")


if __name__ == "__main__":
    main()
