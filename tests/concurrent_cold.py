"""The child process of test_gpu_concurrent_contexts.py::test_cold_start_in_a_fresh_process
(not a test module): four threads each create a context, and each context's first call is a
different MiMC proof with logn >= 11, so the first NTT launches of the process run at once.
Proof i is written to <out_dir>/proof_<i>.bin; the parent compares it with the oracle's bytes.
`--sequential` runs the same four proofs one after another (the measurement the parent's
time limit is sized from).

Usage: python tests/concurrent_cold.py <out_dir> [--sequential]"""
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

COLD_PROOFS = [(1 << 11, 8), (1 << 11, 16), (1 << 12, 8), (1 << 12, 16)]  # (n, blowup): logn >= 11 each
BARRIER_TIMEOUT = 60.0  # the inputs are built before the threads start: they meet within milliseconds


def main(out_dir, sequential=False):
    from folding_cases import options
    from test_gpu_options import mimc_inputs
    from zk_stark_project_amd import AIR_MIMC, _native

    _native.load()
    inputs = [(mimc_inputs(n), options(20, blowup, 4)) for n, blowup in COLD_PROOFS]  # built before any thread starts
    barrier = threading.Barrier(len(inputs))
    errors = []

    def prove(i):
        (_, trace, pub), opts = inputs[i]
        ctx = None
        try:
            if not sequential:
                barrier.wait(BARRIER_TIMEOUT)
            ctx = _native.Context(0)
            proof, _ = ctx.prove(AIR_MIMC, trace.data, pub, opts)
            with open(os.path.join(out_dir, f"proof_{i}.bin"), "wb") as f:
                f.write(proof)
        except BaseException as e:  # noqa: BLE001 — reported by the exit status
            errors.append(f"thread {i}: {type(e).__name__}: {e}")
            barrier.abort()
        finally:
            if ctx is not None:
                ctx.close()

    if sequential:
        for i in range(len(inputs)):
            prove(i)
    else:
        threads = [threading.Thread(target=prove, args=(i,)) for i in range(len(inputs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    for e in errors:
        print(e, file=sys.stderr)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], "--sequential" in sys.argv[2:]))
