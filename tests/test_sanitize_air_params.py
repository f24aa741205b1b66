"""CPU: the host code of programs with public inputs under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/sanitize_air_params.cpp):
zkp_air_register_params' binding and validation code, zkp_air_check_trace_pub, and zkp_verify
under ids with public inputs on an oracle-made MiMC proof and bit flips of it. Host build
only; any sanitizer report aborts the binary."""
import os
import subprocess

from test_air_program import oracle_case
from test_sanitizers import CSRC, ROOT, SAN, write_case
from zk_stark_project_amd.field import to_bytes


def test_air_params_host_code_under_asan_ubsan(tmp_path):
    host = []
    for f in SAN:  # host-only sanitizers on the hipcc line
        host += ["-Xarch_host", f] if f.startswith("-fsanitize") or f.startswith("-fno-sanitize") else [f]
    exe = str(tmp_path / "sanitize_air_params")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", *host,
                           "-fno-gpu-sanitize", os.path.join(CSRC, "verifier.cpp"),
                           os.path.join(ROOT, "tests", "native", "sanitize_air_params.cpp"),
                           "-Xarch_host", "-fsanitize=address,undefined", "-o", exe])
    air, proof, pub, opts, n = oracle_case("mimc64")
    d = str(tmp_path / "mimc64")
    write_case(d, air, proof, to_bytes(pub), opts)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, d], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "checked 918 verifications, 0 failures" in r.stdout, r.stdout
