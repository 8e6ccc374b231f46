"""AddressSanitizer + UBSan over the host-only half of the two-source egress (host_egress_mix.cpp): the stand-alone driver
tests/sanitize/egress_mix_san.cpp feeds fvad_nsnet2_delay seeded random rates and fvad_egress_mix_check seeded random row
tables and weights (zeros, NaN, infinities, values near UINT64_MAX), and checks that whatever is accepted lies inside the lanes
it reads and its output bytes.  A program of its own, built on the CPU from that one source file: nothing loaded into Python
runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")


@pytest.fixture(scope="module")
def egress_mix_san(tmp_path_factory):
    # g++, else the library's own host compiler (csrc/Makefile's HOSTCXX); without either the test fails: it never skips
    hostcxx = os.environ.get("HOSTCXX", "/opt/rocm/lib/llvm/bin/clang++")
    cxx = shutil.which("g++") or shutil.which(hostcxx) or shutil.which("clang++")
    assert cxx, f"no compiler for the sanitizer build: neither g++ nor {hostcxx}"
    out = tmp_path_factory.mktemp("san") / "egress_mix_san"
    srcs = [os.path.join(CSRC, "host_egress_mix.cpp"), os.path.join(ROOT, "tests", "sanitize", "egress_mix_san.cpp")]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), *srcs, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_delay_and_check_under_sanitizers(egress_mix_san, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([egress_mix_san, str(seed)], capture_output=True, text=True, env=env, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split("delays=")[1].split()[0]) == 2000 and int(r.stdout.split("tables=")[1].split()[0]) == 4000
