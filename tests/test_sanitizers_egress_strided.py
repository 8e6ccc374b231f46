"""AddressSanitizer + UBSan over the host-only half of the strided resampling egress (host_egress_strided.cpp with
host_egress_resample.cpp and host_resample.cpp): the stand-alone driver tests/sanitize/egress_strided_san.cpp feeds
fvad_egress_resample_strided_check seeded random row tables with random steps and values near UINT64_MAX, and checks that
whatever is accepted lies inside its lanes -- counted `step` apart, without wrapping -- and inside its output bytes and is given
the window it reads.  No Python code runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")


@pytest.fixture(scope="module")
def egress_strided_san(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++ for the sanitizer build")
    out = tmp_path_factory.mktemp("san") / "egress_strided_san"
    srcs = [os.path.join(CSRC, "host_egress_strided.cpp"), os.path.join(CSRC, "host_egress_resample.cpp"), os.path.join(CSRC, "host_resample.cpp"),
            os.path.join(ROOT, "tests", "sanitize", "egress_strided_san.cpp")]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), *srcs, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_strided_check_under_sanitizers(egress_strided_san, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([egress_strided_san, str(seed)], capture_output=True, text=True, env=env, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split("tables=")[1].split()[0]) == 6000 and int(r.stdout.split("step1=")[1].split()[0]) > 0
