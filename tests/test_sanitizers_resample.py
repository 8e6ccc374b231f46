"""AddressSanitizer + UBSan over the host-only half of the resampling ingest (host_resample.cpp alone): the driver
tests/sanitize/resample_san.cpp feeds fvad_resample_ratio / _out_frames / _window / _design and fvad_ingest_resample_tile seeded
random arguments and fvad_ingest_resample_check seeded random source tables and ratios with values near UINT64_MAX, and checks
that whatever is accepted lies inside its bytes, its file and its lanes and is given every frame its outputs read."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")


@pytest.fixture(scope="module")
def resample_san(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++ for the sanitizer build")
    out = tmp_path_factory.mktemp("san") / "resample_san"
    srcs = [os.path.join(CSRC, "host_resample.cpp"), os.path.join(ROOT, "tests", "sanitize", "resample_san.cpp")]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), *srcs, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_resample_host_functions_under_sanitizers(resample_san, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([resample_san, str(seed)], capture_output=True, text=True, env=env, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split("tables=")[1].split()[0]) == 4000 and int(r.stdout.split("designs=")[1].split()[0]) == 60
    assert int(r.stdout.split("rows=")[1].split()[0]) >= 200   # rows of accepted tables: the acceptance side is exercised
