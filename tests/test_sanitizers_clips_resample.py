"""AddressSanitizer + UBSan over fvad_clips_resample_check, fvad_clips_resample_tile and fvad_clips_plan_resampled
(host_clips_resample.cpp with host_resample.cpp, host only): the stand-alone driver tests/sanitize/clips_resample_san.cpp feeds
them seeded ratios, tap counts and tap tables with NaN and the infinities among them and clip lengths up to UINT64_MAX, and holds
every answer against the rules restated in 128 bits.  The driver is a plain process of its own; nothing loaded into Python is
sanitised."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")


@pytest.fixture(scope="module")
def clips_resample_san(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++ for the sanitizer build")
    out = tmp_path_factory.mktemp("san") / "clips_resample_san"
    srcs = [os.path.join(CSRC, "host_clips_resample.cpp"), os.path.join(CSRC, "host_resample.cpp"),
            os.path.join(ROOT, "tests", "sanitize", "clips_resample_san.cpp")]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), *srcs, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_check_tile_and_plan_under_sanitizers(clips_resample_san, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([clips_resample_san, str(seed)], capture_output=True, text=True, env=env, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split("rounds=")[1].split()[0]) == 4000
