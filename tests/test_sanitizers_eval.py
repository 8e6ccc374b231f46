"""AddressSanitizer + UBSan over the host scorer of a VAD batch (host_eval.cpp with host_vad.cpp and host_stats.cpp): the driver
tests/sanitize/eval_san.cpp runs host sweeps over random streams, scores them against random ragged label sets on one and
several threads, checks every machine against fvad_stats_from_segments bit for bit, and exercises the argument checks."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")


@pytest.fixture(scope="module")
def eval_san(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++ for the sanitizer build")
    out = tmp_path_factory.mktemp("san") / "eval_san"
    srcs = [os.path.join(CSRC, f) for f in ("host_vad.cpp", "host_stats.cpp", "host_eval.cpp")]
    srcs.append(os.path.join(ROOT, "tests", "sanitize", "eval_san.cpp"))
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), *srcs, "-o", str(out), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_scorer_under_sanitizers(eval_san, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([eval_san, str(seed)], capture_output=True, text=True, env=env, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split("machines=")[1]) == 30
