"""AddressSanitizer + UBSan over fvad_clips_split_mel_check and fvad_clips_split_fbank_check (host_clips_features.cpp, host only):
the stand-alone driver tests/sanitize/clips_feat_split_san.cpp feeds them seeded random split rows, buffers and frame parameters
with values near UINT64_MAX, and checks with 128-bit arithmetic that whatever is accepted has every piece inside its buffer and
the output beside both sources, that the numbers are the family's plan's for a_len + b_len, and that a refusal's status follows
the stated order.  The driver is a plain process of its own, built from the host file alone; nothing loaded into Python is
sanitised."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "formula-vad_amd", "csrc")


@pytest.fixture(scope="module")
def clips_feat_split_san(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++ for the sanitizer build")
    out = tmp_path_factory.mktemp("san") / "clips_feat_split_san"
    srcs = [os.path.join(CSRC, "host_clips_features.cpp"), os.path.join(ROOT, "tests", "sanitize", "clips_feat_split_san.cpp")]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), *srcs, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_split_feature_checks_under_sanitizers(clips_feat_split_san, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([clips_feat_split_san, str(seed)], capture_output=True, text=True, env=env, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split("tables=")[1].split()[0]) == 4000
