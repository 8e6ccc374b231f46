"""Sweeps in time slices, without a GPU: run_grid's slice-size check, the mapped WAV reader (binding.wav_map) against
fvad_wav_read / fvad_wav_read_i16, and the device-part entry points where there is no device."""
import json
import struct

import numpy as np
import pytest

from test_harness import write_wav

CHUNK = 24000


@pytest.fixture(scope="module")
def sim(pkg):
    return pkg.simulator


@pytest.mark.parametrize("fft_size,bad,good", [(1024, [0, -16, 8, 17, 24, 16.0, True], [16, 48, 1024]),
                                               (2048, [0, -32, 16, 48], [32, 64]),
                                               (1000, [0, -1], [1, 3])])
def test_slice_chunks_check(sim, fft_size, bad, good):
    assert sim.slice_align(fft_size) == np.lcm(CHUNK, fft_size) // CHUNK
    for n in bad:
        with pytest.raises(ValueError):
            sim.check_slice_chunks(n, fft_size)
    for n in good:
        sim.check_slice_chunks(n, fft_size)


def test_run_grid_refuses_a_bad_slice_before_any_gpu_work(fv, sim, tmp_path):
    pcm = np.zeros((1, 3 * CHUNK), np.float32)
    fv.wav_write(str(tmp_path / "a.wav"), pcm)
    (tmp_path / "a.txt").write_text("0.5\t1.0\tspeech\n")
    for fft_size, n in ((1024, 0), (1024, -16), (1024, 24), (2048, 16)):
        plan = {"instances": [{"name": "a", "audio_path": "a.wav", "ref_path": "a.txt"}],
                "config": {"vad_config": {"fft_size": fft_size}}}
        (tmp_path / "plan.json").write_text(json.dumps(plan))
        with pytest.raises(ValueError, match="slice_chunks"):   # (a context is never made: no device is needed)
            sim.run_grid(str(tmp_path / "plan.json"), {"axes": {"speech_threshold_factor": [3.0, 5.0]}}, slice_chunks=n, out=None)


def _as_planar(mapped):
    return np.ascontiguousarray(np.asarray(mapped).T)


@pytest.mark.parametrize("nch,n,fmt,extensible", [(1, 1001, "f32", False), (2, 777, "f32", False), (1, 999, "pcm16", False),
                                                  (2, 1235, "pcm16", False), (3, 501, "f32", True), (2, 333, "pcm16", True)])
def test_wav_map_equals_the_readers(fv, tmp_path, nch, n, fmt, extensible):
    rng = np.random.default_rng(n)
    pcm = rng.uniform(-0.9, 0.9, (nch, n)).astype(np.float32)
    path = str(tmp_path / "x.wav")
    write_wav(path, pcm, fmt=fmt, extensible=extensible)   # (a LIST chunk of odd size before the data chunk)
    mapped, sr = fv.wav_map(path)
    assert sr == 48000 and mapped.shape == (n, nch)
    want, _ = fv.wav_read(path)
    if fmt == "pcm16":
        assert mapped.dtype == np.int16
        want16, _ = fv.wav_read_i16(path)
        assert np.array_equal(_as_planar(mapped), want16)
        assert np.array_equal((_as_planar(mapped) * np.float32(1.0 / 32768.0)).astype(np.float32), want)
    else:
        assert mapped.dtype == np.float32
        assert np.array_equal(_as_planar(mapped).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("pcm16", [False, True])
def test_wav_map_on_library_written_files(fv, tmp_path, pcm16):
    rng = np.random.default_rng(5)
    for nch, n in ((1, 4097), (2, 48001)):
        pcm = rng.uniform(-0.9, 0.9, (nch, n)).astype(np.float32)
        path = str(tmp_path / f"w{nch}.wav")
        fv.wav_write(path, pcm, pcm16=pcm16)
        mapped, sr = fv.wav_map(path)
        want, sr2 = fv.wav_read(path)
        assert sr == sr2 == 48000 and mapped.shape == (n, nch)
        if pcm16:
            assert np.array_equal(_as_planar(mapped), fv.wav_read_i16(path)[0])
        else:
            assert np.array_equal(_as_planar(mapped), want)


def test_wav_map_edge_cases(fv, tmp_path):
    def riff(chunks):
        return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks

    fmt16 = b"fmt " + struct.pack("<IHHIIHH", 16, 1, 2, 48000, 48000 * 4, 4, 16)
    data = np.arange(-10, 10, dtype="<i2").tobytes()              # 10 stereo frames
    # a data length past the end of the file is cut to the file (fvad_wav_read tolerates a streaming length); a partial
    # frame at the end is dropped
    p = tmp_path / "long.wav"
    p.write_bytes(riff(fmt16 + b"data" + struct.pack("<I", 1 << 30) + data + b"\x01"))
    mapped, _ = fv.wav_map(str(p))
    assert mapped.shape == (10, 2) and np.array_equal(_as_planar(mapped), fv.wav_read_i16(str(p))[0])
    # an empty data chunk
    p = tmp_path / "empty.wav"
    p.write_bytes(riff(fmt16 + b"data" + struct.pack("<I", 0)))
    mapped, _ = fv.wav_map(str(p))
    assert mapped.shape == (0, 2) and fv.wav_read(str(p))[0].shape == (2, 0)
    # what the library refuses, wav_map refuses: 24-bit PCM, no fmt before data, not RIFF, no data chunk
    bad = {"pcm24": riff(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, 48000, 48000 * 3, 3, 24) + b"data" + struct.pack("<I", 6) + b"\0" * 6),
           "nofmt": riff(b"data" + struct.pack("<I", len(data)) + data + fmt16),
           "notriff": b"RIFX" + riff(fmt16)[4:],
           "nodata": riff(fmt16)}
    for name, blob in bad.items():
        p = tmp_path / f"{name}.wav"
        p.write_bytes(blob)
        with pytest.raises(fv.FvadError):
            fv.wav_read(str(p))
        with pytest.raises(fv.FvadError):
            fv.wav_map(str(p))


def test_device_part_entry_points_without_a_device(fv):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    sw = fv.VadSweep(2, [{}, {"speech_threshold_factor": 3.0}])
    try:
        nf = (fv.sz * 2)(0, 0)
        rms = np.zeros((2, 1), np.float32)
        lib = fv.lib()
        assert lib.fvad_vad_batch_run_device_part(None, sw.h, None, 1, nf, fv.fptr(rms), 1, nf, CHUNK, 0) == fv.FVAD_ERR_NO_DEVICE
        assert lib.fvad_vad_batch_run_device_part(None, sw.h, None, 1, nf, fv.fptr(rms), 1, nf, CHUNK, 375) == fv.FVAD_ERR_NO_DEVICE
        assert lib.fvad_vad_batch_score_device(None, sw.h) == fv.FVAD_ERR_NO_DEVICE
        assert sw.device_bytes() == 0 and lib.fvad_vad_batch_device_bytes(None) == 0
        # the host parts are unaffected
        band = np.zeros((1, 2, 375), np.float32)
        r = np.zeros((2, 16), np.float32)
        assert lib.fvad_vad_batch_run_part(sw.h, fv.fptr(band), 375, 375, fv.fptr(r), 16, 16, CHUNK, 0, 1) == 0
        assert sw.device_bytes() == 0
    finally:
        sw.close()
