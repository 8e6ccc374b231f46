"""The default design of the resampling ingest (fvad_resample_design): from the library's own f32 taps, in numpy
float64, per ratio -- the taps and the taps per phase, the pass-band ripple up to 0.40/m, the stop band from 0.60/m (m =
max(up, down), frequencies in cycles per sample of the up-times-oversampled input, the response normalised by up), the spread
of the phases' DC gains and the largest sum of |taps| of a phase; then the same for the outgoing ratios of the resampled clip
exports, whose prototypes have the ingest's shape at the mirrored ratio but other phases.  No device.
python tools/resample_response.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

RATES = (44100, 22050, 11025, 16000, 32000, 24000, 96000, 8000)
OUT_RATES = (44100, 32000, 22050, 11025, 16000)   # the outgoing ratios of the resampled clip exports: 147/160, 2/3, 147/320, 147/640, 1/3


def report(fv, rate, up, down):
    h = fv.resample_design(up, down).astype(np.float64)
    m = max(up, down)
    n = 1 << 22
    H = np.abs(np.fft.rfft(h, n)) / up
    f = np.fft.rfftfreq(n)
    pb, sb = H[f <= 0.40 / m], H[f >= 0.60 / m]
    dc = [h[r::up].sum() for r in range(up)]
    print(f"{rate:6d} Hz  {up:3d}/{down:<3d}  {h.size:5d} taps, {-(-h.size // up):3d} a phase   pass-band ripple {20 * np.log10(pb.max() / pb.min()):.3f} dB   "
          f"stop band {20 * np.log10(sb.max()):.1f} dB   phase DC spread {max(dc) - min(dc):.2e}   max sum|taps| of a phase {max(np.abs(h[r::up]).sum() for r in range(up)):.3f}")


def main():
    fv = load_package().binding
    print("the resampling ingest: files at these rates into 48 kHz lanes")
    for rate in RATES:
        report(fv, rate, *fv.resample_ratio(rate))
    print("the resampled clip exports (fvad_clips_export*_resampled, DESIGN 7.2): 48 kHz lanes out at these rates")
    for rate in OUT_RATES:
        report(fv, rate, *fv.resample_ratio(48000, rate))


if __name__ == "__main__":
    main()
