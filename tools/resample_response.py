"""The default design of the resampling ingest (fvad_resample_design): from the library's own f32 taps, in numpy
float64, per ratio -- the taps and the taps per phase, the pass-band ripple up to 0.40/m, the stop band from 0.60/m (m =
max(up, down), frequencies in cycles per sample of the up-times-oversampled input, the response normalised by up), the spread
of the phases' DC gains and the largest sum of |taps| of a phase.  No device.
python tools/resample_response.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

RATES = (44100, 22050, 11025, 16000, 32000, 24000, 96000, 8000)


def main():
    fv = load_package().binding
    for rate in RATES:
        up, down = fv.resample_ratio(rate)
        h = fv.resample_design(up, down).astype(np.float64)
        m = max(up, down)
        n = 1 << 22
        H = np.abs(np.fft.rfft(h, n)) / up
        f = np.fft.rfftfreq(n)
        pb, sb = H[f <= 0.40 / m], H[f >= 0.60 / m]
        dc = [h[r::up].sum() for r in range(up)]
        print(f"{rate:6d} Hz  {up:3d}/{down:<3d}  {h.size:5d} taps, {-(-h.size // up):2d} a phase   pass-band ripple {20 * np.log10(pb.max() / pb.min()):.3f} dB   "
              f"stop band {20 * np.log10(sb.max()):.1f} dB   phase DC spread {max(dc) - min(dc):.2e}   max sum|taps| of a phase {max(np.abs(h[r::up]).sum() for r in range(up)):.3f}")


if __name__ == "__main__":
    main()
