"""fvad_nsnet2_delay against the CPU oracle (no GPU, and not the library's own denoiser): with a model whose last layer is zero
and whose bias is +30 every gain is exactly 1.0f, so the oracle's NSNet2 is analysis, synthesis and the resamplers alone -- a
delay line with the sqrt-Hann reconstruction ripple on top.  The lag at which its output matches its input, searched over
0 .. 999, must be the delay the library states, and by a wide margin: 0.0018 at 482 against at least 0.515 anywhere else was
measured when the issue was written (a factor of 280); the tests ask for a factor of 50, which leaves room for another seed."""
import numpy as np
import pytest

import egress_mix_cases as mc
import orc

MARGIN = 50.0


def errors_by_lag(fv, rate, seed):
    r = rate // 16000
    den = orc.Denoiser(mc.unit_gain_weights(fv), sample_rate=rate)
    assert den.chunk == 8000 * r
    x = (np.random.default_rng(seed).standard_normal(3 * den.chunk) * 0.1).astype(np.float32)
    y = []
    for c in range(3):
        rc, out = den.denoise(x[c * den.chunk:(c + 1) * den.chunk])
        assert rc == 0
        assert np.all(den.gains()[4:] == np.float32(1.0))        # the chunk's 50 frames: sigmoid(30) is 1.0f
        y.append(out)
    y = np.concatenate(y)
    # the samples the up-sampler copies from the network's output (the others are interpolated between two of them)
    n = np.arange(2000, y.size)
    n = n[n % r == r - 1]
    return np.array([np.abs(y[n] - x[n - d]).max() for d in range(1000)])


@pytest.mark.parametrize("rate,seed", [(48000, 5), (48000, 6), (16000, 5)])
def test_the_oracles_output_lags_its_input_by_the_stated_delay(fv, rate, seed):
    D = fv.nsnet2_delay(rate)
    assert D == {48000: 482, 16000: 160}[rate] == 161 * (rate // 16000) - 1
    err = errors_by_lag(fv, rate, seed)
    others = np.delete(err, D)
    print(f"rate {rate}, seed {seed}: max|y[n] - x[n - d]| is {err[D]:.4g} at d = {D}, at least {others.min():.4g} elsewhere "
          f"(a factor of {others.min() / err[D]:.0f})")
    assert int(err.argmin()) == D
    assert err[D] * MARGIN <= others.min()
