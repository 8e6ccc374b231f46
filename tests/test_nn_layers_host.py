"""The yardstick of the NSNet2 layer tests, on the CPU: the oracle's layers judged one kernel at a time in the units of
nn_layer_cases.py (which yields the tolerances), the units' sanity on a model whose pre-activations are exact, and what each
mutation of the float64 model costs -- in its layer's units and in the end-to-end gains check's metric."""
import ctypes as C

import numpy as np
import pytest

import nn_layer_cases as N
import orc


@pytest.fixture(scope="module")
def oracle_table(weights7):
    """{(model, input index): (features, oracle layers)}"""
    return {(name, i): (f, N.oracle_layers(N.model(name, weights7), f)) for name in N.MODELS for i, f in enumerate(N.input_table())}


def test_oracle_layers_variant_is_the_oracle(weights7, oracle_table):
    # The gains of the layers variant are those of orc_nsnet2_forward bit for bit.  orc_nsnet2_forward calls the layers variant
    # (nothing between the two but NULL outputs), so this pins the wrapper and the copies out, not the arithmetic: no golden
    # of the oracle's bits is kept, because expf / tanhf are the host libm's.  What guards the arithmetic is the float64 model:
    # test_oracle_distances_are_the_constants fails if any layer of the oracle moves by a hundredth of a unit.
    # The one-step form is a second statement of every layer: it must restate each from the oracle's own previous-layer
    # outputs bit for bit.
    for (name, i), (feat, lay) in oracle_table.items():
        m = N.model(name, weights7)
        for s, f in enumerate(feat):
            assert np.array_equal(lay["gains"][s].view(np.uint32), orc.nsnet2_forward(m.w, f).view(np.uint32)), (name, i, s)
        n, T = feat.shape[:2]
        prev = lambda h: np.concatenate([np.zeros((n, 1, N.H), np.float32), h[:, :-1]], axis=1).reshape(n * T, N.H)  # noqa: E731
        flat = lambda a: a.reshape(n * T, -1)                                                                        # noqa: E731
        steps = {"h1": orc.nsnet2_layer_rows(m.w, "h1", flat(feat), prev(lay["h1"])),
                 "h2": orc.nsnet2_layer_rows(m.w, "h2", flat(lay["h1"]), prev(lay["h2"])),
                 "f2": orc.nsnet2_layer_rows(m.w, "f2", flat(lay["h2"])), "f3": orc.nsnet2_layer_rows(m.w, "f3", flat(lay["f2"])),
                 "gains": orc.nsnet2_layer_rows(m.w, "gains", flat(lay["f3"]))}
        for k in N.LAYERS:
            assert np.array_equal(steps[k].view(np.uint32), flat(lay[k]).view(np.uint32)), (name, i, k)


def test_oracle_distances_are_the_constants(weights7, oracle_table):
    worst = {k: 0.0 for k in N.ORACLE_UNITS}
    for (name, i), (feat, lay) in oracle_table.items():
        m = N.model(name, weights7)
        res = N.judge(m, feat, lay)
        res.update(N.judge(m, feat, dict(lay, h1=None)))            # the two GRU layers as one, as the pipelined kernels are judged
        print(f"oracle, {name:9s} T = {feat.shape[1]:2d}: " + "  ".join(f"{k} {res[k][0]:6.2f}" for k in N.ORACLE_UNITS))
        for k in worst:
            worst[k] = max(worst[k], res[k][0])
    print("oracle, worst: " + ", ".join(f'"{k}": {v:.3f}' for k, v in worst.items()))
    for k, v in worst.items():
        # the constant is the measured figure rounded up to two decimals: neither exceeded nor padded
        assert v <= N.ORACLE_UNITS[k] <= v + 0.011, (k, v, N.ORACLE_UNITS[k])
        # a healthy f32 evaluation costs a few units.  Hundreds would mean that the unit is wrong, not that the oracle is.
        assert N.ORACLE_UNITS[k] < 100 and N.TOL[k] == 4 * N.ORACLE_UNITS[k], k


def test_units_on_the_exact_selection_model(weights7, oracle_table):
    # select_varied: z = sigmoid(x - 100) = 0, R = 0, one exact product per pre-activation.  What is left is the nonlinearity's
    # own error -- expf / tanhf within an ulp, a reciprocal, three roundings of (1 - z) n + z h -- each at most eps on values
    # in [-1, 1]: a handful of units, whatever the input.  fc2 / fc3 copy one value (a 1.0 weight, a 0 bias): exact.
    m = N.model("select", weights7)
    for i, f in enumerate(N.input_table()):
        feat, lay = oracle_table[("select", i)]
        res = N.judge(m, feat, lay)
        print(f"oracle, select T = {feat.shape[1]:2d}: " + "  ".join(f"{k} {v[0]:.2f}" for k, v in res.items()))
        assert res["h1"][0] <= 8 and res["h2"][0] <= 8 and res["gains"][0] <= 8, res
        assert res["f2"][0] == 0 and res["f3"][0] == 0, res
        # and the network is not trivially dead there: the selected values reach the gains
        assert lay["h2"].std() > 0.05 and lay["gains"].std() > 0.01


@pytest.mark.parametrize("what", list(N.MUTATIONS))
def test_a_mutation_costs_more_than_fifty_tolerances(weights7, what):
    layer, mut, engine = N.MUTATIONS[what]
    m = N.model("synth", weights7)
    feat, skip = (N.chunked_features(6, 201), N.SKIP) if engine else (N.make_inputs(5, 54, 202), 0)
    good, bad = N.float64_cached(m, feat) if not skip else N.float64_layers(m, feat, None, skip), N.float64_layers(m, feat, mut, skip)
    res = N.judge(m, feat, bad, skip)
    clean = N.judge(m, feat, N.float64_layers(m, feat, None, skip), skip)
    e2e = N.gains_metric(bad["gains"], good["gains"])
    cost = res[layer][0] / N.TOL[layer]
    print(f"{what}: {layer} {res[layer][0]:.3g} units at {res[layer][1]} = {cost:.3g} x its tolerance of {N.TOL[layer]:.2f}; "
          f"end-to-end gains {e2e:.3g} relative (floor 1e-2), the existing check's bound is 1e-4: {'seen' if e2e > 1e-4 else 'NOT seen'}")
    assert max(v[0] for v in clean.values()) < 1e-3, clean     # the unmutated float64 model is its own reference
    assert cost > 50, (what, cost)
    if layer == "h1":
        # the default small-batch kernels keep no h1: there the same mutation is judged through "h12", whose unit carries the
        # propagated error of both layers and is therefore blunter.  Printed, and it must still fail the check; the bias case
        # reaches only 16 x that tolerance (measured), below the 50 x that holds where h1 exists.
        d12 = N.judge(m, feat, dict(bad, h1=None), skip)["h12"][0]
        print(f"{what}: judged as one with layer 2 (no h1: gru_ws2k / gru_ws2m): h12 {d12:.3g} units = {d12 / N.TOL['h12']:.3g} x its "
              f"tolerance of {N.TOL['h12']:.2f}")
        assert d12 > 10 * N.TOL["h12"], (what, d12)
    # ... and only the layer it touches pays: every other kernel is judged from the mutated outputs and finds them consistent
    assert all(v[0] < 1e-3 for k, v in res.items() if k != layer), res


def test_tap_argument_rules_without_a_context(fv):
    # the rules that need no device: no context, nothing else is looked at (the rest is in test_nn_layers_gpu.py)
    rows, width = C.c_size_t(7), C.c_size_t(7)
    buf = np.zeros(4, np.float32)
    assert fv.lib().fvad_ctx_nn_tap(None, 0, 0, 1, fv.fptr(buf), C.byref(rows), C.byref(width)) == fv.FVAD_ERR_INVALID_ARGUMENT
    assert rows.value == 7 and width.value == 7 and not buf.any()
    assert fv.lib().fvad_status_name(fv.FVAD_ERR_NOT_AVAILABLE) == b"NotAvailable"
