"""The context option vad_chain where no device is needed: simulator.run_sweep / run_grid refuse a bad value before any context
or device work, the CLI's --vad-chain, the accessor fvad_vad_batch_chain_form in the ctypes binding, and the option put on a
caller's context for the call only."""
import ctypes as C

import pytest

from test_vad_grid_devices_host import GRID, fake_ctx, write_plan


@pytest.fixture(scope="module")
def sim(pkg):
    return pkg.simulator


def test_run_grid_and_run_sweep_refuse_a_bad_vad_chain(pkg, sim, tmp_path, monkeypatch):
    plan = write_plan(pkg, tmp_path, [(1, "pcm16", 2.0)])
    monkeypatch.setattr(sim, "_make_ctx", lambda *a, **k: pytest.fail("a context was made"))
    with pytest.raises(ValueError, match="vad_chain"):
        sim.run_grid(plan, GRID, vad_chain="x")
    with pytest.raises(ValueError, match="vad_chain"):
        sim.run_sweep(plan, vad_chain="x")
    with pytest.raises(ValueError, match="vad_chain"):
        sim.run_grid(plan, GRID, vad_chain="x", ctx=[fake_ctx(pkg.binding)])


def test_cli_parses_vad_chain(sim):
    ap = sim.arg_parser()
    assert ap.parse_args(["-i", "p.json", "--sweep"]).vad_chain is None
    for v in sim.VAD_CHAINS:
        assert ap.parse_args(["-i", "p.json", "--sweep-grid", "g.json", "--vad-chain", v]).vad_chain == v
    with pytest.raises(SystemExit):
        ap.parse_args(["-i", "p.json", "--sweep", "--vad-chain", "x"])


def test_auto_threshold_per_form(sim):
    """the lane form's threshold stays; the cooperative form's is its own constant"""
    assert sim.SWEEP_DEVICE_MIN_CONFIGS == 256
    assert sim._auto_vad_on(255, None) == sim._auto_vad_on(255, "lane") == "host"
    assert sim._auto_vad_on(256, "lane") == "device"
    n = sim.SWEEP_DEVICE_MIN_CONFIGS_COOP
    assert sim._auto_vad_on(n, "coop") == "device" and sim._auto_vad_on(n - 1, "coop") == "host"


def test_ctypes_exposes_chain_form(fv):
    f = fv.lib().fvad_vad_batch_chain_form
    assert f.restype is C.c_int and len(f.argtypes) == 2
    sw = fv.VadSweep(1, [{}])
    try:
        assert sw.chain_form() == 0   # no device launch yet
        form = C.c_int(7)
        assert f(None, C.byref(form)) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert f(sw.h, None) == fv.FVAD_ERR_INVALID_ARGUMENT
    finally:
        sw.close()


def test_option_is_put_back_on_a_callers_context(fv, sim):
    """_VadChain: set for the call, then back to what the caller had set (a context the call made is left alone: it is closed)"""
    calls = []
    ctx = fake_ctx(fv)
    ctx.set_option = lambda name, value=None: calls.append((name, value))
    ctx.option_set = lambda name: "coop"
    ch = sim._VadChain("lane")
    ch.apply(ctx, owned=False)
    ch.close()
    assert calls == [("vad_chain", "lane"), ("vad_chain", "coop")]
    calls.clear()
    ch = sim._VadChain("coop")
    ch.apply(ctx, owned=True)
    ch.close()
    assert calls == [("vad_chain", "coop")]
    calls.clear()
    ch = sim._VadChain(None)
    ch.apply(ctx, owned=False)
    ch.close()
    assert calls == []
