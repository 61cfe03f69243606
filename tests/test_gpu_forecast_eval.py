"""GPU: forecast_eval of the cycle driver (vaevar.cycle.CyclicDA): forecasts started at each analysis, scored
against the truth at every lead by Metrics.verify. The tiny decoder and forecast setup of test_gpu_cycle.py, 2 cycles,
forecast_steps = 3."""
import datetime as dt
import os

import numpy as np
import pytest
import torch

from conftest import check_bitwise
from test_gpu_cycle import T0, _setup, _truth

pytestmark = pytest.mark.gpu

H6 = dt.timedelta(hours=6)
K = 3
FILES = ("xb", "bg_wrmse", "ana_wrmse", "bg_bias", "ana_bias", "bg_mse", "ana_mse", "error_obs")


@pytest.fixture(scope="module")
def nets():
    from vaevar import config as C
    from vaevar.engine import LGUnet

    return LGUnet(C.TINY, 1, 1).load_synthetic(), LGUnet(C.TINY_FLOW, 1, 1).load_synthetic()


def _run(nets, out_dir, name, end, truth=_truth, obs=None, **kw):
    from vaevar.cycle import CyclicVAE4DVar, SyntheticObs

    H, R, xb0 = _setup()
    dec, fc = nets
    obs = obs or SyntheticObs(truth, H, R)
    cyc = CyclicVAE4DVar(dec, fc, obs, T0, end, Nit=1, name=name, out_dir=str(out_dir), xb0=xb0, **kw)
    xas = []
    cyc.run_assimilation(log=lambda t, res: xas.append(res["xa"].clone()))
    return cyc, xas


@pytest.fixture(scope="module")
def runs(nets, tmp_path_factory):
    """The same two cycles without and with forecast_eval, the integrate calls of the second counted."""
    import vaevar.cycle as vc

    d = tmp_path_factory.mktemp("fe")
    off, xas_off = _run(nets, d, "off", T0 + 2 * H6)
    calls, real = [], vc.integrate

    def counting(model, x, mean, std, steps=1, out=None):
        calls.append(steps)
        return real(model, x, mean, std, steps, out)

    vc.integrate = counting
    try:
        on, xas_on = _run(nets, d, "on", T0 + 2 * H6, forecast_eval=True, forecast_steps=K)
    finally:
        vc.integrate = real
    return {"dir": str(d), "off": off, "on": on, "xas_off": xas_off, "xas_on": xas_on, "calls": calls}


def test_analysis_and_metric_files_unchanged(runs):
    for k in range(2):
        check_bitwise(f"forecast_eval cycle {k} xa", runs["xas_on"][k], runs["xas_off"][k])
    check_bitwise("forecast_eval final xb", runs["on"].xb, runs["off"].xb)
    for f in FILES:
        a = np.load(os.path.join(runs["dir"], "on", f + ".npy"))
        b = np.load(os.path.join(runs["dir"], "off", f + ".npy"))
        assert a.shape == b.shape, f
        check_bitwise(f"forecast_eval {f}.npy", a, b)
    assert not [f for f in os.listdir(os.path.join(runs["dir"], "off")) if f.startswith("forecast_")]


def test_forecast_wrmse_equals_hand_composition(runs, nets):
    from vaevar.engine import integrate

    cyc = runs["on"]
    got = np.load(os.path.join(runs["dir"], "on", "forecast_wrmse.npy"))
    assert got.shape == (2, K, 4) and got.dtype == np.float64 and np.isfinite(got).all() and (got > 0).all()
    assert [f for f in os.listdir(os.path.join(runs["dir"], "on")) if f.startswith("forecast_")] == \
        ["forecast_wrmse.npy"]
    want = np.empty_like(got)
    for c in range(2):
        x = runs["xas_on"][c]
        for k in range(1, K + 1):
            x = integrate(nets[1], x, cyc.mean_d, cyc.std_d, 1)
            gt = torch.from_numpy(_truth(T0 + c * H6 + k * H6)).cuda()
            want[c, k - 1] = cyc.metric.verify(x, gt)["WRMSE"].cpu().numpy()
    check_bitwise("forecast_wrmse.npy vs integrate + Metrics.verify by hand", got, want)


def test_a_cycle_costs_exactly_K_forecast_steps(runs):
    assert runs["calls"] == [1] * (2 * K)


class _WindowedTruth:
    """SyntheticObs whose truth is missing from `lead` cycle times after the analysis time on."""

    def __init__(self, H, R, lead, exc):
        from vaevar.cycle import SyntheticObs

        self._obs = SyntheticObs(_truth, H, R)
        self._lead, self._exc, self._t0 = lead, exc, None

    def get_obs_info(self, t):
        self._t0 = t
        return self._obs.get_obs_info(t)

    def truth(self, t):
        if self._t0 is not None and t >= self._t0 + self._lead * H6:
            raise self._exc(str(t))
        return _truth(t)


@pytest.mark.parametrize("exc", [FileNotFoundError, KeyError])
def test_missing_truth_ends_the_rollout(runs, nets, tmp_path, exc):
    import vaevar.cycle as vc

    H, R, _ = _setup()
    calls, real = [], vc.integrate

    def counting(model, x, mean, std, steps=1, out=None):
        calls.append(steps)
        return real(model, x, mean, std, steps, out)

    vc.integrate = counting
    try:
        _run(nets, tmp_path, "gap", T0 + 2 * H6, obs=_WindowedTruth(H, R, 3, exc), forecast_eval=True,
             forecast_steps=K)
    finally:
        vc.integrate = real
    got = np.load(os.path.join(str(tmp_path), "gap", "forecast_wrmse.npy"))
    full = np.load(os.path.join(runs["dir"], "on", "forecast_wrmse.npy"))
    assert got.shape == (2, K, 4) and np.isnan(got[:, 2]).all()
    check_bitwise("rollout with a missing truth, leads 1 and 2", got[:, :2], full[:, :2])
    assert calls == [1] * (2 * 2)  # the cycle's own step and lead 2; none towards the lead without a truth


def test_resumed_run_ends_with_the_same_file(runs, nets, tmp_path):
    _run(nets, tmp_path, "res", T0 + H6, forecast_eval=True, forecast_steps=K)
    one = np.load(os.path.join(str(tmp_path), "res", "forecast_wrmse.npy"))
    assert one.shape == (1, K, 4)
    cyc, _ = _run(nets, tmp_path, "res", T0 + 2 * H6, forecast_eval=True, forecast_steps=K)
    assert cyc.current_time == T0 + 2 * H6
    two = np.load(os.path.join(str(tmp_path), "res", "forecast_wrmse.npy"))
    check_bitwise("resumed forecast_wrmse.npy", two, np.load(os.path.join(runs["dir"], "on", "forecast_wrmse.npy")))


def test_other_scores_and_climatology(runs, nets, tmp_path):
    """Every requested score gets its file; a climatology score is scored against clim(t) of the lead's time."""
    seen = []

    def clim(t):
        seen.append(t)
        return _truth(t + dt.timedelta(hours=1000))

    cyc, _ = _run(nets, tmp_path, "cl", T0 + H6, forecast_eval=True, forecast_steps=2,
                  forecast_scores=("WRMSE", "TBias", "WACC"), clim=clim)
    assert seen == [T0 + H6, T0 + 2 * H6]
    d = os.path.join(str(tmp_path), "cl")
    assert sorted(f for f in os.listdir(d) if f.startswith("forecast_")) == \
        ["forecast_tbias.npy", "forecast_wacc.npy", "forecast_wrmse.npy"]
    w = np.load(os.path.join(d, "forecast_wacc.npy"))
    assert w.shape == (1, 2, 4) and np.isfinite(w).all() and (np.abs(w) <= 1 + 1e-6).all()
    check_bitwise("forecast_wrmse.npy with more scores", np.load(os.path.join(d, "forecast_wrmse.npy"))[0],
                  np.load(os.path.join(runs["dir"], "on", "forecast_wrmse.npy"))[0, :2])


def test_bad_keywords_raise(nets, tmp_path):
    from vaevar.cycle import CyclicVAE4DVar, SyntheticObs

    H, R, xb0 = _setup()
    dec, fc = nets
    obs = SyntheticObs(_truth, H, R)

    def make(**kw):
        return CyclicVAE4DVar(dec, fc, obs, T0, T0 + H6, Nit=1, name="bad", out_dir=str(tmp_path), xb0=xb0, **kw)

    with pytest.raises(ValueError, match="climatology"):
        make(forecast_eval=True, forecast_steps=K, forecast_scores=("WRMSE", "WACC"))
    with pytest.raises(ValueError, match="forecast_steps"):
        make(forecast_eval=True, forecast_steps=0)
    with pytest.raises(ValueError, match="forecast_steps"):
        make(forecast_eval=True)
    with pytest.raises(ValueError, match="forecast_scores"):
        make(forecast_eval=True, forecast_steps=K, forecast_scores=("RMSE",))
    make(forecast_scores=("WACC",))  # off: the forecast keywords are not looked at
