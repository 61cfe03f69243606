"""The cycle driver for the three da_modes and --use_eval (vaevar.cycle.CyclicDA: da_4dvar.py:933-966 free_run,
:1064-1177 sc4dvar, :1179-1306 vae4dvar, :934-937 / :1154-1155 / :1285-1286 the held-out verification) on the GPU.
Analyses are compared bit for bit with the same steps composed by hand; error_obs and the free-run MSE against the
torch CPU restatements of tests/_obs_error_ref.py under its rule e_hip <= max(4 e_ref, 5e-7)."""
import datetime as dt
import os

import numpy as np
import pytest
import torch

from _obs_error_ref import check_error_obs, mse_ref
from conftest import GOLD, check, check_bitwise, note
from test_gpu_cycle import T0, _setup, _truth

pytestmark = pytest.mark.gpu
BQ = os.path.join(GOLD, "bq_info_lr.npz")
H6 = dt.timedelta(hours=6)


def _mask(seed, Hs, Ws, frac=0.3):
    from vaevar.synth import splitmix_uniform

    return (splitmix_uniform(seed, Hs * Ws).reshape(Hs, Ws) < frac).astype(np.float32)


class _ShiftedObs:
    """SyntheticObs with the observations moved by `shift` (C,1,1) at the pixels `where` (Hs,Ws) only."""

    def __init__(self, base, where, shift):
        self.base, self.where, self.shift = base, where, shift

    def get_obs_info(self, t):
        yo, H, R, gt = self.base.get_obs_info(t)
        return (yo + self.shift * self.where).astype(np.float32), H, R, gt


def test_vae4dvar_use_eval_tiny_and_resume(tmp_path):
    from vaevar import config as C
    from vaevar.cycle import CyclicDA, SyntheticObs
    from vaevar.engine import LGUnet

    H, R, xb0 = _setup()
    mask = _mask(79, 32, 64)
    assert (H[0, 0] * mask).sum() > 20  # held-out observations exist
    dec = LGUnet(C.TINY, 1, 1).load_synthetic()
    fc = LGUnet(C.TINY_FLOW, 1, 1).load_synthetic()
    end = T0 + 2 * H6

    def run(name, obs):
        cyc = CyclicDA(fc, obs, T0, end, Nit=1, name=name, decoder=dec, out_dir=str(tmp_path), xb0=xb0,
                       use_eval=True, mask_eval=mask)
        xas = []
        cyc.run_assimilation(log=lambda t, res: xas.append(res["xa"].cpu().numpy()))
        return cyc, xas

    obs = SyntheticObs(_truth, H, R)
    cyc, xas = run("eval", obs)
    eo = np.load(os.path.join(str(tmp_path), "eval", "error_obs.npy"))
    assert eo.shape == (2, 4) and eo.dtype == np.float32 and len(xas) == 2
    for k in range(2):
        yo = _truth(T0 + k * H6)
        check_error_obs(f"vae4dvar cycle {k} error_obs", eo[k], xas[k], yo, H[0], mask, None, nan_channels=[])
    assert np.load(os.path.join(str(tmp_path), "eval", "ana_wrmse.npy")).shape == (2, 4)

    # the reduced mask is what was bound: observations moved at held-out pixels only leave every analysis unchanged
    # bit for bit, and change the verification
    std = np.asarray(C.MODEL_STD[:4], np.float32)[:, None, None]
    cyc_s, xas_s = run("eval_shift", _ShiftedObs(obs, mask, 3 * std))
    for k in range(2):
        check_bitwise(f"cycle {k} xa with observations moved at held-out pixels", xas_s[k], xas[k])
    eo_s = np.asarray(cyc_s.metrics_list["error_obs"])
    check("error_obs rows unchanged by the moved observations", np.count_nonzero((eo_s == eo).all(1)), 0, "==")
    # without use_eval the same move does change the analysis (the control of the check above)
    cyc_c = CyclicDA(fc, _ShiftedObs(obs, mask, 3 * std), T0, T0 + H6, Nit=1, name="ctl", decoder=dec,
                     out_dir=str(tmp_path), xb0=xb0)
    cyc_c.run_assimilation()
    assert not np.array_equal(cyc_c.xa.cpu().numpy(), xas[0])
    assert len(cyc_c.metrics_list["error_obs"]) == 0

    # resume: a second driver over the same directory reloads error_obs and continues
    cyc2 = CyclicDA(fc, obs, T0, end + H6, Nit=1, name="eval", decoder=dec, out_dir=str(tmp_path), use_eval=True,
                    mask_eval=mask)
    assert cyc2.current_time == end and len(cyc2.metrics_list["error_obs"]) == 2
    check_bitwise("use_eval resume xb", cyc2.xb, cyc.xb)
    check_bitwise("use_eval resume error_obs", np.asarray(cyc2.metrics_list["error_obs"]), eo)
    cyc2.run_assimilation()
    assert np.load(os.path.join(str(tmp_path), "eval", "error_obs.npy")).shape == (3, 4)


@pytest.fixture(scope="module")
def sc_setup():
    from vaevar import config as C
    from vaevar.engine import LGUnet
    from vaevar.problem import make_problem
    from vaevar.sc4dvar import BMatrix
    from vaevar.synth import smooth_field

    mean = np.asarray(C.MODEL_MEAN, np.float32)[:, None, None]
    std = np.asarray(C.MODEL_STD, np.float32)[:, None, None]
    fields = {}

    def truth(t):
        k = int((t - T0).total_seconds() // 3600)
        if k not in fields:
            fields[k] = (mean + std * smooth_field(6100 + k, (69, 128, 256))).astype(np.float32)
        return fields[k]

    p = make_problem(nch=69, Hs=128, Ws=256, T=1, seed=8181, obs_frac=0.03)
    fc = LGUnet(C.FLOW, 1, 1).load_synthetic()  # the flow network stands in as the forecast model
    return {"truth": truth, "p": p, "fc": fc, "bmat": BMatrix.from_npz(BQ), "mask": _mask(83, 128, 256)}


@pytest.mark.parametrize("kind", ["synthetic", "real"])
def test_sc4dvar_cycle_matches_manual_composition(tmp_path, sc_setup, kind):
    from vaevar.cycle import CyclicDA, SyntheticObs, SyntheticRealObs
    from vaevar.engine import integrate
    from vaevar.metrics import held_out
    from vaevar.problem import ObsInterpolater
    from vaevar.sc4dvar import Sc4dvarProblem, one_step_sc4dvar
    from vaevar.synth import splitmix_uniform

    s = sc_setup
    p, fc, mask = s["p"], s["fc"], s["mask"]
    if kind == "real":
        interp = ObsInterpolater(13, 40).interp
        H = (splitmix_uniform(84, 204 * 128 * 256).reshape(1, 204, 128, 256) < 0.03).astype(np.float32)
        obs = SyntheticRealObs(fc.ctx, s["truth"], H, p["R"], interp)
    else:
        interp = None
        obs = SyntheticObs(s["truth"], p["H"], p["R"])
    c_obs = 204 if kind == "real" else 69
    cyc = CyclicDA(fc, obs, T0, T0 + 2 * H6, Nit=1, name=kind, da_mode="sc4dvar", bmatrix=s["bmat"],
                   out_dir=str(tmp_path), xb0=p["xb"], obs_interp=interp, use_eval=True, mask_eval=mask)
    xas = []
    cyc.run_assimilation(log=lambda t, res: xas.append(res["xa"].clone()))
    assert len(xas) == 2
    eo = np.load(os.path.join(str(tmp_path), kind, "error_obs.npy"))
    assert eo.shape == (2, c_obs) and eo.dtype == np.float32
    # by hand: the reduced mask bound, one_step_sc4dvar without logging, the forecast
    xb = torch.from_numpy(p["xb"]).cuda()
    for k in range(2):
        yo, H_all, R, gt = obs.get_obs_info(T0 + k * H6)
        H_red, H_old = held_out(H_all, mask)
        prob = Sc4dvarProblem(s["bmat"], {"xb": xb, "yo": yo, "H": H_red, "R": R, "mean": cyc.mean, "std": cyc.std},
                              obs_interp=interp)
        xa = one_step_sc4dvar(prob, nit=1)["xa"]
        check_bitwise(f"sc4dvar {kind} cycle {k} xa vs hand composition", xa, xas[k])
        check_error_obs(f"sc4dvar {kind} cycle {k} error_obs", eo[k], xa.cpu(), torch.as_tensor(yo)[0].cpu(),
                        H_old[0].cpu(), mask, interp, nan_channels=[])
        xb = integrate(fc, xa, cyc.mean_d, cyc.std_d, 1)
    check_bitwise(f"sc4dvar {kind} cycle xb vs hand composition", xb, cyc.xb)
    for key in ("bg_wrmse", "ana_wrmse", "bg_bias", "ana_bias"):
        w = np.load(os.path.join(str(tmp_path), kind, key + ".npy"))
        assert w.shape == (2, 69) and np.isfinite(w).all(), key


def test_one_step_sc4dvar_logging(sc_setup):
    """The WRMSE / Bias logged on pass 0 are those of the background (transform(0) = xb), the logging changes no
    analysis, and the existing keys stay."""
    from vaevar.metrics import Metrics
    from vaevar.sc4dvar import Sc4dvarProblem, one_step_sc4dvar

    s = sc_setup
    p = s["p"]
    prob = Sc4dvarProblem(s["bmat"], p)
    m = Metrics(prob.ctx)
    gt = torch.from_numpy(p["gt"]).cuda()
    plain = one_step_sc4dvar(prob, nit=1)
    assert "metrics" not in plain and "error_obs" not in plain
    res = one_step_sc4dvar(prob, nit=1, gt=gt, metrics=m)
    assert set(plain) <= set(res) and len(res["metrics"]) == 2
    check_bitwise("sc4dvar xa with and without logging", res["xa"], plain["xa"])
    w, b = m.wrmse_bias(torch.from_numpy(p["xb"]).cuda(), gt[0])
    check_bitwise("sc4dvar pass 0 WRMSE = background WRMSE", res["metrics"][0][0], w)
    check_bitwise("sc4dvar pass 0 Bias = background Bias", res["metrics"][0][1], b)
    w1, b1 = m.wrmse_bias(res["xa"], gt[0])
    check_bitwise("sc4dvar pass Nit WRMSE = analysis WRMSE", res["metrics"][1][0], w1)
    with pytest.raises(ValueError, match="H_old"):
        one_step_sc4dvar(prob, nit=1, mask_eval=s["mask"], metrics=m)


def test_free_run_cycle(tmp_path):
    from vaevar import config as C
    from vaevar.cycle import CyclicDA, SyntheticObs
    from vaevar.engine import LGUnet, integrate

    H, R, xb0 = _setup()
    mean, std = np.asarray(C.MODEL_MEAN[:4], np.float32), np.asarray(C.MODEL_STD[:4], np.float32)
    fc = LGUnet(C.TINY_FLOW, 1, 1).load_synthetic()
    obs = SyntheticObs(_truth, H, R)
    cyc = CyclicDA(fc, obs, T0, T0 + 2 * H6, Nit=1, name="free", da_mode="free_run", out_dir=str(tmp_path),
                   xb0=xb0, mean=mean, std=std, std_tr=np.asarray(C.STD_TR[:4], np.float32))
    xb_first = cyc.xb
    yo, Hh, Rr, gt = obs.get_obs_info(T0)
    assert cyc.one_step_DA(gt, xb_first, yo, Hh, Rr) is xb_first  # xa = xb, the same tensor
    for v in cyc.metrics_list.values():
        v.clear()
    xbs = []
    cyc.run_assimilation(log=lambda t, res: xbs.append(res["xa"]))
    assert len(xbs) == 2 and xbs[0] is xb_first
    xb = torch.from_numpy(xb0).cuda()
    for k in range(2):
        check_bitwise(f"free_run cycle {k} xa = xb", xbs[k], xb)
        m32, m64 = (mse_ref(xb.cpu().numpy(), _truth(T0 + k * H6), mean, std, d) for d in (torch.float32, torch.float64))
        e_ref = abs(m32 - m64) / m64
        e_hip = abs(cyc.metrics_list["bg_mse"][k] - m64) / m64
        print(f"free_run cycle {k} MSE: e_hip {e_hip:.2e}, e_ref {e_ref:.2e}")
        note(f"free_run cycle {k} bg_mse e_ref", e_ref)
        check(f"free_run cycle {k} bg_mse e_hip", e_hip, max(4 * e_ref, 5e-7), "<=")
        xb = integrate(fc, xb, cyc.mean_d, cyc.std_d, 1)
    check_bitwise("free_run xb = two forecasts", cyc.xb, xb)
    d = os.path.join(str(tmp_path), "free")
    for k in ("wrmse", "bias", "mse"):
        bg, ana = np.load(os.path.join(d, f"bg_{k}.npy")), np.load(os.path.join(d, f"ana_{k}.npy"))
        assert bg.shape == ((2, 4) if k != "mse" else (2,)) and np.isfinite(bg).all()
        check_bitwise(f"free_run bg_{k} = ana_{k}", bg, ana)
    assert np.load(os.path.join(d, "error_obs.npy")).size == 0
    assert open(os.path.join(d, "current_time.txt")).read() == "2018-01-01 12:00:00"


def test_unknown_da_mode_and_batched_mask_eval():
    from vaevar import config as C
    from vaevar.cycle import CyclicDA
    from vaevar.da import one_step_da
    from vaevar.engine import DAProblem, LGUnet
    from vaevar.metrics import Metrics, held_out
    from vaevar.problem import make_problem

    with pytest.raises(NotImplementedError):
        CyclicDA(None, None, T0, T0 + H6, Nit=1, name="x", da_mode="interpolation")
    probs = [make_problem(nch=4, Hs=32, Ws=64, T=1, seed=780 + b, obs_frac=0.1) for b in range(2)]
    dec2 = LGUnet(C.TINY, 2, 1).load_synthetic()
    pb = DAProblem(dec2, probs)
    mask = _mask(79, 32, 64)
    _, H_old = held_out(probs[0]["H"], mask)
    m = Metrics(dec2.ctx, C.MODEL_MEAN[:4], C.MODEL_STD[:4])
    with pytest.raises(ValueError, match="single analysis"):
        one_step_da(pb, 1, metrics=m, mask_eval=mask, H_old=H_old)
