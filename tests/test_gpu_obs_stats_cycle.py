"""obs_stats through the analysis steps and the cycle driver (one_step_da, one_step_sc4dvar, CyclicDA) on
the GPU: tiny networks on their own grid, T = 2, two cycles, Nit = 1.

0.5 * sum of row JB (JA) is the closure's J_o at z = 0 (at the final z): the same fp32 terms in another fp64 order,
so the two agree within 4 n 2^-53 relative with n = Hs Ws. This holds where the closure forms x and its misfit per
element (k_misfit_fwd: the state grid is the network grid); on a larger state grid k_misfit_grid multiplies by one
reciprocal of R and agrees at fp32 level only. sc4dvar's states come from a separate integrate, so its comparison is
recorded, not bounded. With obs_stats on, every file a cycle writes without it keeps its bits."""
import datetime as dt
import os

import numpy as np
import pytest
import torch

import _obs_stats_ref as Rf
from conftest import GOLD, check, check_bitwise, note
from test_gpu_cycle import T0, _setup, _truth

pytestmark = pytest.mark.gpu
H6 = dt.timedelta(hours=6)
T, NIT = 2, 1


def _mask(seed, Hs, Ws, frac=0.3):
    from vaevar.synth import splitmix_uniform

    return (splitmix_uniform(seed, Hs * Ws).reshape(Hs, Ws) < frac).astype(np.float32)


@pytest.fixture(scope="module")
def nets():
    from vaevar import config as C
    from vaevar.engine import LGUnet

    return {"dec": LGUnet(C.TINY, 1, 1).load_synthetic(), "flow": LGUnet(C.TINY_FLOW, 1, 1).load_synthetic(),
            "fc": LGUnet(C.TINY_FLOW, 1, 1).load_synthetic()}


def _j_check(tag, table, J, n, bounded=True):
    for row, k, name in ((Rf.JB, 0, "background"), (Rf.JA, len(J) - 1, "analysis")):
        jo = J[k][1]
        half = 0.5 * table[:, :, row].sum()
        e = abs(half - jo) / abs(jo)
        print(f"{tag} {name}: 0.5 sum {Rf.NAMES[row]} = {half:.17e}, J_o = {jo:.17e}, rel {e:.2e}")
        if bounded:
            check(f"{tag} 0.5 * sum of row {Rf.NAMES[row]} vs J_o of the {name}", e, 4 * n * 2.0 ** -53, "<=")
        else:
            note(f"{tag} 0.5 * sum of row {Rf.NAMES[row]} vs J_o of the {name}", e)


def test_vae4dvar_tables_are_the_closures_j_o(nets):
    from vaevar.da import one_step_da
    from vaevar.engine import DAProblem, obs_stats
    from vaevar.problem import make_problem

    p = make_problem(nch=4, Hs=32, Ws=64, T=T, seed=7301, obs_frac=0.1)
    prob = DAProblem(nets["dec"], p, flow=nets["flow"])
    plain = one_step_da(prob, NIT)
    assert "obs_stats" not in plain
    res = one_step_da(prob, NIT, obs_stats=True)
    tab = res["obs_stats"]
    assert isinstance(tab, np.ndarray) and tab.shape == (T, 4, 10) and tab.dtype == np.float64
    assert "obs_stats_heldout" not in res and set(plain) | {"obs_stats"} == set(res)
    check_bitwise("vae4dvar xa with and without obs_stats", res["xa"], plain["xa"])
    check_bitwise("vae4dvar J with and without obs_stats", np.asarray(res["J"]), np.asarray(plain["J"]))
    assert res["n_eval"] == plain["n_eval"] and res["n_iter"] == plain["n_iter"]
    assert np.isfinite(tab).all() and (tab[:, :, Rf.COUNT] == (p["H"] != 0).sum((2, 3))).all()
    _j_check("vae4dvar tiny T = 2", tab, res["J"], 32 * 64)
    assert tab[:, :, Rf.JA].sum() < tab[:, :, Rf.JB].sum()  # the analysis fits the observations better
    # without per-pass logging: two J-only evaluations of its own, the same table, the same count of evaluations
    quiet = one_step_da(prob, NIT, log_terms=False, obs_stats=True)
    check_bitwise("vae4dvar table without log_terms", quiet["obs_stats"], tab)
    check_bitwise("vae4dvar xa without log_terms", quiet["xa"], plain["xa"])
    assert quiet["n_eval"] == plain["n_eval"] and quiet["J"] == []
    # the table is obs_stats of the two trajectories
    z0 = torch.zeros_like(res["z"])
    prob.closure(z0, None)
    xb_win = prob.trajectory()
    prob.closure(res["z"], None)
    direct = obs_stats(prob.ctx, xb_win, prob.trajectory(), prob.yo, prob.H, prob.R)
    check_bitwise("vae4dvar table vs obs_stats of the two trajectories", direct, tab)


def test_batched_problem_is_refused():
    from vaevar import config as C
    from vaevar.da import one_step_da
    from vaevar.engine import DAProblem, LGUnet
    from vaevar.problem import make_problem

    probs = [make_problem(nch=4, Hs=32, Ws=64, T=1, seed=7310 + b, obs_frac=0.1) for b in range(2)]
    pb = DAProblem(LGUnet(C.TINY, 2, 1).load_synthetic(), probs)
    with pytest.raises(ValueError, match="single analysis"):
        one_step_da(pb, 1, obs_stats=True)


def test_sc4dvar_tables(nets):
    from vaevar import config as C
    from vaevar.engine import LGUnet, obs_stats
    from vaevar.problem import make_problem
    from vaevar.sc4dvar import BMatrix, Sc4dvarProblem, one_step_sc4dvar

    p = make_problem(nch=69, Hs=128, Ws=256, T=T, seed=7302, obs_frac=0.03)
    flow = LGUnet(C.FLOW, 1, 1).load_synthetic()
    prob = Sc4dvarProblem(BMatrix.from_npz(os.path.join(GOLD, "bq_info_lr.npz")), p, flow=flow)
    plain = one_step_sc4dvar(prob, NIT)
    res = one_step_sc4dvar(prob, NIT, obs_stats=True)
    tab = res["obs_stats"]
    assert tab.shape == (T, 69, 10) and np.isfinite(tab).all() and set(plain) | {"obs_stats"} == set(res)
    check_bitwise("sc4dvar xa with and without obs_stats", res["xa"], plain["xa"])
    check_bitwise("sc4dvar J with and without obs_stats", np.asarray(res["J"]), np.asarray(plain["J"]))
    assert res["n_eval"] == plain["n_eval"]
    _j_check("sc4dvar 128x256 T = 2", tab, res["J"], 128 * 256, bounded=False)
    win = prob.window(res["w"])
    assert win.shape == (T, 69, 128, 256)
    check_bitwise("sc4dvar window level 0 = xa", win[0], res["xa"])
    direct = obs_stats(prob.ctx, prob.window(torch.zeros_like(res["w"])), win, prob.yo, prob.H, prob.R)
    check_bitwise("sc4dvar table vs obs_stats of the two windows", direct, tab)


def _obs():
    from vaevar.cycle import SyntheticObs

    H, R, xb0 = _setup()
    H2, R2 = np.repeat(H, T, 0), np.repeat(R, T, 0) * np.asarray([1.0, 1.5], np.float32).reshape(T, 1, 1, 1)
    return SyntheticObs(_truth, H2, R2, da_win=T), H2, xb0


def _files(d):
    return {f: (np.load(os.path.join(d, f)) if f.endswith(".npy") else open(os.path.join(d, f)).read())
            for f in sorted(os.listdir(d))}


def test_cycle_on_versus_off_resume_and_use_eval(tmp_path, nets):
    from vaevar.calib import DepartureStats
    from vaevar.cycle import CyclicDA

    obs, H2, xb0 = _obs()
    mask = _mask(79, 32, 64)
    end = T0 + 2 * H6
    kw = dict(Nit=NIT, decoder=nets["dec"], flow=nets["flow"], out_dir=str(tmp_path), xb0=xb0, use_eval=True,
              mask_eval=mask, save_field=True)

    def run(name, until=end, **over):
        cyc = CyclicDA(nets["fc"], obs, T0, until, name=name, **dict(kw, **over))
        xas, js = [], []
        cyc.run_assimilation(log=lambda t, res: (xas.append(res["xa"].clone()), js.append(res["J"])))
        return cyc, xas, js

    off, xas_off, _ = run("off")
    on, xas_on, js_on = run("on", obs_stats=True)
    assert not hasattr(off, "departures") and off.departure_tables == {}
    assert set(on.metrics_list) == set(off.metrics_list)  # the reference's key set
    f_off, f_on = _files(os.path.join(str(tmp_path), "off")), _files(os.path.join(str(tmp_path), "on"))
    assert set(f_on) - set(f_off) == {"obs_stats.npy", "obs_stats_heldout.npy"} and set(f_off) <= set(f_on)
    assert {"xb.npy", "bg_wrmse.npy", "ana_wrmse.npy", "bg_bias.npy", "ana_bias.npy", "error_obs.npy"} <= set(f_off)
    for f, v in f_off.items():
        if isinstance(v, str):
            assert f_on[f] == v, f
        else:
            assert f_on[f].dtype == v.dtype, f
            check_bitwise(f"{f} with obs_stats on vs off", f_on[f], v)
    for k in range(2):
        check_bitwise(f"cycle {k} xa with obs_stats on vs off", xas_on[k], xas_off[k])
    tabs, held = f_on["obs_stats.npy"], f_on["obs_stats_heldout.npy"]
    assert tabs.shape == held.shape == (2, T, 4, 10) and tabs.dtype == held.dtype == np.float64
    assert np.isfinite(tabs).all()
    n_held = ((H2 * mask) != 0).sum((2, 3))
    n_seen = ((H2 * (1 - mask)) != 0).sum((2, 3))
    for k in range(2):
        check_bitwise(f"cycle {k} held-out count = sum(H_old * mask_eval != 0)", held[k, :, :, Rf.COUNT], n_held)
        check_bitwise(f"cycle {k} count = the entries the analysis saw", tabs[k, :, :, Rf.COUNT], n_seen)
        _j_check(f"cycle {k}", tabs[k], js_on[k], 32 * 64)
    assert n_held.sum() > 40 and (held[:, :, :, Rf.COUNT] > 0).any()
    # the accumulated departures are the sum of the cycles' tables
    assert isinstance(on.departures, DepartureStats) and on.departures.cycles == 2
    check_bitwise("departures = the sum of the cycles' tables", on.departures.table, tabs[0] + tabs[1])
    s = on.departures.summary()
    assert s["n"].shape == (T, 4) and (s["rms_oa"] < s["rms_ob"]).all() and np.isfinite(s["r_desroziers"]).all()

    # resume: one cycle, then a second driver over the same directory ends with an uninterrupted run's bits
    run("resumed", until=T0 + H6, obs_stats=True)
    d = os.path.join(str(tmp_path), "resumed")
    assert np.load(os.path.join(d, "obs_stats.npy")).shape == (1, T, 4, 10)
    cyc2 = CyclicDA(nets["fc"], obs, T0, end, name="resumed", **dict(kw, obs_stats=True, xb0=None))
    assert cyc2.current_time == T0 + H6 and len(cyc2.departure_tables["obs_stats"]) == 1
    assert cyc2.departures.cycles == 1
    cyc2.run_assimilation()
    for f in ("obs_stats.npy", "obs_stats_heldout.npy", "error_obs.npy", "xb.npy"):
        check_bitwise(f"{f} of a resumed run vs an uninterrupted one", np.load(os.path.join(d, f)), f_on[f])
    check_bitwise("departures of a resumed run", cyc2.departures.table, on.departures.table)


def test_free_run_records_the_background_at_level_0(tmp_path, nets):
    from vaevar import config as C
    from vaevar.cycle import CyclicDA, CyclicInterpolation
    from vaevar.engine import obs_stats

    obs, H2, xb0 = _obs()
    mean, std = np.asarray(C.MODEL_MEAN[:4], np.float32), np.asarray(C.MODEL_STD[:4], np.float32)
    kw = dict(Nit=1, da_mode="free_run", out_dir=str(tmp_path), xb0=xb0, mean=mean, std=std,
              std_tr=np.asarray(C.STD_TR[:4], np.float32))
    cyc = CyclicDA(nets["fc"], obs, T0, T0 + 2 * H6, name="free", obs_stats=True, **kw)
    cyc.run_assimilation()
    CyclicDA(nets["fc"], obs, T0, T0 + 2 * H6, name="free_off", **kw).run_assimilation()
    f_on, f_off = _files(os.path.join(str(tmp_path), "free")), _files(os.path.join(str(tmp_path), "free_off"))
    assert set(f_on) - set(f_off) == {"obs_stats.npy"}
    for f, v in f_off.items():
        if not isinstance(v, str):
            check_bitwise(f"free_run {f} with obs_stats on vs off", f_on[f], v)
    tabs = f_on["obs_stats.npy"]
    assert tabs.shape == (2, T, 4, 10) and np.isnan(tabs[:, 1:]).all()
    assert np.isnan(tabs[:, 0][:, :, list(Rf.ANALYSIS_ROWS)]).all()
    yo, H, R, _ = obs.get_obs_info(T0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[:1])).cuda()  # noqa: E731
    direct = obs_stats(nets["fc"].ctx, torch.from_numpy(xb0).cuda()[None], None, dev(yo), dev(H), dev(R))
    check_bitwise("free_run cycle 0, time level 0 vs obs_stats of xb", tabs[0, 0], direct[0])
    with pytest.raises(ValueError, match="obs_stats"):
        CyclicInterpolation(nets["fc"], obs, T0, T0 + H6, name="interp", out_dir=str(tmp_path), xb0=xb0,
                            obs_stats=True)
