"""vv_obs_grid / engine.obs_grid / cycle.StationObs / cycle.ReportMaskObs (the gridding of station reports:
data_reader.get_real_obs, da_4dvar.py:301-440, and get_obs_mask for obs_type prepbufr*, :190-274) on the GPU against
the per-row numpy restatement (tests/_obs_grid_ref.py), which tests/test_obs_grid_host.py pins bitwise to the
reference's own output for the golden reports (tests/golden/g17_obs_grid.npz).

What is exact: H, stats, yo on the q, u, v, msl and surface channels (fp64 products and sums of the same operands round
identically; the fp32 additions happen in row order on both sides), determinism (two calls are bitwise equal), and
that the call overwrites buffers pre-filled with garbage. What has a tolerance: yo on the z and t channels, whose values
go through the device's fp64 log: at most 1 fp32 ulp of the reference per cell (the log's last fp64 bit can move a
value across an fp32 rounding boundary, about one value in 10^7); the number of such cells is recorded.

Grids 33 x 47, 1 x 300 (one row: every latitude lands on it) and 67 x 131; 40 and 7 levels; da_win 1 and 6; tables of
0, 1 and 5000 rows, 5000 rows confined to 20 pixels (lists of tens of members), 12 / 300 / 5000 rows in one cell (the
thread walk up to 16 members, the wave's merge sort beyond, more than 64 x 64 members), and the order case."""
import datetime as dt
import os

import numpy as np
import pytest
import torch

from _obs_grid_ref import MASK, REAL, dense, levels_of, obs_grid_ref, one_cell_table, random_table
from conftest import GOLD, check, check_bitwise

pytestmark = pytest.mark.gpu

GRIDS = {"33x47": (33, 47), "1x300": (1, 300), "67x131": (67, 131)}
T0 = dt.datetime(2018, 1, 1, 0)
H6 = dt.timedelta(hours=6)

# (grid, n_lev, da_win, kind, n)
CASES = [("33x47", 40, 1, "random", 5000), ("33x47", 7, 6, "random", 5000), ("1x300", 7, 1, "random", 5000),
         ("1x300", 40, 6, "random", 1), ("67x131", 40, 6, "random", 5000), ("67x131", 7, 1, "random", 0),
         ("33x47", 7, 6, "random", 1), ("67x131", 7, 6, "cells20", 5000), ("33x47", 40, 1, "cells20", 5000),
         ("33x47", 7, 1, "onecell", 12), ("33x47", 40, 6, "onecell", 300), ("67x131", 7, 1, "onecell", 5000),
         ("1x300", 7, 6, "order", 12), ("33x47", 7, 1, "order", 300), ("67x131", 40, 6, "order", 5000)]


def _id(c):
    return f"{c[0]}-L{c[1]}-w{c[2]}-{c[3]}{c[4]}"


@pytest.fixture(scope="module")
def ctx():
    from vaevar.engine import Context

    return Context.get(0)


_TABLES: dict = {}


def _table(key):
    """The seeded table of a case and the restatement's result, computed once and never modified."""
    if key not in _TABLES:
        g, n_lev, da_win, kind, n = key
        Hs, Ws = GRIDS[g]
        seed = 7100 + 13 * CASES.index(key)
        if kind == "random":
            t = random_table(n, n_lev, da_win, seed)
        elif kind == "cells20":
            t = random_table(n, n_lev, da_win, seed, cells=20, Hs=Hs, Ws=Ws)
        else:
            t = one_cell_table(n, n_lev, da_win, seed, order=kind == "order")
        _TABLES[key] = (t, obs_grid_ref(t, REAL, da_win, levels_of(n_lev), Hs, Ws))
    return _TABLES[key]


def _zt_channels(idx, n_lev, HW):
    """True where a flat cell index lies on a z or an upper-air t channel (the values that go through the log)."""
    ch = (idx // HW) % (4 + 5 * n_lev)
    return ((ch >= 4) & (ch < 4 + n_lev)) | (ch >= 4 + 4 * n_lev)


def _check_yo(tag, got, ref, zt):
    """got, ref: fp32 values at the observed cells; exact off the z / t channels, within 1 ulp of the reference on
    them."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert np.isfinite(got).all() and got.shape == ref.shape
    check(f"{tag} yo, cells off the z / t channels that are not bitwise",
          np.count_nonzero(got[~zt].view(np.uint32) != ref[~zt].view(np.uint32)), 0, "==")
    if zt.any():
        ulps = np.abs(got[zt].astype(np.float64) - ref[zt]) / np.spacing(np.abs(ref[zt])).astype(np.float64)
        check(f"{tag} yo on the z / t channels, max error in fp32 ulps of the reference", ulps.max(), 1.0, "<=")
        check(f"{tag} yo, z / t cells that are not bitwise (of {int(zt.sum())})", np.count_nonzero(ulps), zt.sum(), "<=")


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_obs_grid_vs_restatement(ctx, key):
    from vaevar.engine import obs_grid

    g, n_lev, da_win, kind, n = key
    Hs, Ws = GRIDS[g]
    t, (idx, yo_r, st_r) = _table(key)
    shape = (da_win, 4 + 5 * n_lev, Hs, Ws)
    yo = torch.full(shape, float("nan"), device="cuda")  # garbage: the call overwrites everything
    H = torch.full(shape, -7.5, device="cuda")
    y1, H1, st = obs_grid(ctx, t, REAL, da_win, levels_of(n_lev), Hs, Ws, out=(yo, H))
    assert y1 is yo and H1 is H and st.dtype == torch.int64
    tag = _id(key)
    check_bitwise(f"{tag} stats (rows used, skipped, dropped, cells)", st, st_r)
    check_bitwise(f"{tag} H", H, dense(idx, None, shape))
    yo_h = yo.cpu().numpy().reshape(-1)
    rest = np.ones(yo_h.size, bool)
    rest[idx] = False
    check(f"{tag} yo, unobserved cells that are not +0", np.count_nonzero(yo_h[rest].view(np.uint32)), 0, "==")
    _check_yo(tag, yo_h[idx], yo_r, _zt_channels(idx, n_lev, Hs * Ws))
    if n == 0:
        assert len(idx) == 0 and st.tolist() == [0, 0, 0, 0]
    if kind in ("onecell", "order"):
        assert len(idx) == 9 and st_r[0] == n  # nine lists of n members
    # determinism: a second call into fresh buffers
    y2, H2, st2 = obs_grid(ctx, t, REAL, da_win, levels_of(n_lev), Hs, Ws)
    assert torch.equal(y2.view(torch.int32), yo.view(torch.int32)) and torch.equal(H2, H) and torch.equal(st2, st)


def test_order_case_is_order_sensitive(ctx):
    """The control of the order cases: the same rows reversed give another fp32 result on the device too, so a kernel
    that added in any other order than the rows' would not pass them."""
    from vaevar.engine import obs_grid

    t = _table(("33x47", 7, 1, "order", 300))[0]
    a = obs_grid(ctx, t, REAL, 1, levels_of(7), 33, 47)[0]
    b = obs_grid(ctx, t[::-1].copy(), REAL, 1, levels_of(7), 33, 47)[0]
    idx, yo_b, _ = obs_grid_ref(t[::-1], REAL, 1, levels_of(7), 33, 47)
    assert not torch.equal(a, b)
    _check_yo("reversed order case", b.cpu().numpy().reshape(-1)[idx], yo_b, _zt_channels(idx, 7, 33 * 47))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g17_obs_grid.npz"))


@pytest.mark.parametrize("name", ["real_w1_n40", "real_w6_n7", "mask_w6"])
def test_golden_cases_at_721x1440(ctx, gold, name):
    """The reference's own output for the golden reports, compared on the device: H and yo gathered at the fixture's
    indices, H.sum() and sum |yo| over the complement; no dense grid is downloaded."""
    from vaevar.engine import obs_grid

    da_win, n_out = (int(x) for x in gold[name + "_meta"])
    mask = name.startswith("mask")
    idx = torch.from_numpy(gold[name + "_idx"]).cuda()
    table = gold[name + "_table"]
    if mask:
        _, H, st = obs_grid(ctx, table, MASK, da_win, None, 721, 1440)
        assert tuple(H.shape) == (6, 69, 721, 1440)
    else:
        yo, H, st = obs_grid(ctx, table, REAL, da_win, levels_of(n_out), 721, 1440)
    Hf = H.reshape(-1)
    check(f"{name} H at the reference's cells that is not 1", int((Hf[idx] != 1).sum()), 0, "==")
    check(f"{name} H.sum() - the reference's cell count", float(Hf.sum(dtype=torch.float64)) - len(idx), 0, "==")
    st = st.cpu().numpy()
    assert st[2] == 0 and st[3] == len(idx) and st[:3].sum() == len(table)
    if not mask:
        yf = yo.reshape(-1)
        got = yf[idx].cpu().numpy()
        yf[idx] = 0.0
        check(f"{name} sum |yo| off the reference's cells", float(yf.abs().sum(dtype=torch.float64)), 0, "==")
        _check_yo(name, got, gold[name + "_yo"], _zt_channels(gold[name + "_idx"], n_out, 721 * 1440))


@pytest.mark.parametrize("g,da_win,n", [("33x47", 6, 5000), ("67x131", 1, 5000), ("1x300", 6, 0), ("33x47", 1, 1)])
def test_mask_mode(ctx, g, da_win, n):
    from vaevar.engine import obs_grid

    Hs, Ws = GRIDS[g]
    t = random_table(n, 13, da_win, 7700 + n + da_win, p_none=0.2)
    idx, _, st_r = obs_grid_ref(t, MASK, da_win, None, Hs, Ws)
    shape = (da_win, 69, Hs, Ws)
    yo = torch.full(shape, 3.25, device="cuda")
    H = torch.full(shape, float("nan"), device="cuda")
    y1, H1, st = obs_grid(ctx, t, MASK, da_win, None, Hs, Ws, out=(yo, H))
    tag = f"mask {g} w{da_win} n{n}"
    check_bitwise(f"{tag} H", H, dense(idx, None, shape))
    check_bitwise(f"{tag} stats", st, st_r)
    assert y1 is yo and bool((yo == 3.25).all())  # yo is not touched
    y2, H2, st2 = obs_grid(ctx, t, MASK, da_win, None, Hs, Ws)  # a NULL yo
    assert y2 is None and torch.equal(H2, H) and torch.equal(st2, st)
    if n == 5000:
        assert st_r[2] > 0 and bool((H[:, :3].sum() > 0)) and bool((H[:, 3].sum() > 0))
        assert torch.equal(H[:, 0], H[:, 4 + 2 * 13 + 12]) and torch.equal(H[:, 2], H[:, 68])


def test_engine_obs_grid_rejects(ctx):
    from vaevar._lib import VVError
    from vaevar.engine import obs_grid

    t = random_table(10, 7, 1, 1)
    with pytest.raises(VVError, match="da_win"):
        obs_grid(ctx, t, REAL, 3, levels_of(7), 8, 8)
    with pytest.raises(ValueError):
        obs_grid(ctx, t[:, :11], REAL, 1, levels_of(7), 8, 8)
    with pytest.raises(ValueError):
        obs_grid(ctx, t, 2, 1, levels_of(7), 8, 8)


def _truth69(t):
    from vaevar import config as C
    from vaevar.synth import smooth_field

    k = int((t - T0).total_seconds() // 3600)
    mean = np.asarray(C.MODEL_MEAN, np.float32)[:, None, None]
    std = np.asarray(C.MODEL_STD, np.float32)[:, None, None]
    return (mean + std * smooth_field(7300 + k, (69, 128, 256))).astype(np.float32)


def _reports(da_win):
    def f(t):
        k = int((t - T0).total_seconds() // 3600)
        tab = random_table(3000, 7, da_win, 7400 + k)
        tab[:, 6] = np.where(np.isnan(tab[:, 6]) | (tab[:, 6] == 0), tab[:, 6], 5000.0 + tab[:, 6] / 10)  # plausible z
        return tab
    return f


@pytest.mark.parametrize("obs_type", ["real", "real_simu"])
def test_station_obs_vs_real_obs(ctx, obs_type):
    """StationObs.get_obs_info against RealObs whose reader returns the restatement's grids of the same table: H' and
    the counts bitwise, yo' within the rule above (bitwise off the z / t channels)."""
    from vaevar.cycle import RealObs, StationObs
    from vaevar.problem import ObsInterpolater, make_problem

    oi = ObsInterpolater(13, 7)
    R = make_problem(nch=69, Hs=128, Ws=256, T=6, seed=41)["R"]
    rep = _reports(6)
    shape = (6, 39, 128, 256)

    def reader(t):
        idx, yo, _ = obs_grid_ref(rep(t), REAL, 6, oi.height_level_new, 128, 256)
        return dense(idx, yo, shape), dense(idx, None, shape)

    kw = dict(filter_coeff=30.0, da_win=6)
    sta = StationObs(ctx, _truth69, rep, R, oi.interp, oi, obs_type, **kw)
    real = RealObs(ctx, _truth69, reader, R, oi.interp, obs_type, **kw)
    ya, Ha, Ra, ga = sta.get_obs_info(T0)
    yb, Hb, Rb, gb = real.get_obs_info(T0)
    check_bitwise(f"StationObs {obs_type} H' vs RealObs on the restatement's grids", Ha, Hb)
    check_bitwise(f"StationObs {obs_type} counts", sta.counts, real.counts)
    check_bitwise(f"StationObs {obs_type} R", Ra, Rb)
    check_bitwise(f"StationObs {obs_type} gt", ga, gb)
    assert sta.counts.shape == (6, 2) and 0 < sta.counts[:, 1].sum() < sta.counts[:, 0].sum()  # the filter rejects some
    st_r = obs_grid_ref(rep(T0), REAL, 6, oi.height_level_new, 128, 256)[2]
    assert sta.grid_stats.dtype == np.int64 and sta.grid_stats.tolist() == st_r.tolist()
    assert sta.grid_stats[3] == sta.counts[:, 0].sum()
    on = (Hb != 0).reshape(-1).cpu().numpy()
    idx = np.flatnonzero(on)
    a, b = ya.reshape(-1).cpu().numpy(), yb.reshape(-1).cpu().numpy()
    check(f"StationObs {obs_type} yo' off the accepted cells, not bitwise",
          np.count_nonzero(a[~on].view(np.uint32) != b[~on].view(np.uint32)), 0, "==")
    _check_yo(f"StationObs {obs_type}", a[idx], b[idx], _zt_channels(idx, 7, 128 * 256))


def test_station_obs_free_run_cycle_and_resume(tmp_path, ctx):
    """Two cycles of CyclicDA(da_mode='free_run') fed by StationObs, then a resumed third; ReportMaskObs delivers the
    mask of the same reports for the same driver."""
    from vaevar import config as C
    from vaevar.cycle import CyclicDA, ReportMaskObs, StationObs
    from vaevar.engine import LGUnet
    from vaevar.problem import ObsInterpolater, make_problem

    oi = ObsInterpolater(13, 7)
    p = make_problem(nch=69, Hs=128, Ws=256, T=1, seed=43)
    rep = _reports(1)
    fc = LGUnet(C.FLOW, 1, 1).load_synthetic()  # the flow network stands in as the forecast model
    obs = StationObs(fc.ctx, _truth69, rep, p["R"], oi.interp, oi, "real", filter_coeff=30.0)
    stats = []
    cyc = CyclicDA(fc, obs, T0, T0 + 2 * H6, Nit=1, name="sta", da_mode="free_run", out_dir=str(tmp_path), xb0=p["xb"])
    cyc.run_assimilation(log=lambda t, res: stats.append((obs.grid_stats.copy(), obs.counts.copy())))
    assert len(stats) == 2 and cyc.current_time == T0 + 2 * H6
    for k, (gs, cnt) in enumerate(stats):
        st_r = obs_grid_ref(rep(T0 + k * H6), REAL, 1, oi.height_level_new, 128, 256)[2]
        assert gs.tolist() == st_r.tolist() and cnt[0, 0] == st_r[3] and 0 < cnt[0, 1] < cnt[0, 0]
    assert not np.array_equal(stats[0][0], stats[1][0])
    cyc2 = CyclicDA(fc, obs, T0, T0 + 3 * H6, Nit=1, name="sta", da_mode="free_run", out_dir=str(tmp_path))
    assert cyc2.current_time == T0 + 2 * H6
    check_bitwise("free_run resume xb", cyc2.xb, cyc.xb)
    cyc2.run_assimilation()
    assert np.load(os.path.join(str(tmp_path), "sta", "bg_wrmse.npy")).shape == (3, 69)
    st_r = obs_grid_ref(rep(T0 + 2 * H6), REAL, 1, oi.height_level_new, 128, 256)[2]
    assert obs.grid_stats.tolist() == st_r.tolist()

    mobs = ReportMaskObs(fc.ctx, _truth69, rep, p["R"])
    yo, H, R, gt = mobs.get_obs_info(T0)
    idx, _, st_m = obs_grid_ref(rep(T0), MASK, 1, None, 128, 256)
    check_bitwise("ReportMaskObs H", H, dense(idx, None, (1, 69, 128, 256)))
    assert mobs.grid_stats.tolist() == st_m.tolist() and yo is gt and np.array_equal(gt[0], _truth69(T0))
    cyc3 = CyclicDA(fc, mobs, T0, T0 + H6, Nit=1, name="mask", da_mode="free_run", out_dir=str(tmp_path), xb0=p["xb"])
    cyc3.run_assimilation()
    assert cyc3.current_time == T0 + H6
