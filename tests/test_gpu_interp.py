"""da_mode 'interpolation' on the GPU (da_4dvar.py:968-1061): vv_tri_interp BITWISE against the numpy restatement
(tests/_interp_ref.py, pinned to scipy's griddata by tests/test_interp_host.py), vv_obs_project against an fp64
product under the standard bound of an n-term fp32 sum, one_step_interpolation against the reference's own
one_step_DA run (tests/golden/g18_interpolation.npz (b)), and the CyclicInterpolation driver. Every triangulation
comes from the fixture; nothing here runs scipy or the reference."""
import datetime as dt
import os
import types

import numpy as np
import pytest
import torch

from _interp_ref import (CASES, COLS, GRIDS, background, kernel_cases, obs_project_ref, stored_triangulations,
                         table_from, tri_interp_ref, ulp32, with_prefix)
from conftest import GOLD, check, check_bitwise

pytestmark = pytest.mark.gpu
T0 = dt.datetime(2018, 1, 1, 0)
H6 = dt.timedelta(hours=6)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g18_interpolation.npz"))


@pytest.fixture(scope="module")
def ctx():
    from vaevar.engine import Context

    return Context.get(0)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float32)
    return a.view(np.uint32)


def run_device(ctx, table, yo, H, bg, slack=0):
    """vv_tri_interp on fresh device copies; with `slack` the three fields are views of buffers that many channels
    longer (filled like the background), returned as well."""
    from vaevar.engine import tri_interp

    def up(a, fill):
        full = np.concatenate([a, np.full((slack,) + a.shape[1:], fill, np.float32)]) if slack else a
        d = torch.from_numpy(np.ascontiguousarray(full)).cuda()
        return d, d[:len(a)]

    (yo_f, yo_d), (H_f, H_d), (xa_f, xa_d) = up(yo, 0.0), up(H, 0.0), up(bg, -1.0)
    stats = tri_interp(ctx, torch.from_numpy(table).cuda(), yo_d, H_d, xa_d)
    torch.cuda.synchronize()
    return xa_d.cpu().numpy(), stats.cpu().numpy(), (yo_f, H_f, xa_f)


@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_tri_interp_is_the_restatement_bit_for_bit(gold, ctx, gi):
    yo, H, cases, _ = kernel_cases(gold, gi)
    Hs, Ws = GRIDS[gi]
    table = table_from(cases, Hs, Ws)
    bg = background(H.shape, gi)
    ref, ref_stats, owner, _ = tri_interp_ref(table, yo, H, bg)
    out, stats, _ = run_device(ctx, table, yo, H, bg)
    out2, stats2, _ = run_device(ctx, table, yo, H, bg)
    check_bitwise(f"tri_interp {Hs}x{Ws}: device vs restatement", bits(out), bits(ref))
    check_bitwise(f"tri_interp {Hs}x{Ws}: two calls", bits(out), bits(out2))
    assert stats.tolist() == ref_stats.tolist() == stats2.tolist() and stats[2] > 0 and stats[1] == 0
    kept = bits(out) == bits(bg)
    assert kept[H != 0].all()          # observed cells (and the cell with a mask of 0.5) keep the background
    assert kept[owner < 0].all()       # outside every hull
    assert kept[CASES.index("few")].all()  # <= 10 cells: no rows, untouched
    assert not kept[CASES.index("corners")].all()
    # the NaN vertex: its simplices keep the background, the rest of the channel is written
    c = CASES.index("nan_vertex")
    nan_rows = [t for t, row in enumerate(table) if row[0] == c
                and np.isnan([yo[c, row[1 + 2 * k], row[2 + 2 * k]] for k in range(3)]).any()]
    assert nan_rows and kept[c][np.isin(owner[c], nan_rows)].all() and not kept[c].all()
    assert int((~kept).sum()) == int(stats[2])


def test_tri_interp_skips_bad_rows_and_stays_inside_its_fields(gold, ctx):
    """Bad rows mixed into the good ones of grid 0 (a channel of C, a row of Hs, a neighbour of n_tri, a zero-area
    simplex; each a copy of a large good simplex with one entry changed): skipped and counted, nothing outside the good
    simplices is touched, the rest equals the restatement. All memory involved is in range: the fields are views of
    buffers one channel longer, and that channel must come back unchanged too."""
    yo, H, cases, _ = kernel_cases(gold, 0)
    Hs, Ws = GRIDS[0]
    C = len(H)
    good = table_from(cases, Hs, Ws).astype(np.int64)
    n_good, n_bad = len(good), 4
    n = n_good + n_bad
    big = good[np.argmax(good[:, 11] - good[:, 10])].copy()
    big[0], big[7:10] = 0, -1
    bad = np.stack([big] * n_bad)
    bad[0, 0] = C                               # channel C
    bad[1, 1] = Hs                              # a row index of Hs
    bad[2, 8] = n                               # a neighbour index of n_tri
    bad[3, 3:5], bad[3, 5:7] = bad[3, 1:3], bad[3, 1:3]  # three equal vertices: zero area
    where = np.array([0, n_good // 3, n_good // 2, n_good - 1])  # positions among the good rows
    new_index = np.arange(n_good) + np.searchsorted(where, np.arange(n_good), side="right")
    table = np.zeros((n, COLS), np.int64)
    moved = good.copy()
    nb = moved[:, 7:10]
    moved[:, 7:10] = np.where(nb >= 0, new_index[np.clip(nb, 0, None)], -1)
    table[new_index] = moved
    bad_at = np.setdiff1d(np.arange(n), new_index)
    table[bad_at] = bad
    table = with_prefix(table)
    bg = background(H.shape, 5)
    ref, ref_stats, owner, _ = tri_interp_ref(table, yo, H, bg)
    plain, plain_stats, _, _ = tri_interp_ref(with_prefix(good), yo, H, bg)
    assert ref_stats.tolist() == [n_good, n_bad, plain_stats[2]] and np.array_equal(bits(ref), bits(plain))
    out, stats, (yo_f, H_f, xa_f) = run_device(ctx, table, yo, H, bg, slack=1)
    check_bitwise("tri_interp with bad rows: device vs restatement", bits(out), bits(ref))
    assert stats.tolist() == ref_stats.tolist()
    assert (bits(out) == bits(bg))[owner < 0].all()
    assert bool((xa_f[C] == -1.0).all()) and bool((yo_f[C] == 0).all()) and bool((H_f[C] == 0).all())


def test_tri_interp_without_rows_and_without_stats(ctx):
    from vaevar.engine import tri_interp

    bg = background((2, 9, 70), 1)
    xa = torch.from_numpy(bg).cuda()
    z = torch.zeros_like(xa)
    st = tri_interp(ctx, torch.zeros(0, COLS, dtype=torch.int32, device="cuda"), z, z.clone(), xa)
    assert st.cpu().tolist() == [0, 0, 0]
    assert tri_interp(ctx, torch.zeros(0, COLS, dtype=torch.int32, device="cuda"), z, z.clone(), xa, stats=False) is None
    check_bitwise("tri_interp with an empty table", bits(xa), bits(bg))


@pytest.mark.parametrize("n_in,n_out", [(40, 13), (7, 3)])
@pytest.mark.parametrize("T", [1, 2])
def test_obs_project_against_fp64(ctx, n_in, n_out, T):
    from vaevar.engine import obs_project

    rng = np.random.default_rng(100 * n_in + T)
    Hs, Ws = 33, 47
    W = rng.standard_normal((n_out, n_in)).astype(np.float32)  # dense: the sum must not depend on the level tables
    x_aug = (rng.standard_normal((T, 4 + 5 * n_in, Hs, Ws)) * 10.0 ** rng.uniform(-2, 4, (1, 4 + 5 * n_in, 1, 1)))
    x_aug = x_aug.astype(np.float32)
    dev = obs_project(ctx, torch.from_numpy(W).cuda(), torch.from_numpy(x_aug).cuda()).cpu().numpy()
    ref, bound = obs_project_ref(W, x_aug)
    assert dev.shape == (T, 4 + 5 * n_out, Hs, Ws)
    check_bitwise("obs_project channels 0..3 are copied", bits(dev[:, :4]), bits(x_aug[:, :4]))
    err = np.abs(dev[:, 4:].astype(np.float64) - ref[:, 4:])
    assert (err <= bound[:, 4:]).all()
    check(f"obs_project ({n_in} -> {n_out}, T {T}): largest error / bound", (err / bound[:, 4:]).max(), 1.0, "<=")


def _dense(gold):
    Hs, Ws = (int(v) for v in gold["b_grid"])
    yo = np.zeros(204 * Hs * Ws, np.float32)
    H = np.zeros_like(yo)
    yo[gold["b_idx"]], H[gold["b_idx"]] = gold["b_yo"], 1
    return yo.reshape(1, 204, Hs, Ws), H.reshape(1, 204, Hs, Ws)


def test_one_step_interpolation_against_the_reference_run(gold, ctx):
    """g18(b): the reference's one_step_DA(..., 'interpolation') with obs_type 'real' on 204 channels of 19 x 23.
    xa_aug: bitwise the restatement applied to the device's own augmented background (so within the one-ulp bound of
    the CPU test, hull set exact). xa against the reference's xa, per element: the bound of the 40-term fp32 sum,
    40 * 2^-24 * sum_j |w_j x_j|, plus sum_j |w_j| ulp_j, the one-ulp error of the interpolation stage (ulp_j: one
    fp32 ulp of observation channel j's largest |vertex value|; 0 for a channel without rows) carried through the
    matrix; channels 0..3 are copied, so there the bound is ulp_c alone."""
    from vaevar.engine import obs_augment, obs_project
    from vaevar.interp import one_step_interpolation
    from vaevar.problem import ObsInterpolater

    yo, H = _dense(gold)
    xb = gold["b_xb"]
    chans = [int(c) for c in gold["b_channels"]]
    oi = types.SimpleNamespace(interp=gold["b_interp"], interp_inv=gold["b_interp_inv"])  # the reference's matrices
    mine = ObsInterpolater(13, 40)
    assert np.array_equal(mine.interp, oi.interp) and np.array_equal(mine.interp_inv, oi.interp_inv)
    tri = stored_triangulations(gold, [f"b_c{c}_" for c in chans])
    res = one_step_interpolation(ctx, xb, yo, H, obs_interp=oi, triangulate=tri)
    res2 = one_step_interpolation(ctx, xb, yo, H, obs_interp=oi, triangulate=tri)
    check_bitwise("one_step_interpolation twice", bits(res["xa"]), bits(res2["xa"]))
    assert res["metrics"] is None and set(res) >= {"xa", "xa_aug", "stats", "metrics"}
    # the interpolation stage
    bg_aug = obs_augment(ctx, torch.from_numpy(oi.interp).cuda(), torch.from_numpy(xb).cuda()[None])[0].cpu().numpy()
    cases = [None] * 204
    for c in chans:
        cases[c] = (gold[f"b_c{c}_cells"], gold[f"b_c{c}_simp"], gold[f"b_c{c}_nbr"])
    table = table_from(cases, *xb.shape[1:])
    ref_aug, ref_stats, owner, _ = tri_interp_ref(table, yo[0], H[0], bg_aug)
    xa_aug = res["xa_aug"].cpu().numpy()
    written, ref_written = bits(xa_aug) != bits(bg_aug), bits(ref_aug) != bits(bg_aug)
    assert np.array_equal(written, ref_written) and not written[owner < 0].any()
    assert sorted(set(np.nonzero(written)[0])) == chans
    assert len({bytes(gold[f"b_c{c}_cells"]) for c in chans}) == len(chans) - 1  # two channels share a mask
    ulp = np.zeros(204)
    for c in chans:
        ulp[c] = ulp32(np.abs(yo[0, c][H[0, c] == 1]).max())
    worst = max(float(np.abs(xa_aug[c].astype(np.float64) - ref_aug[c]).max() / ulp[c]) for c in chans)
    check("g18(b) xa_aug vs restatement, ulps of the largest vertex", worst, 1.0, "<=")
    assert res["stats"].cpu().tolist() == ref_stats.tolist()
    # the analysis against the reference's
    Wabs = np.abs(oi.interp_inv.astype(np.float64))
    _, bound = obs_project_ref(oi.interp_inv, xa_aug[None])
    bound = bound[0]
    bound[:4] += ulp[:4, None, None]
    for i in range(5):
        bound[4 + 13 * i:17 + 13 * i] += (Wabs @ ulp[4 + 40 * i:44 + 40 * i])[:, None, None]
    xa = res["xa"].cpu().numpy()
    err = np.abs(xa.astype(np.float64) - gold["b_xa"].astype(np.float64))
    assert (err[:4][gold["b_xa"][:4] == xb[:4]] == 0).all()
    plain = obs_project(ctx, torch.from_numpy(oi.interp_inv).cuda(), torch.from_numpy(bg_aug).cuda()[None])[0]
    assert (bits(xa) != bits(plain)).any(axis=(1, 2)).sum() >= 8  # the interpolated cells reach the model levels
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    print(f"g18(b) xa vs reference: largest error {err.max():.3e}, largest error / bound {ratio.max():.3f}")
    check("g18(b) xa vs the reference's xa: largest error / bound", ratio.max(), 1.0, "<=")


class _StationObs:
    """A SyntheticRealObs-style provider of device tensors: the truth seen at the fixed station cells of g18(c)."""

    def __init__(self, truth, H):
        self.truth = truth
        self.H = torch.from_numpy(H).cuda()

    def get_obs_info(self, t):
        gt = torch.from_numpy(self.truth(t)[None]).cuda()
        return gt * self.H, self.H, None, gt


def _truth(t):
    from vaevar import config as C
    from vaevar.synth import smooth_field

    k = int((t - T0).total_seconds() // 3600)
    mean = np.asarray(C.MODEL_MEAN[:4], np.float32)[:, None, None]
    std = np.asarray(C.MODEL_STD[:4], np.float32)[:, None, None]
    return (mean + std * smooth_field(5200 + k, (4, 32, 64), sigma=3.0)).astype(np.float32)


def test_cyclic_interpolation_two_cycles_and_resume(gold, tmp_path):
    from vaevar import config as C
    from vaevar.cycle import CyclicDA, CyclicInterpolation
    from vaevar.engine import LGUnet
    from vaevar.interp import one_step_interpolation
    from vaevar.synth import smooth_field

    H = np.zeros((1, 4, 32, 64), np.float32)
    for c in range(4):
        cells = gold[f"c_c{c}_cells"].astype(np.int64)
        H[0, c, cells[:, 0], cells[:, 1]] = 1
    tri = stored_triangulations(gold, [f"c_c{c}_" for c in range(3)])
    mean, std = np.asarray(C.MODEL_MEAN[:4], np.float32), np.asarray(C.MODEL_STD[:4], np.float32)
    xb0 = (_truth(T0) + 0.3 * std[:, None, None] * smooth_field(79, (4, 32, 64), sigma=3.0)).astype(np.float32)
    fc = LGUnet(C.TINY_FLOW, 1, 1).load_synthetic()
    obs = _StationObs(_truth, H)
    kw = dict(out_dir=str(tmp_path), mean=mean, std=std, std_tr=np.asarray(C.STD_TR[:4], np.float32), triangulate=tri)

    def run(name, end, **more):
        cyc = CyclicInterpolation(fc, obs, T0, end, name, **kw, **more)
        xas = []
        cyc.run_assimilation(log=lambda t, res: xas.append(res["xa"].clone()))
        return cyc, xas

    cyc, xas = run("interp", T0 + 2 * H6, xb0=xb0)
    assert len(xas) == 2 and cyc.current_time == T0 + 2 * H6
    d = os.path.join(str(tmp_path), "interp")
    for k in ("wrmse", "bias", "mse"):
        for side in ("bg", "ana"):
            v = np.load(os.path.join(d, f"{side}_{k}.npy"))
            assert v.shape == ((2, 4) if k != "mse" else (2,)) and np.isfinite(v).all(), (side, k)
    assert np.load(os.path.join(d, "error_obs.npy")).size == 0  # this mode computes none
    bg, ana = np.load(os.path.join(d, "bg_wrmse.npy")), np.load(os.path.join(d, "ana_wrmse.npy"))
    assert not np.array_equal(bg[0, :3], ana[0, :3]) and bg[0, 3] == ana[0, 3]  # channel 3 has 9 cells: untouched
    # cycle 0 by hand
    yo, Hd, _, gt = obs.get_obs_info(T0)
    hand = one_step_interpolation(fc.ctx, xb0, yo, Hd, triangulate=tri)
    check_bitwise("cycle 0 xa vs one_step_interpolation by hand", bits(xas[0]), bits(hand["xa"]))
    assert int(hand["stats"][2]) > 100 and hand["xa"] is hand["xa_aug"]
    check_bitwise("channel with 9 cells keeps the background", bits(xas[0][3]), bits(xb0[3]))
    # resume: one cycle, then a second driver over the same directory
    first, xa_first = run("resumed", T0 + H6, xb0=xb0)
    check_bitwise("first cycle of the interrupted run", bits(xa_first[0]), bits(xas[0]))
    again, xa_again = run("resumed", T0 + 2 * H6)
    assert len(xa_again) == 1 and again.current_time == T0 + 2 * H6
    check_bitwise("resume: the second cycle's xa", bits(xa_again[0]), bits(xas[1]))
    check_bitwise("resume: the next background", bits(again.xb), bits(cyc.xb))
    for k in ("bg_wrmse", "ana_wrmse", "bg_bias", "ana_bias", "bg_mse", "ana_mse"):
        check_bitwise(f"resume: {k}", np.load(os.path.join(str(tmp_path), "resumed", k + ".npy")),
                      np.load(os.path.join(d, k + ".npy")))
    with pytest.raises(NotImplementedError):
        CyclicDA(fc, obs, T0, T0 + H6, Nit=1, name="x", da_mode="interpolation", out_dir=str(tmp_path))
    with pytest.raises(ValueError):
        CyclicInterpolation(fc, obs, T0, T0 + H6, "y", Nit=3, **kw)


def test_profiler_counts_both_calls_as_misfit(gold, ctx):
    from vaevar.engine import obs_project, tri_interp

    yo, H, cases, _ = kernel_cases(gold, 0)
    table = torch.from_numpy(table_from(cases, *GRIDS[0])).cuda()
    yo_d, H_d, xa = (torch.from_numpy(a).cuda() for a in (yo, H, background(H.shape, 2)))
    x_aug = torch.zeros(1, 4 + 5 * 7, 8, 8, device="cuda")
    W = torch.ones(3, 7, device="cuda")
    ctx.profile_start()
    tri_interp(ctx, table, yo_d, H_d, xa)
    obs_project(ctx, W, x_aug)
    prof = ctx.profile_stop()
    assert prof["misfit"]["launches"] == 2 and prof["misfit"]["bytes"] > 0
    assert sum(v["launches"] for k, v in prof.items() if k != "misfit") == 0
