"""GPU: vv_err_accum / vv_err_finalize / vv_r_fill and what is built on them (calib.ErrorStats, calib.static_r, the
cycle providers' device R) against the restatements of tests/_err_stats_ref.py.

Bounds. The per-cell accumulation and the division are sequences of single IEEE operations in the reference's order:
bitwise. A sum whose order differs from numpy's is held to 2 n 2^-53 times the sum of the magnitudes of its n terms
(_err_stats_ref.sum_bound): the channel totals (n = every difference accumulated so far) and the plane means
(n = H W). The fill only moves table values, or forms vv_obs_augment's sum: bitwise against the broadcast."""
import datetime as dt

import numpy as np
import pytest
import torch

from _err_stats_ref import U, accumulate_ref, calculate_q_ref, diff_sums_ref, moments_ref, sum_bound
from conftest import check, check_bitwise

pytestmark = pytest.mark.gpu


def _ctx():
    from vaevar.engine import Context

    return Context.get(0)


def _fields(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * 3.0


# name: (C, H, W), B, layout. Layouts: "plain" contiguous (B, C, H, W) tensors; "pred138" pred is the first C of 138
# channels; "window" tgt is the slice [:, 1] of a (B, 3, C, H, W) window; "offset1" pred starts one element into its
# buffer (not 16-byte aligned: the element-by-element path at a shape the 16-byte path would take).
# 5 x 7 is odd everywhere; 32 x 64 = 2048 cells is half a workgroup's 4096; 72 x 96 = 6912 and 67 x 71 = 4757 span two
# workgroups per plane, the second one partial, on the 16-byte and the element path.
ACCUM_CASES = {
    "odd_3x5x7_B3": ((3, 5, 7), 3, "plain"),
    "vec_4x32x64_B2": ((4, 32, 64), 2, "plain"),
    "pred138_69x8x12_B1": ((69, 8, 12), 1, "pred138"),
    "pred138_69x8x12_B3": ((69, 8, 12), 3, "pred138"),
    "window_4x32x64_B2": ((4, 32, 64), 2, "window"),
    "offset1_4x32x64_B2": ((4, 32, 64), 2, "offset1"),
    "two_groups_vec_2x72x96_B2": ((2, 72, 96), 2, "plain"),
    "two_groups_tail_2x67x71_B3": ((2, 67, 71), 3, "plain"),
}


def _layout(seed, chw, B, layout):
    """Device (pred, tgt) views of the layout and their host (B, C, H, W) contents."""
    C, H, W = chw
    p, t = _fields(seed, (B, C, H, W)), _fields(seed + 1, (B, C, H, W))
    pd, td = p.cuda(), t.cuda()
    if layout == "pred138":
        full = _fields(seed + 2, (B, 138, H, W)).cuda()
        full[:, :C] = pd
        pd = full[:, :C]
        assert not pd.is_contiguous() or B == 1
    elif layout == "window":
        win = _fields(seed + 2, (B, 3, C, H, W)).cuda()
        win[:, 1] = td
        td = win[:, 1]
    elif layout == "offset1":
        buf = torch.zeros(B * C * H * W + 1, device="cuda")
        buf[1:] = pd.reshape(-1)
        pd = buf[1:].view(B, C, H, W)
        assert pd.data_ptr() % 16 == 4
    return pd, td, p.numpy(), t.numpy()


@pytest.mark.parametrize("case", list(ACCUM_CASES))
def test_err_accum(case):
    """Two calls (the second onto non-zero accumulators): cell bitwise against the numpy loop over the samples in the
    order (call, b); chan within the bound of the fp64 sum and bitwise the same on a second run; each output alone
    gives the bits it has next to the other."""
    from vaevar.engine import err_accum

    chw, B, layout = ACCUM_CASES[case]
    C, H, W = chw
    ctx = _ctx()
    ev = np.zeros(chw, np.float64)
    outs, tgts = [], []
    runs = []
    for run in range(2):
        cell = torch.zeros(chw, device="cuda", dtype=torch.float64)
        chan = torch.zeros(C, device="cuda", dtype=torch.float64)
        cell_only, chan_only = torch.zeros_like(cell), torch.zeros_like(chan)
        for call in range(2):
            pd, td, p, t = _layout(100 * call + 11, chw, B, layout)
            err_accum(ctx, pd, td, cell, chan, C=C)
            err_accum(ctx, pd, td, cell_only, None, C=C)
            err_accum(ctx, pd, td, None, chan_only, C=C)
            if run == 0:
                accumulate_ref(ev, list(p), list(t))
                outs += list(p)
                tgts += list(t)
                if call == 0:
                    check_bitwise(f"{case} cell after one call", cell, ev)
        check_bitwise(f"{case} run {run} cell alone", cell_only, cell)
        check_bitwise(f"{case} run {run} chan alone", chan_only, chan)
        runs.append((cell.cpu().numpy(), chan.cpu().numpy()))
    check_bitwise(f"{case} cell after two calls", runs[0][0], ev)
    check_bitwise(f"{case} cell, second run", runs[1][0], runs[0][0])
    check_bitwise(f"{case} chan, second run", runs[1][1], runs[0][1])
    s, a = diff_sums_ref(outs, tgts)
    n = 2 * B * H * W
    err = float(np.max(np.abs(runs[0][1] - s) / a))
    print(f"{case}: chan error / sum|d| {err:.2e}, bound {sum_bound(n):.2e}")
    check(f"{case} chan vs fp64 sum", err, sum_bound(n), "<=")


def test_err_accum_nan_stays_in_its_cell_and_channel():
    from vaevar.engine import err_accum

    chw, B = (3, 9, 20), 2
    ctx = _ctx()
    pd, td, p, t = _layout(31, chw, B, "plain")
    cell = torch.zeros(chw, device="cuda", dtype=torch.float64)
    chan = torch.zeros(3, device="cuda", dtype=torch.float64)
    err_accum(ctx, pd, td, cell, chan)
    pd2 = pd.clone()
    pd2[1, 1, 4, 7] = float("nan")
    td2 = td.clone()
    td2[0, 2, 8, 19] = float("inf")
    cell2, chan2 = torch.zeros_like(cell), torch.zeros_like(chan)
    err_accum(ctx, pd2, td2, cell2, chan2)
    a, b = cell.cpu().numpy(), cell2.cpu().numpy()
    assert np.isnan(b[1, 4, 7]) and b[2, 8, 19] == np.inf
    same = a.view(np.uint64) == b.view(np.uint64)
    assert int((~same).sum()) == 2 and not same[1, 4, 7] and not same[2, 8, 19]
    ca, cb = chan.cpu().numpy(), chan2.cpu().numpy()
    assert ca.view(np.uint64)[0] == cb.view(np.uint64)[0] and np.isnan(cb[1]) and cb[2] == -np.inf


@pytest.mark.parametrize("chw", [(3, 5, 7), (4, 32, 64), (2, 72, 96), (2, 67, 71)], ids=str)
def test_err_finalize(chw):
    from vaevar.engine import err_finalize

    C, H, W = chw
    ctx = _ctx()
    rng = np.random.default_rng(5)
    ev = rng.random(chw) ** 2 * 10.0 ** rng.integers(-5, 4, (C, 1, 1))
    n = 7
    cell = torch.from_numpy(ev).cuda()
    qf, qt = err_finalize(ctx, cell, n)
    check_bitwise(f"{chw} q_field vs numpy division", qf, ev / n)
    check_bitwise(f"{chw} cell untouched", cell, ev)
    ref = np.mean(ev / n, (1, 2))
    err = float(np.max(np.abs(qt.cpu().numpy() - ref) / ref))
    print(f"{chw}: q_tab relative error {err:.2e}, bound {sum_bound(H * W):.2e}")
    check(f"{chw} q_tab vs np.mean", err, sum_bound(H * W), "<=")
    _, qt_only = err_finalize(ctx, cell, n, q_field=False)
    check_bitwise(f"{chw} q_tab without q_field", qt_only, qt)
    qf_only, none = err_finalize(ctx, cell, n, table=False)
    assert none is None
    check_bitwise(f"{chw} q_field without q_tab", qf_only, qf)
    inplace, qt_in = err_finalize(ctx, cell, n, q_field=cell)
    assert inplace is cell
    check_bitwise(f"{chw} in place q_field", cell, ev / n)
    check_bitwise(f"{chw} in place q_tab", qt_in, qt)


@pytest.mark.parametrize("T, C, Hs, Ws", [(3, 5, 5, 7), (1, 5, 16, 32), (2, 3, 72, 96), (2, 3, 67, 71)])
def test_r_fill_is_the_table_broadcast(T, C, Hs, Ws):
    from vaevar.engine import r_fill

    tab = (np.random.default_rng(9).random((T, C)) * 100).astype(np.float32)
    R = r_fill(_ctx(), tab, Hs, Ws)
    assert tuple(R.shape) == (T, C, Hs, Ws) and R.dtype == torch.float32
    check_bitwise("R vs broadcast", R, np.broadcast_to(tab[:, :, None, None], (T, C, Hs, Ws)))
    # a view one element into a buffer: the element-by-element stores, and nothing written outside the view
    buf = torch.full((T * C * Hs * Ws + 2,), -1.0, device="cuda")
    out = buf[1:-1].view(T, C, Hs, Ws)
    assert r_fill(_ctx(), tab, Hs, Ws, out=out) is out
    check_bitwise("R into an unaligned view", out, R)
    assert float(buf[0]) == -1.0 and float(buf[-1]) == -1.0


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("Hs, Ws", [(5, 7), (16, 32)])
def test_r_fill_with_the_level_operator_is_obs_augment_of_the_broadcast(T, Hs, Ws):
    from vaevar.engine import obs_augment, r_fill
    from vaevar.problem import ObsInterpolater

    oi = ObsInterpolater(13, 40)
    tab = (np.random.default_rng(10 + T).random((T, 69)) * 10.0 ** np.arange(-3, 3).repeat(12)[:69]).astype(np.float32)
    ctx = _ctx()
    interp = torch.from_numpy(oi.interp).cuda()
    dense = torch.from_numpy(np.broadcast_to(tab[:, :, None, None], (T, 69, Hs, Ws)).copy()).cuda()
    ref = obs_augment(ctx, interp, dense)
    R = r_fill(ctx, tab, Hs, Ws, interp=oi.interp)
    assert tuple(R.shape) == (T, 204, Hs, Ws)
    check_bitwise("R vs obs_augment of the broadcast", R, ref)


def test_providers_take_the_device_r():
    """RealObs and SyntheticRealObs given calib.static_r's observation-space device tensor use it as is; it holds the
    bits they derive from the host (T, 69, Hs, Ws) field."""
    from vaevar import config as C
    from vaevar.calib import static_r
    from vaevar.cycle import RealObs, SyntheticRealObs
    from vaevar.problem import ObsInterpolater, obs_variance, static_r_table

    ctx, oi, T, Hs, Ws = _ctx(), ObsInterpolater(13, 40), 2, 6, 8
    ov = obs_variance(69, 0.005, 2, np.asarray(C.MODEL_STD, np.float32))
    q = np.random.default_rng(12).random((T - 1, 69)) * ov
    Rd = static_r(ctx, ov, q, T, Hs, Ws, interp=oi.interp)
    host = np.broadcast_to(static_r_table(ov, q, T)[:, :, None, None], (T, 69, Hs, Ws)).copy()
    H = np.ones((T, 204, Hs, Ws), np.float32)
    for make in (lambda R: SyntheticRealObs(ctx, None, H, R, oi.interp, da_win=T),
                 lambda R: RealObs(ctx, None, None, R, oi.interp, "real_simu", 3.0, da_win=T)):
        a, b = make(Rd), make(host)
        assert a.R.data_ptr() == Rd.data_ptr() and tuple(b.R.shape) == (T, 204, Hs, Ws)
        check_bitwise("provider R, device vs host", a.R, b.R)
    state = static_r(ctx, ov, q, T, Hs, Ws)  # a device R in the state's channels is interpolated like a host one
    check_bitwise("provider R from the device state-space R", SyntheticRealObs(ctx, None, H, state, oi.interp).R, Rd)


def _error_stats_case(cfg, leads, seed):
    """ErrorStats over two add calls against the restatement fed with the engine's own forward_raw outputs."""
    from vaevar.calib import ErrorStats
    from vaevar.engine import LGUnet
    from vaevar.problem import init_q_matrix

    B = 2
    net = LGUnet(cfg, B, 1).load_synthetic()
    C, H, W = net.in_ch, net.H, net.W
    st = ErrorStats(net, leads)
    outs = [[] for _ in range(leads)]
    tgts = [[] for _ in range(leads)]
    for call in range(2):
        win = (_fields(seed + call, (B, leads + 1, C, H, W)) / 3.0).cuda()
        st.add(win)
        z = win[:, 0].contiguous()
        for k in range(1, leads + 1):
            o = net.forward_raw(z)[:, :C].contiguous()
            outs[k - 1] += list(o.cpu().numpy())
            tgts[k - 1] += list(win[:, k].cpu().numpy())
            z = o
    assert st.n == 2 * B
    return st, outs, tgts, (C, H, W), init_q_matrix


def _check_stats(tag, st, outs, tgts, chw, leads):
    C, H, W = chw
    qf, qt = st.q_fields().cpu().numpy(), st.q_table().cpu().numpy()
    mean, std = st.moments()
    assert qf.shape == (leads, C, H, W) and qt.shape == (leads, C) and mean.shape == std.shape == (leads, C)
    N = st.n * H * W
    for k in range(leads):
        ev = accumulate_ref(np.zeros(chw, np.float64), outs[k], tgts[k])
        ref = calculate_q_ref(outs[k], tgts[k])
        assert np.array_equal(ref, ev / st.n)
        check_bitwise(f"{tag} lead {k + 1} q field", qf[k], ref)
        rt = np.mean(ref, (1, 2))
        check(f"{tag} lead {k + 1} q table", np.max(np.abs(qt[k] - rt) / rt), sum_bound(H * W), "<=")
        s, a = diff_sums_ref(outs[k], tgts[k])
        m_ref, v_ref = moments_ref(ev, s, st.n)
        # mean = chan / N: the channel total's bound over N, plus the two divisions' roundings
        d_mean = sum_bound(N) * a / N + 2 * U * np.abs(m_ref)
        check(f"{tag} lead {k + 1} error mean", np.max(np.abs(mean[k] - m_ref) / d_mean), 1.0, "<=")
        # std^2 = m2 - mean^2 with m2 = sum(cell / n) / (H W) against sum(cell) / N: H W non-negative terms in two
        # orders, each divided once more or less (4 roundings); the mean's bound enters through mean^2; the
        # subtraction, the square root and squaring it back round four times more
        m2 = v_ref + m_ref * m_ref
        d_var = (sum_bound(H * W) + 4 * U) * m2 + (2 * np.abs(m_ref) + d_mean) * d_mean + 4 * U * (m2 + m_ref * m_ref)
        check(f"{tag} lead {k + 1} error variance", np.max(np.abs(std[k] ** 2 - v_ref) / d_var), 1.0, "<=")
    return qt


def test_error_stats_flow_two_leads(tmp_path):
    from vaevar import config as C

    st, outs, tgts, chw, init_q_matrix = _error_stats_case(C.TINY_FLOW, 2, 300)
    qt = _check_stats("tiny flow", st, outs, tgts, chw, 2)
    st.save(str(tmp_path / "coeff"))
    q1 = np.load(str(tmp_path / "coeff" / "q1.npy"))
    assert q1.dtype == np.float64 and q1.shape == chw
    tab = init_q_matrix(str(tmp_path / "coeff"), 0, 3, chw[0])
    check("saved files through init_q_matrix", np.max(np.abs(tab - qt) / qt), sum_bound(chw[1] * chw[2]), "<=")


def test_error_stats_lgunet1_one_lead():
    from vaevar import config as C
    from vaevar.calib import calculate_q
    from vaevar.engine import LGUnet

    st, outs, tgts, chw, _ = _error_stats_case(C.TINY_FCST, 1, 400)
    _check_stats("tiny fcst", st, outs, tgts, chw, 1)
    # calculate_q is ErrorStats with one lead: the same windows give the same field
    wins = [(_fields(400 + call, (2, 2) + chw) / 3.0).numpy() for call in range(2)]
    q = calculate_q(st.model, wins)
    assert q.dtype == np.float64
    check_bitwise("calculate_q vs ErrorStats", q, st.q_fields()[0])
    with pytest.raises(ValueError, match="channels"):
        from vaevar.calib import ErrorStats

        ErrorStats(LGUnet(C.TINY, 1, 1), 1, C=5)


T0 = dt.datetime(2018, 1, 1, 0)


def _truth(t):
    from vaevar import config as C
    from vaevar.synth import smooth_field

    k = int((t - T0).total_seconds() // 3600)
    mean = np.asarray(C.MODEL_MEAN[:4], np.float32)[:, None, None]
    std = np.asarray(C.MODEL_STD[:4], np.float32)[:, None, None]
    return (mean + std * smooth_field(5000 + k, (4, 32, 64), sigma=3.0)).astype(np.float32)


def test_two_cycles_with_device_r_equal_host_r(tmp_path):
    """Two cycles of the tiny 4D-Var (T = 2) with R = obs_var + q built on the device by calib.static_r, q from
    ErrorStats over the flow stand-in, against the same R bits uploaded from the host: xa and every metric bitwise."""
    from vaevar import config as C
    from vaevar.calib import ErrorStats, static_r
    from vaevar.cycle import CyclicVAE4DVar, SyntheticObs
    from vaevar.engine import LGUnet
    from vaevar.problem import obs_variance, static_r_table
    from vaevar.synth import smooth_field, splitmix_uniform

    mean = np.asarray(C.MODEL_MEAN[:4], np.float32)[:, None, None]
    std = np.asarray(C.MODEL_STD[:4], np.float32)
    dec = LGUnet(C.TINY, 1, 1).load_synthetic()
    fc = LGUnet(C.TINY_FLOW, 1, 1).load_synthetic()
    st = ErrorStats(fc, 1)
    for k in range(2):
        w = np.stack([_truth(T0 + dt.timedelta(hours=6 * k + i)) for i in range(2)], 0)
        st.add(torch.from_numpy(((w - mean) / std[:, None, None])[None].astype(np.float32)).cuda())
    q = st.q_table()
    ov = obs_variance(4, 0.005, 2, std)
    Rd = static_r(dec.ctx, ov, q, 2, 32, 64)
    Rh = Rd.cpu().numpy()
    tab = static_r_table(ov, q.cpu().numpy(), 2)
    assert np.array_equal(Rh, np.broadcast_to(tab[:, :, None, None], Rh.shape))
    assert (tab[1] >= tab[0]).all() and (tab[1] > tab[0]).any()  # q is in R
    H = np.broadcast_to((splitmix_uniform(77, 32 * 64).reshape(32, 64) < 0.1).astype(np.float32), (2, 4, 32, 64)).copy()
    xb0 = (_truth(T0) + 0.1 * std[:, None, None] * smooth_field(78, (4, 32, 64), sigma=3.0)).astype(np.float32)
    res = {}
    for name, R in (("dev", Rd), ("host", Rh)):
        obs = SyntheticObs(_truth, H, R, da_win=2)
        cyc = CyclicVAE4DVar(dec, fc, obs, T0, T0 + dt.timedelta(hours=12), Nit=1, name=name, out_dir=str(tmp_path),
                             xb0=xb0, flow=fc)
        xas = []
        cyc.run_assimilation(log=lambda t, r: xas.append(r["xa"].clone()))
        assert len(xas) == 2
        res[name] = (xas, cyc.metrics_list, cyc.xb.clone())
    for k in range(2):
        check_bitwise(f"cycle {k} xa", res["dev"][0][k], res["host"][0][k])
    check_bitwise("final xb", res["dev"][2], res["host"][2])
    for key in ("bg_wrmse", "ana_wrmse", "bg_bias", "ana_bias"):
        a, b = np.asarray(res["dev"][1][key]), np.asarray(res["host"][1][key])
        assert a.shape == (2, 4) and np.isfinite(a).all()
        check_bitwise(f"metric {key}", a, b)
