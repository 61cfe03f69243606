"""vv_obs_synth, vv_select_smallest and vv_normal_fill on the GPU (include/vaevar.h; obs_type free_*,
da_4dvar.py:276-292) against the numpy restatement tests/_obs_synth_ref.py: the network and the selection bit for bit,
eps within a bound of the fp64 evaluation of the same formula on the same bits, the fill bit for bit against the
device's own eps, and the cycle with cycle.FreeObs, resumed and uninterrupted."""
import datetime as dt
import os

import numpy as np
import pytest
import torch

from _obs_synth_ref import eps_ref, mask_ref, select_ref
from conftest import check, check_bitwise

pytestmark = pytest.mark.gpu
SEED = 20250620

# the largest |eps - eps_ref| over the vv_normal_fill cases below measured 4.83e-7 on an MI355X (the fp32 logf /
# sinpif / cospif of the build against fp64 on the same bits); the bound is four times that, 1.93e-6, rounded up to a
# power of two, 2^-18 = 3.81e-6, and stays under the cap 2^-16 above which the output would not be this formula
EPS_BOUND = 2.0 ** -18
EPS_CAP = 2.0 ** -16


@pytest.fixture(scope="module")
def ctx():
    from vaevar.engine import Context

    return Context.get(0)


def _bits(a):
    """uint32 words as int64 (exact in check_bitwise's float64): tells -0.0 from +0.0 and keeps NaN payloads."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.int64)


def _differs(t: torch.Tensor, ref: np.ndarray) -> int:
    """The number of 32-bit words of the device tensor t that differ from ref (broadcast to t), counted on the device."""
    r = torch.from_numpy(np.ascontiguousarray(ref, np.float32).view(np.int32)).to(t.device)
    return int((t.view(torch.int32) != r.expand(t.shape)).sum())


def _amounts(hw):
    return [0, 1, max(2, hw // 10), hw // 2, hw - 1, hw]


@pytest.mark.parametrize("hs, ws", [(5, 7), (33, 47), (1, 300), (67, 131)])
def test_mask_is_the_restatement(ctx, hs, ws):
    from vaevar.engine import obs_synth

    hw = hs * ws
    shapes = [(1, 3), (2, 3), (6, 3), (1, 69), (2, 69), (6, 69)]
    for n_obs in _amounts(hw):
        ref, ties = mask_ref(SEED, 11, hs, ws, n_obs)
        assert ref.sum() == n_obs
        for i, (T, C) in enumerate(shapes):
            gt = torch.zeros(T, C, hs, ws, device="cuda")
            fill = float("nan") if i % 2 == 0 else -7.5
            out = tuple(torch.full_like(gt, fill) for _ in range(3))
            rt = np.arange(T * C, dtype=np.float32).reshape(T, C) + 1
            yo, H, R, stats = obs_synth(ctx, gt, n_obs, SEED, 11, r_table=rt, out=out)
            tag = f"{hs}x{ws} n_obs {n_obs} T {T} C {C}"
            check(f"H words differing from the restatement, {tag}", _differs(H, ref), 0, "==")
            check(f"stats[0], {tag}", int(stats[0]), n_obs, "==")
            check(f"stats[1], {tag}", int(stats[1]), ties, "==")
            check(f"yo words differing from gt, {tag}", _differs(yo, np.zeros((), np.float32)), 0, "==")
            check(f"R words differing from the table, {tag}", _differs(R, rt[:, :, None, None]), 0, "==")
            if i == 0:
                _, H2, _, st2 = obs_synth(ctx, gt, n_obs, SEED, 11)
                check(f"second call, {tag}", int((H2.view(torch.int32) != H.view(torch.int32)).sum()), 0, "==")
                check(f"second call stats, {tag}", int((st2 != stats).sum()), 0, "==")


def test_mask_changes_with_draw_and_seed(ctx):
    from vaevar.engine import obs_synth

    gt = torch.zeros(1, 3, 33, 47, device="cuda")
    base = obs_synth(ctx, gt, 500, SEED, 11)[1]
    for name, (seed, draw) in {"draw": (SEED, 12), "seed": (SEED + 1, 11), "seed high word": (SEED + 2 ** 32, 11)}.items():
        H = obs_synth(ctx, gt, 500, seed, draw)[1]
        check(f"another {name}: cells selected", float(H[0, 0].sum()), 500, "==")
        assert int((H != base).sum()) > 0, name
        check(f"another {name}: H words differing from the restatement",
              _differs(H, mask_ref(seed, draw, 33, 47, 500)[0]), 0, "==")


N_SEL = 300007  # 293 wave chunks, 74 workgroups of the tie kernels, the last chunk partly filled


def _key_sets():
    rng = np.random.default_rng(5)
    vals = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xDEADBEEF, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    return {"eight values": vals[rng.integers(0, 8, N_SEL)], "all equal": np.full(N_SEL, 0x12345678, np.uint32),
            "all ffffffff": np.full(N_SEL, 0xFFFFFFFF, np.uint32), "ascending": np.arange(N_SEL, dtype=np.uint32) * 7,
            "descending": (np.arange(N_SEL, dtype=np.uint32) * 7)[::-1].copy()}


@pytest.mark.parametrize("kind", ["eight values", "all equal", "all ffffffff", "ascending", "descending"])
def test_select_smallest_is_the_restatement(ctx, kind):
    from vaevar.engine import select_smallest

    keys = _key_sets()[kind]
    kd = torch.from_numpy(keys.view(np.int32)).cuda()
    for k in (0, 1, N_SEL // 3, N_SEL - 1, N_SEL):
        ref, ties = select_ref(keys, k)
        out = torch.full((N_SEL,), float("nan"), device="cuda")
        mask, stats = select_smallest(ctx, kd, k, out=out)
        check(f"{kind} k {k}: mask words differing from select_ref", _differs(mask, ref), 0, "==")
        check(f"{kind} k {k}: stats[0]", int(stats[0]), k, "==")
        check(f"{kind} k {k}: stats[1]", int(stats[1]), ties, "==")


N_BIG = 1551 * 69 * 2 + 1


@pytest.mark.parametrize("first", [0, 1, 2, 3, 2 ** 33 + 5])
def test_normal_fill_is_the_formula(ctx, first):
    from vaevar.engine import normal_fill

    ref = eps_ref(SEED, 7, first, N_BIG)
    for n in (1, 3, 4, N_BIG):
        out = torch.full((n + 2,), -7.5, device="cuda")
        normal_fill(ctx, n, SEED, 7, first=first, out=out[1:n + 1])
        got = out.cpu().numpy()
        assert got[0] == -7.5 and got[-1] == -7.5  # nothing outside the range
        x = got[1:n + 1].astype(np.float64)
        assert np.isfinite(x).all()
        err = float(np.abs(x - ref[:n]).max())
        print(f"normal_fill first {first} n {n}: max |eps - eps_ref| = {err:.3e}")
        assert EPS_BOUND <= EPS_CAP
        check(f"first {first} n {n}: max |eps - eps_ref|", err, EPS_BOUND)
        check(f"first {first} n {n}: max |eps|", float(np.abs(x).max()), 5.78, "<=")
    # eps(e) depends on e alone: the same elements through another window, and under another draw or seed
    a = normal_fill(ctx, 64, SEED, 7, first=first + 5)
    b = normal_fill(ctx, 100, SEED, 7, first=first)
    check_bitwise(f"first {first}: a shifted window", _bits(a), _bits(b[5:69]))
    assert not torch.equal(normal_fill(ctx, 64, SEED, 8, first=first), b[:64])
    assert not torch.equal(normal_fill(ctx, 64, SEED + 2 ** 32, 7, first=first), b[:64])


def _truth_field(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 30 + 250).astype(np.float32)


@pytest.mark.parametrize("hs, ws", [(33, 47), (1, 300)])  # the scalar and the 16-byte fill
def test_fill_adds_the_device_eps(ctx, hs, ws):
    from vaevar.engine import normal_fill, obs_synth

    T, C = 2, 5
    gt = _truth_field((T, C, hs, ws), 9)
    sd = np.array([0.5, 3.0, 1e-3, 0.0, 1e4], np.float32)
    rt = (np.arange(T * C, dtype=np.float32).reshape(T, C) + 1) * 0.37
    gd = torch.from_numpy(gt).cuda()
    yo, H, R, _ = obs_synth(ctx, gd, 100, SEED, 3, sd=sd, r_table=rt, noise_seed=SEED + 9)
    eps = normal_fill(ctx, gt.size, SEED + 9, 3).cpu().numpy().reshape(gt.shape)
    want = np.float32(gt + np.float32(sd[None, :, None, None] * eps))
    check_bitwise("yo = gt + sd * eps_dev", _bits(yo), _bits(want))
    check("R words differing from the table", _differs(R, rt[:, :, None, None]), 0, "==")
    check("H words differing from the restatement", _differs(H, mask_ref(SEED, 3, hs, ws, 100)[0]), 0, "==")
    # the noise seed moves yo and leaves H alone; by default it is the seed
    yo2, H2, _, _ = obs_synth(ctx, gd, 100, SEED, 3, sd=sd, noise_seed=SEED + 10)
    assert not torch.equal(yo2, yo)
    check_bitwise("H under another noise seed", _bits(H2), _bits(H))
    yo3 = obs_synth(ctx, gd, 100, SEED + 9, 3, sd=sd)[0]
    check_bitwise("noise_seed defaults to seed", _bits(yo3), _bits(yo))
    # in place
    g2 = gd.clone()
    yo4, H4, R4, _ = obs_synth(ctx, g2, 100, SEED, 3, sd=sd, r_table=rt, noise_seed=SEED + 9, out=(g2, None, None))
    assert yo4.data_ptr() == g2.data_ptr()
    check_bitwise("yo in place", _bits(yo4), _bits(yo))
    check_bitwise("H of the in-place call", _bits(H4), _bits(H))
    check_bitwise("R of the in-place call", _bits(R4), _bits(R))


@pytest.mark.parametrize("hs, ws", [(33, 47), (1, 300)])
def test_fill_without_noise_copies_the_words(ctx, hs, ws):
    from vaevar.engine import obs_synth

    gt = _truth_field((2, 3, hs, ws), 10)
    w = gt.view(np.uint32).reshape(-1)
    w[5], w[6], w[7], w[-1] = 0x7FC12345, 0x80000000, 0x00000001, 0xFFC00001  # NaNs, -0.0, a subnormal
    gd = torch.from_numpy(gt).cuda()
    yo, H, R, stats = obs_synth(ctx, gd, 40, SEED, 1, out=(torch.full_like(gd, -7.5), None, None))
    assert R is None
    check_bitwise("yo = gt word for word", _bits(yo).reshape(-1), w.astype(np.int64))
    g2 = gd.clone()
    yo2, H2, _, _ = obs_synth(ctx, g2, 40, SEED, 1, out=(g2, None, None))
    check_bitwise("yo = gt in place", _bits(yo2).reshape(-1), w.astype(np.int64))
    check_bitwise("H of the in-place call", _bits(H2), _bits(H))


def _dir_bytes(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_free_obs_cycle_and_resume(tmp_path):
    """vae4dvar with FreeObs('free_0003') on the 69-channel 128 x 256 models (the grids of the 4-channel tiny models
    hold 2048 cells, fewer than the 3000 of free_0003)."""
    from vaevar import config as C
    from vaevar.cycle import CyclicDA, FreeObs
    from vaevar.engine import LGUnet
    from vaevar.problem import make_problem, obs_variance, r_table
    from vaevar.synth import smooth_field

    T0, H6 = dt.datetime(2018, 1, 1, 0), dt.timedelta(hours=6)
    mean = np.asarray(C.MODEL_MEAN, np.float32)[:, None, None]
    std = np.asarray(C.MODEL_STD, np.float32)[:, None, None]
    fields = {}

    def truth(t):
        k = int((t - T0).total_seconds() // 3600)
        if k not in fields:
            fields[k] = (mean + std * smooth_field(6100 + k, (69, 128, 256))).astype(np.float32)
        return fields[k]

    xb0 = make_problem(nch=69, Hs=128, Ws=256, T=1, seed=8181, obs_frac=0.03)["xb"]
    ov = obs_variance(69, 0.005, 2, std.reshape(-1))
    dec = LGUnet(C.DECODER, 1, 1).load_synthetic()
    fc = LGUnet(C.FLOW, 1, 1).load_synthetic()  # the flow network stands in as the forecast model

    class Keep:
        def __init__(self, obs):
            self.obs, self.H = obs, []

        def get_obs_info(self, t):
            out = self.obs.get_obs_info(t)
            self.H.append(out[1].clone())
            assert self.obs.stats.tolist()[0] == 3000
            return out

    def run(name, end, **kw):
        obs = Keep(FreeObs(dec.ctx, truth, "free_0003", r_table(ov), seed=SEED, **kw))
        assert obs.obs.amount == 3000
        cyc = CyclicDA(fc, obs, T0, end, Nit=1, name=name, decoder=dec, out_dir=str(tmp_path), xb0=xb0)
        xas = []
        cyc.run_assimilation(log=lambda t, res: xas.append(res["xa"].clone()))
        return cyc, obs, xas

    cyc, obs, xas = run("full", T0 + 2 * H6)
    assert len(xas) == 2 and len(obs.H) == 2
    for k, H in enumerate(obs.H):
        assert H.shape == (1, 69, 128, 256)
        check(f"cycle {k}: H.sum() per slot", float(H[0].double().sum()), 69 * 3000, "==")
        draw = FreeObs.draw_number(T0 + k * H6)
        check(f"cycle {k}: H words differing from the restatement",
              _differs(H, mask_ref(SEED, draw, 128, 256, 3000)[0]), 0, "==")
    assert int((obs.H[0] != obs.H[1]).sum()) > 0
    # stopped after cycle 1 and resumed
    run("part", T0 + H6)
    cyc_r, _, xas_r = run("part", T0 + 2 * H6)
    assert len(xas_r) == 1
    check_bitwise("resumed cycle 2 xa", xas_r[0], xas[1])
    full, part = _dir_bytes(os.path.join(str(tmp_path), "full")), _dir_bytes(os.path.join(str(tmp_path), "part"))
    assert list(full) == list(part) and "xb.npy" in full
    for f in full:
        check(f"resumed run: bytes of {f} differing", float(full[f] != part[f]), 0, "==")
    # observation noise
    cyc_n, obs_n, xas_n = run("noise", T0 + H6, noise=True, obs_var=ov)
    check_bitwise("the noise leaves the network alone", _bits(obs_n.H[0]), _bits(obs.H[0]))
    assert not torch.equal(xas_n[0], xas[0])
    for key in ("bg_wrmse", "ana_wrmse", "bg_bias", "ana_bias"):
        w = np.asarray(cyc_n.metrics_list[key])
        assert w.shape == (1, 69) and np.isfinite(w).all(), key
