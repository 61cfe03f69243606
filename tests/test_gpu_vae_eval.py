"""GPU: vv_vae_sample / vv_vae_sse / vv_err_sample and what is built on them (vaevar.vae.VAE_lr, calib.ErrorSamples,
calib.VAEStats) against the restatements of tests/_vae_eval_ref.py, the oracle networks and the fixtures g20 / g21.

Bounds. z against the fp64 restatement: 1.01 (2^-23 |eps s| + 2^-24 |z|), the half-ulp s, one product and one sum
rounding (_vae_eval_ref.z_bound). A row of stat: 2 n 2^-53 sum|term| for the order of the n-term fp64 sum plus 2^-49 of
the magnitudes for the terms' own roundings (stat_bound). sse sums non-negative terms: relative 2 n 2^-53 (sum_bound);
its terms, the error sample and every copy are single IEEE operations: bitwise. Networks: G1's 5e-6 (tiny) and G3's 1e-5
(full), "rel" = max|a - b| / max|b|."""
import os

import numpy as np
import pytest
import torch

from _vae_eval_ref import (chunk, err_sample_ref, loss_ref, nearest_ref, sample_ref, sse_ref, stat_bound, stat_ref,
                           sum_bound, summary_ref, z_bound)
from conftest import GOLD, check, check_bitwise, note

pytestmark = pytest.mark.gpu

SEED, DRAW = 0x5EEDC0DE12345, 3  # g20's


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _ctx():
    from vaevar.engine import Context

    return Context.get(0)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _eps(n, seed=SEED, draw=DRAW):
    from vaevar.engine import normal_fill

    return normal_fill(_ctx(), n, seed, draw).cpu().numpy()


def _enc(seed, B, L, H, W):
    """mu of a few units, log_var uniform in [-20, 20]."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn((B, L, H, W), generator=g) * 2.0
    lv = (torch.rand((B, L, H, W), generator=g) * 2.0 - 1.0) * 20.0
    return torch.cat([mu, lv], 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# vv_vae_sample
# ---------------------------------------------------------------------------------------------------------------
# 5 x 7 = 35 cells: groups of four eps straddle planes and samples, the element path; 32 x 64 is half a chunk on the
# 16-byte path; 67 x 71 = 4757 and 72 x 96 = 6912 are two chunks, the first with a tail on the element path
SAMPLE_CASES = [(1, 1, 5, 7), (3, 3, 5, 7), (2, 4, 32, 64), (2, 2, 67, 71), (1, 2, 72, 96)]


def _check_sample(tag, enc, z, stat, eps):
    e = enc.numpy()
    B, L2, H, W = e.shape
    z64, absprod = sample_ref(e, eps.reshape(B, L2 // 2, H, W))
    if z is not None:
        err = float(np.max(np.abs(z.cpu().numpy().astype(np.float64) - z64) / z_bound(z64, absprod)))
        check(f"{tag} z vs fp64 / bound", err, 1.0, "<=")
    if stat is not None:
        ref, mag, abst = stat_ref(e)
        err = float(np.max(np.abs(stat.cpu().numpy() - ref) / stat_bound(H * W, mag, abst)))
        check(f"{tag} stat vs fp64 / bound", err, 1.0, "<=")


@pytest.mark.parametrize("shape", SAMPLE_CASES, ids=str)
def test_vae_sample(shape):
    from vaevar.engine import vae_sample

    B, L, H, W = shape
    ctx = _ctx()
    enc = _enc(17 + H, B, L, H, W)
    ed = enc.cuda()
    eps = _eps(B * L * H * W)
    stat = torch.full((B, L, 4), -7.0, device="cuda", dtype=torch.float64)  # overwritten, not added to
    z, _ = vae_sample(ctx, ed, SEED, DRAW, stat=stat)
    _check_sample(str(shape), enc, z, stat, eps)
    check_bitwise(f"{shape} enc untouched", ed, enc)
    z2, stat2 = vae_sample(ctx, ed, SEED, DRAW, z=torch.full_like(z, 3.0), stat=torch.zeros_like(stat))
    assert np.array_equal(_bits(z2), _bits(z)) and np.array_equal(_bits(stat2), _bits(stat))
    z_only, none = vae_sample(ctx, ed, SEED, DRAW)
    assert none is None and np.array_equal(_bits(z_only), _bits(z))
    none, stat_only = vae_sample(ctx, ed, SEED + 1, DRAW + 1, stat=torch.empty_like(stat), want_z=False)
    assert none is None and np.array_equal(_bits(stat_only), _bits(stat))  # stat does not depend on the noise
    zm, stat_m = vae_sample(ctx, ed, SEED, DRAW, mean=True, stat=torch.empty_like(stat))
    assert np.array_equal(_bits(zm), _bits(chunk(enc.numpy())[0])) and np.array_equal(_bits(stat_m), _bits(stat))
    z_other, _ = vae_sample(ctx, ed, SEED, DRAW + 1)
    assert not np.array_equal(_bits(z_other), _bits(z))


def test_vae_sample_element_path_gives_the_16_byte_path_bits():
    """The same (2, 4, 32, 64) values once aligned and once one element into their buffers (enc and z): the element
    path at a shape the 16-byte path would take. Equal bits, and nothing is written outside z."""
    from vaevar.engine import vae_sample

    B, L, H, W = 2, 4, 32, 64
    ctx = _ctx()
    enc = _enc(5, B, L, H, W)
    stat = torch.empty(B, L, 4, device="cuda", dtype=torch.float64)
    z, _ = vae_sample(ctx, enc.cuda(), SEED, DRAW, stat=stat)
    ebuf = torch.zeros(enc.numel() + 1, device="cuda")
    ebuf[1:] = enc.cuda().reshape(-1)
    zbuf = torch.full((B * L * H * W + 2,), -1.0, device="cuda")
    ev, zv = ebuf[1:].view(B, 2 * L, H, W), zbuf[1:-1].view(B, L, H, W)
    assert ev.data_ptr() % 16 == 4 and zv.data_ptr() % 16 == 4
    stat2 = torch.empty_like(stat)
    vae_sample(ctx, ev, SEED, DRAW, z=zv, stat=stat2)
    assert np.array_equal(_bits(zv), _bits(z)) and np.array_equal(_bits(stat2), _bits(stat))
    assert float(zbuf[0]) == -1.0 and float(zbuf[-1]) == -1.0


def test_vae_sample_special_values():
    """log_var = -200: s is below half an ulp of any mu here, z == mu bitwise. log_var = 100 and a NaN each stay in
    their own element of z and their own (b, l) row of stat."""
    from vaevar.engine import vae_sample

    B, L, H, W = 2, 2, 5, 8
    ctx = _ctx()
    enc = _enc(23, B, L, H, W)
    stat = torch.empty(B, L, 4, device="cuda", dtype=torch.float64)
    z, _ = vae_sample(ctx, enc.cuda(), SEED, DRAW, stat=stat)
    e2 = enc.clone()
    e2[0, L + 1, 2, 3] = -200.0          # log_var of (b 0, l 1)
    e2[1, L + 0, 4, 7] = 100.0           # log_var of (b 1, l 0)
    e2[1, 1, 0, 0] = float("nan")        # mu of (b 1, l 1)
    stat2 = torch.empty_like(stat)
    z2, _ = vae_sample(ctx, e2.cuda(), SEED, DRAW, stat=stat2)
    za, zb = z.cpu().numpy(), z2.cpu().numpy()
    assert abs(float(e2[0, 1, 2, 3])) > 1e-3 and _bits(zb)[0, 1, 2, 3] == _bits(e2.numpy())[0, 1, 2, 3]
    eps = _eps(B * L * H * W).reshape(B, L, H, W).astype(np.float64)
    big = eps[1, 0, 4, 7] * np.exp(50.0) + float(e2[1, 0, 4, 7])
    assert np.isfinite(zb[1, 0, 4, 7]) and abs(zb[1, 0, 4, 7] - big) <= 1.01 * 3 * 2.0 ** -24 * abs(big)
    assert np.isnan(zb[1, 1, 0, 0])
    same = _bits(za) == _bits(zb)
    assert int((~same).sum()) == 3 and not (same[0, 1, 2, 3] or same[1, 0, 4, 7] or same[1, 1, 0, 0])
    sa, sb = stat.cpu().numpy(), stat2.cpu().numpy()
    rows = _bits(sa) == _bits(sb)
    assert rows[0, 0].all() and not rows[0, 1, 0] and rows[0, 1, 1] and rows[0, 1, 2]
    assert abs(sb[1, 0, 3] - (sa[1, 0, 3] + np.exp(100.0))) <= 1e-12 * np.exp(100.0) and np.isfinite(sb[1, 0]).all()
    assert rows[1, 0, 1] and rows[1, 0, 2]  # the sums of mu and mu^2 do not see log_var
    assert np.isnan(sb[1, 1, :3]).all() and rows[1, 1, 3]


# ---------------------------------------------------------------------------------------------------------------
# vv_vae_sse
# ---------------------------------------------------------------------------------------------------------------
def _fields(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * 3.0


# the layouts of test_gpu_err_stats.py: "pred138" recon is the first C of 138 channels, "offset1" recon starts one
# element into its buffer; "terms" has one cell per plane, so every output is one term
SSE_CASES = {
    "odd_3x5x7_B3": ((3, 5, 7), 3, "plain"),
    "vec_4x32x64_B2": ((4, 32, 64), 2, "plain"),
    "pred138_69x8x12_B1": ((69, 8, 12), 1, "pred138"),
    "pred138_69x8x12_B3": ((69, 8, 12), 3, "pred138"),
    "offset1_4x32x64_B2": ((4, 32, 64), 2, "offset1"),
    "two_groups_vec_2x72x96_B2": ((2, 72, 96), 2, "plain"),
    "two_groups_tail_2x67x71_B3": ((2, 67, 71), 3, "plain"),
    "terms_257x1x1_B3": ((257, 1, 1), 3, "plain"),
}


def _layout(seed, chw, B, layout):
    C, H, W = chw
    r, x = _fields(seed, (B, C, H, W)), _fields(seed + 1, (B, C, H, W))
    rd, xd = r.cuda(), x.cuda()
    if layout == "pred138":
        full = _fields(seed + 2, (B, 138, H, W)).cuda()
        full[:, :C] = rd
        rd = full[:, :C]
    elif layout == "offset1":
        buf = torch.zeros(B * C * H * W + 1, device="cuda")
        buf[1:] = rd.reshape(-1)
        rd = buf[1:].view(B, C, H, W)
        assert rd.data_ptr() % 16 == 4
    return rd, xd, r.numpy(), x.numpy()


@pytest.mark.parametrize("case", list(SSE_CASES))
def test_vae_sse(case):
    from vaevar.engine import vae_sse

    chw, B, layout = SSE_CASES[case]
    C, H, W = chw
    rd, xd, r, x = _layout(61, chw, B, layout)
    out = torch.full((B, C), -3.0, device="cuda", dtype=torch.float64)
    assert vae_sse(_ctx(), rd, xd, out=out, C=C) is out
    terms, ref = sse_ref(r, x)
    if H * W == 1:
        check_bitwise(f"{case} terms vs numpy fp32", out, terms.astype(np.float64).reshape(B, C))
    err = float(np.max(np.abs(out.cpu().numpy() - ref) / ref))
    check(f"{case} sse vs fp64 sum", err, sum_bound(H * W), "<=")
    again = vae_sse(_ctx(), rd, xd, C=C)
    assert np.array_equal(_bits(again), _bits(out))
    xn = xd.clone()
    xn[B - 1, C - 1, H - 1, W - 1] = float("inf")
    bad = vae_sse(_ctx(), rd, xn, C=C).cpu().numpy()
    same = _bits(bad) == _bits(out)
    assert bad[B - 1, C - 1] == np.inf and int((~same).sum()) == 1


def test_vae_sse_scratch_regrowth():
    """The chunk-sum workspace of a fresh context starts empty: one chunk sum for the 5 x 7 plane, a growth for the
    (2, 2, 67, 71) fields (two chunks a plane, eight sums), then the small call again on the larger buffer. The small
    result does not change by a bit and the large one meets test_vae_sse's bound; the workspace goes with the context."""
    from vaevar.engine import Context, vae_sse

    ctx = Context(0)
    try:
        small, large = _layout(61, (1, 5, 7), 1, "plain"), _layout(61, (2, 67, 71), 2, "plain")
        first = vae_sse(ctx, small[0], small[1], C=1)
        second = vae_sse(ctx, large[0], large[1], C=2)
        third = vae_sse(ctx, small[0], small[1], C=1)
        assert np.array_equal(_bits(third), _bits(first))
        for out, (_, _, r, x) in ((first, small), (second, large)):
            ref = sse_ref(r, x)[1]
            err = float(np.max(np.abs(out.cpu().numpy() - ref) / ref))
            check(f"regrowth {r.shape} sse vs fp64 sum", err, sum_bound(r.shape[2] * r.shape[3]), "<=")
    finally:
        assert ctx.close() == 0


# ---------------------------------------------------------------------------------------------------------------
# vv_err_sample
# ---------------------------------------------------------------------------------------------------------------
# (B, C, Hs, Ws), (Hn, Wn), layout: the identity on the network's 138-channel output; down-sampling with odd sizes;
# the reference's own 721 x 1440 -> 128 x 256; and the two other branches of the nearest rule, 2x and a general
# up-sampling
ERR_CASES = {
    "identity_2x69x8x12": ((2, 69, 8, 12), (8, 12), "pred138"),
    "identity_offset1_2x3x8x12": ((2, 3, 8, 12), (8, 12), "offset1"),
    "down_1x3x13x31_to_5x8": ((1, 3, 13, 31), (5, 8), "plain"),
    "down_1x2x721x1440_to_128x256": ((1, 2, 721, 1440), (128, 256), "plain"),
    "double_2x2x4x6_to_8x12": ((2, 2, 4, 6), (8, 12), "plain"),
    "up_1x2x5x8_to_13x31": ((1, 2, 5, 8), (13, 31), "plain"),
}


@pytest.mark.parametrize("case", list(ERR_CASES))
def test_err_sample(case):
    from vaevar import _lib
    from vaevar.engine import err_sample

    (B, C, Hs, Ws), size, layout = ERR_CASES[case]
    for a, b in ((Hs, size[0]), (Ws, size[1])):  # the rule the kernel restates is torch's
        assert np.array_equal(np.array(_lib.nearest_map(a, b)), nearest_ref(a, b))
    pd, td, p, t = _layout(71, (C, Hs, Ws), B, layout)
    sd = (0.02 + torch.rand(C, generator=torch.Generator().manual_seed(3)) * 0.5).float()
    buf = torch.full((B * C * size[0] * size[1] + 2,), -1.0, device="cuda")
    out = buf[1:-1].view(B, C, *size) if layout == "offset1" else None
    got = err_sample(_ctx(), pd, td, sd.cuda(), size, out=out, C=C)
    assert tuple(got.shape) == (B, C) + size and (out is None or got is out)
    ref = err_sample_ref(p, t, sd.numpy(), size)
    assert np.array_equal(_bits(got), _bits(ref))
    check_bitwise(f"{case} vs (tgt - pred) / err_std, interpolated", got, ref)
    assert float(buf[0]) == -1.0 and float(buf[-1]) == -1.0
    if size == (Hs, Ws):
        check_bitwise(f"{case} default size", err_sample(_ctx(), pd, td, sd.cuda(), C=C), ref)


# ---------------------------------------------------------------------------------------------------------------
# the tiny VAE end to end
# ---------------------------------------------------------------------------------------------------------------
def gold(name):
    return np.load(os.path.join(GOLD, name))


@pytest.fixture(scope="module")
def oracle_params():
    from oracle.lgunet_ref import synth_params
    from vaevar import config as C

    return synth_params(C.TINY_VAE["encoder"], "enc."), synth_params(C.TINY_VAE["decoder"], "dec.")


@pytest.fixture(scope="module")
def vaes():
    from vaevar import config as C
    from vaevar.vae import VAE_lr

    return {B: VAE_lr(C.TINY_VAE, B).load_synthetic() for B in (1, 2)}


def _tiny_x(B):
    from vaevar.synth import smooth_field

    return np.concatenate([smooth_field(2001 + b, (1, 17, 32, 64), sigma=2.0) for b in range(B)], 0)


def _oracle(p, cfg, x, prefix):
    from oracle.lgunet_ref import lgunet_forward

    with torch.no_grad():
        return lgunet_forward(p, cfg, torch.from_numpy(np.ascontiguousarray(x)), prefix).numpy()


@pytest.fixture(scope="module")
def stages(vaes):
    """Per batch size: the GPU's stage outputs on the tiny input, computed once."""
    out = {}
    for B, vae in vaes.items():
        x = _tiny_x(B)
        xd = torch.from_numpy(x).cuda()
        enc = vae.encode(xd)
        z = vae.sampling(enc, SEED, DRAW)
        recon = vae.decoder(z)
        loss = [float(v) for v in vae.loss_function(recon, xd, enc, 2.0)]
        out[B] = dict(x=x, xd=xd, enc_d=enc, z_d=z, recon_d=recon, enc=enc.cpu().numpy(), z=z.cpu().numpy(),
                      recon=recon.cpu().numpy(), loss=loss)
    return out


@pytest.mark.parametrize("B", [1, 2])
def test_tiny_vae_stages(B, vaes, stages, oracle_params):
    """Each stage against the restatement applied to the GPU's own previous stage."""
    from vaevar import config as C

    vae, s = vaes[B], stages[B]
    cfg, (p_enc, p_dec) = C.TINY_VAE, oracle_params
    assert s["enc"].shape == (B, 16, 32, 64) and s["z"].shape == (B, 8, 32, 64) and s["recon"].shape == (B, 17, 32, 64)
    check(f"B={B} encoder vs oracle", rel(s["enc"], _oracle(p_enc, cfg["encoder"], s["x"], "enc.")), 5e-6)
    _check_sample(f"B={B} sampling", torch.from_numpy(s["enc"]), s["z_d"], None, _eps(s["z"].size))
    check(f"B={B} decoder(z_gpu) vs oracle", rel(s["recon"], _oracle(p_dec, cfg["decoder"], s["z"], "dec.")), 5e-6)
    loss, rec, kld = s["loss"]
    l_ref, r_ref, k_ref = loss_ref(s["recon"], s["x"], s["enc"], 2.0)
    n_plane = 32 * 64
    # sum sse: (B, C) table entries each within sum_bound(H W) relative, then a 17 B-term fp64 sum of them
    b_rec = (sum_bound(n_plane) + sum_bound(17 * B)) * r_ref
    _, mag, abst = stat_ref(s["enc"])
    b_kld = 0.5 * (float(stat_bound(n_plane, mag, abst)[..., 0].sum()) + sum_bound(8 * B) * float(abst.sum()))
    check(f"B={B} loss_function rec / bound", abs(rec - r_ref) / b_rec, 1.0, "<=")
    check(f"B={B} loss_function kld / bound", abs(kld - k_ref) / b_kld, 1.0, "<=")
    check(f"B={B} loss_function loss / bound", abs(loss - l_ref) / (b_rec / 8.0 + b_kld + 4 * 2.0 ** -53 * abs(l_ref)),
          1.0, "<=")
    # the public protocol: encoder()'s views, sampling on the pair, forward
    mu, lv = vae.encoder(s["xd"])
    assert mu.data_ptr() + 4 * mu[0].numel() == lv.data_ptr() and mu._base is lv._base
    check_bitwise(f"B={B} encoder views", torch.cat([mu, lv], 1), s["enc"])
    check_bitwise(f"B={B} sampling on the (mu, log_var) pair", vae.sampling((mu, lv), SEED, DRAW), s["z"])
    check_bitwise(f"B={B} posterior mean", vae.sampling((mu, lv), SEED, DRAW, mean=True), chunk(s["enc"])[0])
    recon, mu2, lv2 = vae.forward(s["xd"], SEED, DRAW)
    check_bitwise(f"B={B} forward recon", recon, s["recon"])
    check_bitwise(f"B={B} forward mu", mu2, chunk(s["enc"])[0])
    check_bitwise(f"B={B} decoder_hr on the network grid", vae.decoder_hr(s["z_d"]), s["recon"])


def test_tiny_vae_vs_g20(stages):
    """B = 1 against the reference's own run: the encoder at G1's bound; the loss values carry the encoder's error
    through exp and are recorded without a gate."""
    g, s = gold("g20_vae_eval.npz"), stages[1]
    assert int(g["seed"]) == SEED and int(g["draw"]) == DRAW and float(g["sigma"]) == 2.0
    check("B=1 enc_out vs g20", rel(s["enc"], g["enc_out"]), 5e-6)
    note("B=1 z vs g20 (rel)", rel(s["z"], g["z"]))
    note("B=1 recon vs g20 (rel)", rel(s["recon"], g["recon"]))
    for k, v in zip(("loss", "rec", "kld"), s["loss"]):
        note(f"B=1 {k} vs g20 (rel)", abs(v - float(g[k])) / abs(float(g[k])))


def test_tiny_vae_batch2_image0_is_batch1(stages):
    for k in ("enc", "z", "recon"):
        check(f"B=2 image 0 vs B=1 {k}", rel(stages[2][k][0:1], stages[1][k]), 1e-12, "<=")


def test_full_encoder_g21():
    """The full 69 -> 64 encoder (output groups of 12 channels) against the reference's, G3's form and bound."""
    from vaevar import config as C
    from vaevar.engine import LGUnet
    from vaevar.synth import smooth_field

    g = gold("g21_full_encoder.npz")
    net = LGUnet(C.ENCODER, 1, 1).load_synthetic(prefix="enc.")
    x = torch.from_numpy(smooth_field(int(g["x_seed"]), (1, 69, 128, 256))).cuda()
    o = net.forward_raw(x).cpu().numpy().reshape(-1).astype(np.float64)
    assert o.size == 64 * 128 * 256
    check("G21 full encoder out", rel(o[g["idx_out"]], g["out_sample"]), 1e-5)
    note("G21 full encoder out sumsq (rel)", abs((o * o).sum() - g["out_sumsq"]) / g["out_sumsq"])


# ---------------------------------------------------------------------------------------------------------------
# calib.VAEStats, calib.ErrorSamples, VAE_lr.sample_prior
# ---------------------------------------------------------------------------------------------------------------
def _stats_run(vae, errs):
    from vaevar.calib import VAEStats

    st = VAEStats(vae, 2.0)
    for k, e in enumerate(errs):
        st.add(e, SEED, DRAW + k)
    return st


def test_vae_stats(vaes):
    from vaevar.synth import smooth_field

    vae = vaes[2]
    errs = [torch.from_numpy(smooth_field(2100 + k, (2, 17, 32, 64), sigma=2.0)).cuda() for k in range(2)]
    st = _stats_run(vae, errs)
    assert st.n == 4
    samples = []
    for k, e in enumerate(errs):  # the same stages by hand: the same kernels on the same inputs, hence the same bits
        enc = vae.encode(e)
        rs = vae.dec.forward_raw(vae.sampling(enc, SEED, DRAW + k)).cpu().numpy()
        rm = vae.dec.forward_raw(vae.sampling(enc, 0, 0, mean=True)).cpu().numpy()
        samples += [(e[b].cpu().numpy(), enc[b].cpu().numpy(), rs[b], rm[b]) for b in range(2)]
    got, ref = st.summary(), summary_ref(samples, 2.0)
    assert set(got) == set(ref) and got["n"] == 4 and got["active_units"] == ref["active_units"]
    HW, n = 32 * 64, 4
    # rec, rmse: fp64 sums of at most N = n C H W non-negative terms taken in two orders, 2 N 2^-53 relative, doubled
    # for the divisions and the square root
    tol = 2.0 * sum_bound(n * 17 * HW)
    for k in ("rec", "rmse", "rmse_mean"):
        check(f"summary {k}", np.max(np.abs(got[k] - ref[k]) / np.abs(ref[k])), tol, "<=")
    # the latent tables: per sample and channel stat_bound (the plane sum's order and the terms' roundings), added over
    # the samples, plus the few roundings of the n-term accumulation and the final arithmetic (16 ulp of the magnitudes)
    _, mag, abst = stat_ref(np.stack([s[1] for s in samples]))
    sb = stat_bound(HW, mag, abst).sum(0)  # (L, 4)
    mags = mag.sum(0)
    ulps = 16.0 * 2.0 ** -53
    b_kl = 0.5 * (sb[:, 0] + ulps * mags[:, 0]) / n
    check("summary kl_channel / bound", np.max(np.abs(got["kl_channel"] - ref["kl_channel"]) / b_kl), 1.0, "<=")
    check("summary kld / bound", abs(got["kld"] - ref["kld"]) / b_kl.sum(), 1.0, "<=")
    check("summary loss / bound", abs(got["loss"] - ref["loss"]) / (tol * ref["rec"] / 8.0 + b_kl.sum()), 1.0, "<=")
    b_mean = (sb[:, 1] + ulps * mags[:, 1]) / (n * HW)
    m_abs = mags[:, 1] / (n * HW)
    b_var = (sb[:, 2] + sb[:, 3] + ulps * (mags[:, 2] + mags[:, 3])) / (n * HW) + (2.0 * m_abs + b_mean) * b_mean \
        + ulps * m_abs ** 2
    check("summary agg_mean / bound", np.max(np.abs(got["agg_mean"] - ref["agg_mean"]) / b_mean), 1.0, "<=")
    check("summary agg_var / bound", np.max(np.abs(got["agg_var"] - ref["agg_var"]) / b_var), 1.0, "<=")
    assert st.active_units() == got["active_units"] and st.active_units(1e9) == 0
    again = _stats_run(vae, errs)
    for a, b in ((st.sse, again.sse), (st.sse_mean, again.sse_mean), (st.stat, again.stat)):
        assert np.array_equal(_bits(a), _bits(b))
    with pytest.raises(ValueError, match="no samples"):
        from vaevar.calib import VAEStats

        VAEStats(vae, 2.0).summary()


def test_error_samples_is_rollout_plus_restatement():
    from vaevar import config as C
    from vaevar.calib import ErrorSamples
    from vaevar.engine import LGUnet

    B, lead, size = 2, 2, (20, 45)
    net = LGUnet(C.TINY_FLOW, B, 1).load_synthetic()
    sd = np.asarray([0.2, 0.05, 0.7, 1.3], np.float32)
    win = (_fields(91, (B, lead + 1, 4, 32, 64)) / 3.0).cuda()
    es = ErrorSamples(net, lead, sd, size)
    got = es.make(win[:, 0], win[:, lead])
    z = win[:, 0].contiguous()
    for _ in range(lead):
        z = net.forward_raw(z)[:, :4].contiguous()
    ref = err_sample_ref(z.cpu().numpy(), win[:, lead].cpu().numpy(), sd, size)
    assert tuple(got.shape) == (B, 4) + size
    check_bitwise("ErrorSamples.make vs rollout + restatement", got, ref)
    same = ErrorSamples(net, lead, sd).make(win[:, 0], win[:, lead])
    check_bitwise("ErrorSamples.make on the model grid", same,
                  err_sample_ref(z.cpu().numpy(), win[:, lead].cpu().numpy(), sd, (32, 64)))
    with pytest.raises(ValueError, match="err_std"):
        ErrorSamples(net, lead, sd[:3])


def test_sample_prior(vaes):
    vae = vaes[2]
    sd = np.asarray(np.linspace(0.03, 0.5, 17), np.float32)
    z, y = vae.sample_prior(SEED, 9, sd)
    assert tuple(z.shape) == (2, 8, 32, 64) and tuple(y.shape) == (2, 17, 32, 64)
    assert np.array_equal(_bits(z).reshape(-1), _bits(_eps(z.numel(), SEED, 9)))
    dec = vae.dec.forward_raw(z).cpu().numpy()
    assert np.array_equal(_bits(y), _bits(dec * sd[None, :, None, None]))
    check_bitwise("sample_prior y vs decoder(z) * err_std", y, dec * sd[None, :, None, None])
