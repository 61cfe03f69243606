"""CPU: the ABI of vv_vae_sample / vv_vae_sse / vv_err_sample (exports, version, the argument checks decided before
any device work), the configurations, and the fixture g20 against the oracle chain and the restatements of
tests/_vae_eval_ref.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _vae_eval_ref import U32, chunk, loss_ref, sse_ref, stat_ref, summary_ref
from conftest import GOLD


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_exported_and_versioned():
    from vaevar import _lib

    for name in ("vv_vae_sample", "vv_vae_sse", "vv_err_sample"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert _lib.lib.vv_version() >= 112


def test_configs():
    from vaevar import config as C

    assert C.VAE["encoder"] is C.ENCODER and C.VAE["decoder"] is C.DECODER
    assert C.in_channels(C.ENCODER) == 69 and C.out_channels(C.ENCODER) == 64 == 2 * C.in_channels(C.DECODER)
    assert C.ENCODER["outchans_list"] == [4, 12, 12, 12, 12, 12]
    e, d = C.TINY_VAE["encoder"], C.TINY_VAE["decoder"]
    assert (e["inchans_list"], e["outchans_list"], d["inchans_list"], d["outchans_list"]) == \
        ([4, 13], [4, 12], [2, 6], [4, 13])
    for k in ("img_size", "enc_dim", "embed_dim", "window_size", "enc_depths", "enc_heads", "lg_depths", "lg_heads"):
        assert e[k] == d[k] == C.TINY[k]


# ---------------------------------------------------------------------------------------------------------------
# VV_E_ARG before any device work: the pointers below are host buffers that are never dereferenced
# ---------------------------------------------------------------------------------------------------------------
def _bufs(k):
    keep = [ctypes.create_string_buffer(1 << 12) for _ in range(k)]
    return keep, [ctypes.cast(b, ctypes.c_void_p) for b in keep]


def _rejected(lib, call):
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001  # another message first, so the one below is this call's
    before = _msg(lib)
    assert call() == 1001
    after = _msg(lib)
    assert after and after != before


# B = 1, L = 2, H = 3, W = 4: enc holds 48 floats = 192 bytes, z 24 floats
BAD_SAMPLE = {"null_ctx": dict(ctx=None), "null_enc": dict(enc=None), "no_output": dict(z=None, stat=None),
              "B_0": dict(B=0), "L_0": dict(L=0), "H_0": dict(H=0), "W_negative": dict(W=-2),
              "enc_2^31": dict(B=1, L=1, H=32768, W=32768), "enc_2^31_through_B": dict(B=2 ** 15, L=2 ** 15, H=1, W=1),
              "flag_2": dict(flags=2), "flag_high": dict(flags=1 | 1 << 20), "flag_negative": dict(flags=-1),
              "z_is_enc": dict(z="enc+0"), "z_at_log_var": dict(z="enc+96"), "z_ends_in_enc": dict(z="enc-92"),
              "z_starts_at_last_word": dict(z="enc+188")}


@pytest.mark.parametrize("case", list(BAD_SAMPLE))
def test_vae_sample_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, big, stat) = _bufs(3)
    enc = ctypes.c_void_p(big.value + 1024)  # room on both sides inside the 4 KiB buffer
    z = ctypes.c_void_p(big.value + 2048)
    a = dict(ctx=ctx, enc=enc, B=1, L=2, H=3, W=4, flags=0, z=z, stat=stat)
    a.update(BAD_SAMPLE[case])
    if isinstance(a["z"], str):
        a["z"] = ctypes.c_void_p(enc.value + int(a["z"][3:]))
    _rejected(lib, lambda: lib.vv_vae_sample(a["ctx"], a["enc"], a["B"], a["L"], a["H"], a["W"], 7, 1, a["flags"],
                                             a["z"], a["stat"], None))


BAD_SSE = {"null_ctx": dict(ctx=None), "null_recon": dict(recon=None), "null_x": dict(x=None),
           "null_sse": dict(sse=None), "B_0": dict(B=0), "C_0": dict(C=0), "H_0": dict(H=0), "W_negative": dict(W=-3),
           "recon_stride_short": dict(rs=23), "x_stride_short": dict(xs=0),
           "sample_2^31": dict(C=2, H=32768, W=32768, rs=2 ** 40, xs=2 ** 40),
           "workgroups_2^31": dict(B=2 ** 16, C=2 ** 15, H=1, W=1, rs=2 ** 15, xs=2 ** 15)}


@pytest.mark.parametrize("case", list(BAD_SSE))
def test_vae_sse_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, recon, x, sse) = _bufs(4)
    a = dict(ctx=ctx, recon=recon, rs=24, x=x, xs=24, B=2, C=2, H=3, W=4, sse=sse)
    a.update(BAD_SSE[case])
    _rejected(lib, lambda: lib.vv_vae_sse(a["ctx"], a["recon"], a["rs"], a["x"], a["xs"], a["B"], a["C"], a["H"],
                                          a["W"], a["sse"], None))


BAD_ERR = {"null_ctx": dict(ctx=None), "null_pred": dict(pred=None), "null_tgt": dict(tgt=None),
           "null_err_std": dict(sd=None), "null_out": dict(out=None), "B_0": dict(B=0), "C_0": dict(C=0),
           "Hs_0": dict(Hs=0), "Ws_negative": dict(Ws=-1), "Hn_0": dict(Hn=0), "Wn_0": dict(Wn=0),
           "pred_stride_short": dict(ps=23), "tgt_stride_short": dict(ts=0),
           "sample_2^31": dict(C=2, Hs=32768, Ws=32768, ps=2 ** 40, ts=2 ** 40),
           "output_2^31": dict(Hn=32768, Wn=32768)}


@pytest.mark.parametrize("case", list(BAD_ERR))
def test_err_sample_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, pred, tgt, sd, out) = _bufs(5)
    a = dict(ctx=ctx, pred=pred, ps=24, tgt=tgt, ts=24, B=2, C=2, Hs=3, Ws=4, sd=sd, Hn=2, Wn=3, out=out)
    a.update(BAD_ERR[case])
    _rejected(lib, lambda: lib.vv_err_sample(a["ctx"], a["pred"], a["ps"], a["tgt"], a["ts"], a["B"], a["C"], a["Hs"],
                                             a["Ws"], a["sd"], a["Hn"], a["Wn"], a["out"], None))


# ---------------------------------------------------------------------------------------------------------------
# the fixture g20: the reference's VAE_lr and loss_function on the tiny configuration
# ---------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def g20():
    from vaevar.synth import smooth_field

    g = dict(np.load(os.path.join(GOLD, "g20_vae_eval.npz")))
    g["x"] = smooth_field(int(g["x_seed"]), (1, 17, 32, 64), sigma=2.0)
    return g


def test_g20_shapes_and_sample(g20):
    """The stored z is the reference's eps.mul(std).add_(mu) on the stored encoder output and the fp32 rounding of the
    restated noise stream: recomputed here with torch on the CPU, within one rounding of each of the three steps."""
    from _obs_synth_ref import eps_ref

    assert g20["enc_out"].shape == (1, 16, 32, 64) and g20["z"].shape == (1, 8, 32, 64)
    assert g20["recon"].shape == (1, 17, 32, 64)
    mu, lv = (torch.from_numpy(a.copy()) for a in chunk(g20["enc_out"]))
    eps = torch.from_numpy(eps_ref(int(g20["seed"]), int(g20["draw"]), 0, mu.numel()).astype(np.float32)).view(mu.shape)
    z = eps.mul(torch.exp(0.5 * lv)).add_(mu)
    d = np.abs(z.numpy().astype(np.float64) - g20["z"])
    bound = 4 * U32 * (np.abs(eps.numpy() * np.exp(0.5 * lv.numpy())) + np.abs(g20["z"]))
    assert (d <= bound).all()


def test_g20_oracle_chain(g20):
    """oracle.lgunet_ref.lgunet_forward under the `enc.` / `dec.` prefixes is the reference's encoder and decoder."""
    from oracle.lgunet_ref import lgunet_forward, synth_params
    from vaevar import config as C

    cfg = C.TINY_VAE
    with torch.no_grad():
        enc = lgunet_forward(synth_params(cfg["encoder"], "enc."), cfg["encoder"], torch.from_numpy(g20["x"]), "enc.")
        rec = lgunet_forward(synth_params(cfg["decoder"], "dec."), cfg["decoder"], torch.from_numpy(g20["z"]), "dec.")
    e_enc, e_rec = rel(enc, g20["enc_out"]), rel(rec, g20["recon"])
    print(f"oracle chain vs g20: enc_out rel {e_enc:.2e}, recon rel {e_rec:.2e}")
    assert e_enc < 1e-6 and e_rec < 1e-6


def test_g20_restatement_is_the_reference_loss(g20):
    """sum sse and KLD of tests/_vae_eval_ref.py against the reference's fp32 loss_function outputs: an fp32 sum of n
    terms in any order is within (n - 1) 2^-24 sum|term| of the exact sum, each term carries up to four elementwise
    fp32 roundings, and the stored value one more: (n + 4) 2^-24 sum|term|."""
    sigma = float(g20["sigma"])
    loss, rec, kld = loss_ref(g20["recon"], g20["x"], g20["enc_out"], sigma)
    terms, _ = sse_ref(g20["recon"], g20["x"])
    n = terms.size
    b_rec = (n + 4) * U32 * float(terms.astype(np.float64).sum())
    stat, mag, abst = stat_ref(g20["enc_out"])
    nk = g20["z"].size
    b_kld = (nk + 4) * U32 * 0.5 * float(mag[..., 0].sum())
    print(f"rec {rec:.9e} vs {float(g20['rec']):.9e} (diff {abs(rec - g20['rec']):.2e}, bound {b_rec:.2e}); "
          f"kld {kld:.9e} vs {float(g20['kld']):.9e} (diff {abs(kld - g20['kld']):.2e}, bound {b_kld:.2e})")
    assert abs(rec - float(g20["rec"])) <= b_rec
    assert abs(kld - float(g20["kld"])) <= b_kld
    # loss = MSE + KLD with MSE = rec / (2 sigma^2): the two bounds, scaled, and the fp32 roundings of the result
    b_loss = b_rec / (2 * sigma ** 2) + b_kld + 4 * U32 * (abs(rec) / (2 * sigma ** 2) + abs(kld))
    assert abs(loss - float(g20["loss"])) <= b_loss


def test_summary_is_the_restatement_on_tables():
    """calib.vae_summary (what VAEStats.summary returns from its accumulators) against summary_ref, which averages
    per-sample quantities computed from the fields: they agree to fp64 summation error."""
    from vaevar.calib import vae_summary

    rng = np.random.default_rng(3)
    C, L, H, W, n, sigma = 5, 3, 6, 10, 4, 1.5
    samples = []
    for _ in range(n):
        x = rng.standard_normal((C, H, W)).astype(np.float32)
        e = (0.5 * rng.standard_normal((2 * L, H, W))).astype(np.float32)
        e[2 * L - 1] = 0.0  # log_var = 0 ...
        e[L - 1] = 0.0      # ... and mu = 0: a collapsed unit, KL exactly 0
        samples.append((x, e, x + 0.1 * rng.standard_normal(x.shape).astype(np.float32),
                        x + 0.05 * rng.standard_normal(x.shape).astype(np.float32)))
    sse = sum(sse_ref(r[None], x[None])[1][0] for x, e, r, m in samples)
    sse_m = sum(sse_ref(m[None], x[None])[1][0] for x, e, r, m in samples)
    stat = sum(stat_ref(e[None])[0][0] for x, e, r, m in samples)
    got, ref = vae_summary(sse, sse_m, stat, n, H * W, sigma), summary_ref(samples, sigma)
    assert set(got) == set(ref)
    for k in ref:
        assert np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-13), k
    assert got["active_units"] == L - 1 and got["kl_channel"][L - 1] == 0.0
    assert got["rmse_mean"].max() < got["rmse"].min()
