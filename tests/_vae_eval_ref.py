"""Shared by the VAE-evaluation tests: numpy fp64 restatements, written from the cited lines, of what vv_vae_sample,
vv_vae_sse, vv_err_sample, VAE_lr.loss_function and VAEStats.summary compute, and the bounds the tests hold them to.
Nothing here comes from the device.

  sampling        nf_model/vae.py:78-81     z = eps * exp(0.5 * log_var) + mu
  loss_function   nf_model/vae.py:104-107   MSE = sum((recon - x)^2) / (2 sigma^2), KLD = -0.5 sum(1 + lv - mu^2 - e^lv)
  training sample model/model.py:593-596    err = (pred2 - pred1) / err_std; F.interpolate(err, size)
"""
import numpy as np
import torch

U32 = 2.0 ** -24  # unit roundoffs
U64 = 2.0 ** -53


def chunk(enc):
    """(mu, log_var) of a (B, 2L, H, W) encoder output: chunk(2, dim=1)."""
    L = enc.shape[1] // 2
    return enc[:, :L], enc[:, L:]


def sample_ref(enc, eps):
    """(z64, |eps s64|): the sample in fp64 from the fp32 encoder output and eps (B, L, H, W), and the magnitude of
    the product, which the bound on the fp32 result needs."""
    mu, lv = (a.astype(np.float64) for a in chunk(np.asarray(enc, np.float32)))
    with np.errstate(over="ignore", invalid="ignore"):
        prod = np.asarray(eps, np.float64) * np.exp(0.5 * lv)
        return prod + mu, np.abs(prod)


def z_bound(z64, absprod):
    """|z - z64| <= 1.01 (2^-23 |eps s| + 2^-24 |z|): s within half an fp32 ulp of exp(lv / 2) (relative 2^-24), the
    product's rounding (2^-24 more on |eps s|), the sum's rounding (2^-24 |z|); 1.01 covers the second-order terms and
    the fp64 exponential's own error."""
    return 1.01 * (2.0 * U32 * absprod + U32 * np.abs(z64))


def stat_ref(enc):
    """(stat, mag): stat (B, L, 4) fp64 = the plane sums of t = 1 + lv - mu^2 - e^lv, mu, mu^2, e^lv; mag (B, L, 4)
    the sums of the magnitudes the bounds need: sum(1 + |lv| + mu^2 + e^lv) for t, sum|term| for the others."""
    mu, lv = (a.astype(np.float64) for a in chunk(np.asarray(enc, np.float32)))
    with np.errstate(over="ignore", invalid="ignore"):
        ex = np.exp(lv)
        t = ((1.0 + lv) - mu * mu) - ex
        tm = 1.0 + np.abs(lv) + mu * mu + ex
        stat = np.stack([a.sum((2, 3)) for a in (t, mu, mu * mu, ex)], -1)
        mag = np.stack([a.sum((2, 3)) for a in (tm, np.abs(mu), mu * mu, ex)], -1)
        abst = np.abs(t).sum((2, 3))
    return stat, mag, abst


def stat_bound(n, mag, abst):
    """Per entry of stat: the order of the n-term fp64 sum, 2 n 2^-53 sum|term|, plus the terms' own roundings (three
    operations and an exponential good to a few ulp: 2^-49 of the magnitudes covers 16 ulp)."""
    b = 2.0 ** -49 * mag
    sums = mag.copy()
    sums[..., 0] = abst
    return 2.0 * n * U64 * sums + b


def sse_ref(recon, x):
    """(terms fp32 (B, C, H, W), sums (B, C) fp64): d = recon - x and d * d each rounded to fp32, as torch forms
    (recon_x - x)**2; the sums of the fp32 terms in fp64."""
    d = np.asarray(recon, np.float32) - np.asarray(x, np.float32)
    s = d * d
    assert s.dtype == np.float32
    return s, s.astype(np.float64).sum((2, 3))


def sum_bound(n):
    """Two fp64 sums of the same n non-negative terms in any two orders: relative difference <= 2 n 2^-53."""
    return 2.0 * n * U64


def nearest_ref(n_in, n_out):
    """F.interpolate's nearest source indices n_in -> n_out, read off a ramp (g4's method)."""
    import torch.nn.functional as F

    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return F.interpolate(ramp, (n_out, 1)).view(-1).to(torch.int64).numpy()


def err_sample_ref(pred, tgt, err_std, size):
    """model.py:593-596 word for word on CPU tensors: divide on the input grid, then F.interpolate."""
    import torch.nn.functional as F

    p, t = torch.from_numpy(np.ascontiguousarray(pred, np.float32)), torch.from_numpy(np.ascontiguousarray(tgt, np.float32))
    err = (t - p) / torch.from_numpy(np.asarray(err_std, np.float32)).reshape(1, -1, 1, 1)
    return F.interpolate(err, tuple(size)).numpy()


def loss_ref(recon, x, enc, sigma):
    """(MSE + KLD, MSE 2 sigma^2, KLD) in fp64 from the restatements above."""
    rec = sse_ref(recon, x)[1].sum()
    kld = -0.5 * stat_ref(enc)[0][..., 0].sum()
    return rec / (2.0 * sigma ** 2) + kld, rec, kld


def summary_ref(samples, sigma, threshold=0.01):
    """VAEStats.summary from scratch: samples is a list of (x, enc, recon_sampled, recon_mean), each one sample
    (C, H, W) / (2L, H, W) fp32. Means over the samples of the per-sample quantities, computed without the tables."""
    n = len(samples)
    H, W = samples[0][0].shape[-2:]
    rec = np.mean([sse_ref(r[None], x[None])[1].sum() for x, e, r, m in samples])
    klc = np.mean([-0.5 * stat_ref(e[None])[0][0, :, 0] for x, e, r, m in samples], 0)
    mse = np.mean([sse_ref(r[None], x[None])[0][0].astype(np.float64).mean((1, 2)) for x, e, r, m in samples], 0)
    mse_m = np.mean([sse_ref(m[None], x[None])[0][0].astype(np.float64).mean((1, 2)) for x, e, r, m in samples], 0)
    mu = np.stack([chunk(e[None])[0][0] for x, e, r, m in samples]).astype(np.float64)  # (n, L, H, W)
    lv = np.stack([chunk(e[None])[1][0] for x, e, r, m in samples]).astype(np.float64)
    agg_mean = mu.mean((0, 2, 3))
    agg_var = np.exp(lv).mean((0, 2, 3)) + (mu * mu).mean((0, 2, 3)) - agg_mean ** 2
    kld = klc.sum()
    return {"n": n, "loss": rec / (2.0 * sigma ** 2) + kld, "rec": rec, "kld": kld, "rmse": np.sqrt(mse),
            "rmse_mean": np.sqrt(mse_m), "kl_channel": klc, "active_units": int((klc / (H * W) > threshold).sum()),
            "agg_mean": agg_mean, "agg_var": agg_var}
