"""Shared by the departure-statistics tests (vv_obs_stats): the numpy restatement of the table -- the fp32
terms of include/vaevar.h formed element by element, their sums over the observed entries in long double (64-bit
mantissa, pairwise: the error of a sum of n <= 10^7 terms is below 2^-59 of sum|term|, four orders under the bound of
the kernel's fp64 tree) --, the error bounds the tests hold the kernel to, and seeded cases."""
import numpy as np
import torch

from _obs_qc_ref import gt_aug_ref

COUNT, H, OB, OA, OB2, OA2, OAOB, R, JB, JA = range(10)
NSTAT = 10
ANALYSIS_ROWS = (OA, OA2, OAOB, JA)
NAMES = ("count", "h", "ob", "oa", "ob2", "oa2", "oaob", "r", "jb", "ja")
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the restatement needs the 80-bit long double"


def _np32(a):
    return None if a is None else np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a,
                                                       np.float32)


def terms_ref(xb_aug, xa_aug, yo, Hm, Rm):
    """The ten per-entry terms as fp64 arrays (T, C_obs, Hs, Ws), zero where Hm == 0 (junk there is never used), from
    fp32 fields; xb_aug / xa_aug are the operator's outputs. Every fp32 operation rounds on its own (numpy float32);
    the fp64 products of widened fp32 values are exact. xa_aug None: the analysis terms are None."""
    xb_aug, xa_aug, yo, Hm, Rm = (_np32(a) for a in (xb_aug, xa_aug, yo, Hm, Rm))
    obs = Hm != 0
    z32 = np.float32(0)
    h, y, r = np.where(obs, Hm, z32), np.where(obs, yo, z32), np.where(obs, Rm, np.float32(1))
    out = [None] * NSTAT
    out[COUNT] = obs.astype(np.float64)
    out[H] = h.astype(np.float64)
    out[R] = np.where(obs, Rm, z32).astype(np.float64)
    with np.errstate(all="ignore"):
        ds = {}
        for key, x in (("b", xb_aug), ("a", xa_aug)):
            if x is None:
                continue
            d = y - np.where(obs, x, z32)  # one fp32 subtraction
            assert d.dtype == np.float32
            ds[key] = d.astype(np.float64)
            j = (h * (d * d)) / r  # the closure's fp32 term
            assert j.dtype == np.float32
            out[OB if key == "b" else OA] = np.where(obs, ds[key], 0.0)
            out[OB2 if key == "b" else OA2] = np.where(obs, ds[key] * ds[key], 0.0)
            out[JB if key == "b" else JA] = np.where(obs, j.astype(np.float64), 0.0)
        if "a" in ds:
            out[OAOB] = np.where(obs, ds["a"] * ds["b"], 0.0)
    return out


def table_ref(xb_aug, xa_aug, yo, Hm, Rm, terms=None):
    """(table, mag): the (T, C_obs, 10) float64 table of exact sums rounded once, and mag = sum|term| per entry of the
    table (the factor of the kernel's error bound). Rows of a missing analysis are NaN in both. terms: terms_ref of the
    same arguments, when the caller has them."""
    terms = terms_ref(xb_aug, xa_aug, yo, Hm, Rm) if terms is None else terms
    T, Ca = terms[COUNT].shape[:2]
    tab = np.full((T, Ca, NSTAT), np.nan)
    mag = np.full((T, Ca, NSTAT), np.nan)
    with np.errstate(all="ignore"):
        for i, t in enumerate(terms):
            if t is None:
                continue
            t = t.reshape(T, Ca, -1).astype(LD)
            tab[:, :, i] = t.sum(-1).astype(np.float64)
            mag[:, :, i] = np.abs(t).sum(-1).astype(np.float64)
    return tab, mag


def tree_bound(n_cells: int, mag):
    """|S - exact| <= 2 n 2^-53 sum|term| for the fixed tree over the n = Hs*Ws cells of a plane (include/vaevar.h)."""
    return 2.0 * n_cells * 2.0 ** -53 * mag


def operator_bound(xb_aug, xa_aug, yo, Hm, Rm, n_cells: int, terms=None, mag=None):
    """The bound on |table(kernel) - table(pure-CPU restatement)| with a level operator, (T, C_obs, 10): the kernel's
    x_aug differs from F.linear's by at most e_c = 1e-6 max|x_aug_c| per channel (the bound vv_obs_augment
    is held to), so a departure moves by at most delta = e_c + 2^-23 max|d| (the two fp32 subtractions round on their own).
    Propagated through each term over the observed entries, plus the tree bound:
      OB, OA      N delta                           OB2, OA2   sum delta (2|d| + delta)
      OAOB        sum delta (|d_a| + |d_b| + delta) JB, JA     sum (h / r) delta (2|d| + delta) + 2^-21 sum term
    (the fp32 term h d^2 / r carries three roundings on each side). COUNT, H and R do not see the operator. terms, mag:
    terms_ref / table_ref of the same arguments, when the caller has them."""
    terms = terms_ref(xb_aug, xa_aug, yo, Hm, Rm) if terms is None else terms
    xb_aug, xa_aug, Hm, Rm = (_np32(a) for a in (xb_aug, xa_aug, Hm, Rm))
    T, Ca = Hm.shape[:2]
    obs = (Hm != 0).reshape(T, Ca, -1)
    n = obs.sum(-1).astype(np.float64)
    hr = np.where(obs, Hm.reshape(T, Ca, -1).astype(np.float64) / np.where(obs, Rm.reshape(T, Ca, -1), 1.0), 0.0)
    out = np.zeros((T, Ca, NSTAT))
    absd = {}
    for key, x, i1, i2, ij in (("b", xb_aug, OB, OB2, JB), ("a", xa_aug, OA, OA2, JA)):
        if x is None:
            continue
        e = 1e-6 * np.abs(x.astype(np.float64)).max((0, 2, 3)).reshape(1, Ca, 1)
        d = np.abs(terms[i1].reshape(T, Ca, -1))
        delta = e + 2.0 ** -23 * d.max(-1, keepdims=True)
        absd[key] = (d, delta)
        out[:, :, i1] = n * delta[..., 0]
        out[:, :, i2] = (delta * (2 * d + delta) * obs).sum(-1)
        out[:, :, ij] = (hr * delta * (2 * d + delta)).sum(-1) + 2.0 ** -21 * terms[ij].reshape(T, Ca, -1).sum(-1)
    if "a" in absd:
        (da, dla), (db, dlb) = absd["a"], absd["b"]
        dl = np.maximum(dla, dlb)
        out[:, :, OAOB] = (dl * (da + db + dl) * obs).sum(-1)
    if mag is None:
        _, mag = table_ref(xb_aug, xa_aug, yo, Hm, Rm, terms)
    return out + np.nan_to_num(tree_bound(n_cells, mag))


def make_case(Hs, Ws, T=1, n_out=40, C=69, seed=7100, density=0.02, zero_slice=None):
    """A window with correlated, non-trivial departures. xb = mean_c + std_c N(0,1) (C channels; mean / std the model's
    for C = 69, else 1 + c / 7 and 0.5 + c / 11); the truth is xb + 0.3 std e1, the analysis xb + 0.2 std e1 + 0.05 std
    e2 (so d_a and d_b share e1), yo = Op(truth) + 0.1 s_c e3 in observation space with s_c the channel's spread.
    R = (0.1 s_c)^2 (1 + t / 2), varying per (t, c); H at `density` per (t, c, pixel) with values in {0.5, 1}, 0
    elsewhere. n_out = 0: the identity operator. zero_slice: a time index whose H is all zero. fp32 CPU tensors."""
    from vaevar import config as Cf
    from vaevar.problem import ObsInterpolater

    g = torch.Generator().manual_seed(seed)
    if C == 69:
        mean = torch.tensor(Cf.MODEL_MEAN, dtype=torch.float32)
        std = torch.tensor(Cf.MODEL_STD, dtype=torch.float32)
    else:
        mean = 1.0 + torch.arange(C, dtype=torch.float32) / 7
        std = 0.5 + torch.arange(C, dtype=torch.float32) / 11
    mean, std = mean.reshape(1, -1, 1, 1), std.reshape(1, -1, 1, 1)
    xb = mean + std * torch.randn(T, C, Hs, Ws, generator=g)
    e1, e2 = torch.randn(T, C, Hs, Ws, generator=g), torch.randn(T, C, Hs, Ws, generator=g)
    truth = xb + 0.3 * std * e1
    xa = xb + 0.2 * std * e1 + 0.05 * std * e2
    interp = ObsInterpolater(13, n_out).interp if n_out else None
    ta = gt_aug_ref(truth, interp)
    shape = ta.shape
    s = gt_aug_ref(std.expand(1, C, 1, 1).contiguous(), interp).abs().reshape(1, -1, 1, 1)
    yo = ta + 0.1 * s * torch.randn(shape, generator=g)
    tl = 1.0 + 0.5 * torch.arange(T, dtype=torch.float32).reshape(-1, 1, 1, 1)
    R = ((0.1 * s) ** 2 * tl).expand(shape).contiguous()
    st = torch.rand(shape, generator=g) < density
    H = st.float() * torch.where(torch.rand(shape, generator=g) < 0.2, 0.5, 1.0)
    if zero_slice is not None:
        H[zero_slice] = 0
    return {"xb": xb.contiguous(), "xa": xa.contiguous(), "yo": yo.contiguous(), "H": H, "R": R, "interp": interp,
            "n_out": n_out}
