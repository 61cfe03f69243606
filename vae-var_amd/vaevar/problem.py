"""Synthetic 3D/4D-Var problems (background, observations, operator, errors).

Shapes follow the reference's `one_step_DA(gt, xb, yo, H, R, 'vae4dvar')`
(`da_4dvar.py:1179-1306`): xb (C,Hs,Ws); yo, H, R (T,C,Hs,Ws).

Observation error R follows `data_reader.__init__` (`da_4dvar.py:106-127`):
obs_var = obs_std^2 * model_std_c^2, with the `modify_tp` rescalings, and
`get_static_info` (`da_4dvar.py:630-634`): R[0] = obs_var,
R[t] = obs_var + q[t-1]; the synthetic case uses q_type = -1 (q = 0).
Observations are the truth (`get_obs_gt`, `da_4dvar.py:445-449`), seen
through a random column mask like the `free_*` obs types
(`da_4dvar.py:277-292`: one lat/lon mask shared by every channel and time).
SURVEY §8 d1 defines the synthetic truth and background.
"""
from __future__ import annotations

import numpy as np

from . import config as C
from .synth import smooth_field, splitmix_uniform


def obs_variance(nch: int, obs_std: float, modify_tp: int, std: np.ndarray) -> np.ndarray:
    v = (np.float32(obs_std) ** 2 * std.astype(np.float32) ** 2).astype(np.float32)
    if nch == 69:
        if modify_tp == 1:
            v[56:] /= 4
        elif modify_tp == 2:
            v[56:] /= 16
            v[2] /= 16
        elif modify_tp == 3:
            v[56:] /= 16
            v[2] /= 16
            v[30:56] /= 16
        elif modify_tp == 4:
            v[56:] /= 16
            v[2] /= 16
            v[17:30] /= 4
    return v


def make_problem(nch: int = 69, Hs: int = 128, Ws: int = 256, T: int = 1, seed: int = 20250620,
                 obs_frac: float = 0.01, obs_std: float = 0.005, modify_tp: int = 2) -> dict:
    mean = np.asarray(C.MODEL_MEAN[:nch], dtype=np.float32)
    std = np.asarray(C.MODEL_STD[:nch], dtype=np.float32)
    std_tr = np.asarray(C.STD_TR[:nch], dtype=np.float32)
    s = smooth_field(seed, (nch, Hs, Ws))
    gt0 = mean[:, None, None] + std[:, None, None] * s
    gts = [gt0]
    for t in range(1, T):
        ds = smooth_field(seed + 1000 + t, (nch, Hs, Ws))
        gts.append(gts[-1] + np.float32(0.05) * std[:, None, None] * ds)
    gt = np.stack(gts, 0).astype(np.float32)
    sp = smooth_field(seed + 1, (nch, Hs, Ws))
    xb = (gt0 + np.float32(0.1) * std[:, None, None] * sp).astype(np.float32)
    u = splitmix_uniform(seed + 2, Hs * Ws).reshape(Hs, Ws)
    col = (u < obs_frac).astype(np.float32)
    H = np.broadcast_to(col, (T, nch, Hs, Ws)).astype(np.float32).copy()
    yo = gt.copy()
    ov = obs_variance(nch, obs_std, modify_tp, std)
    R = np.broadcast_to(ov[None, :, None, None], (T, nch, Hs, Ws)).astype(np.float32).copy()
    return {"gt": gt, "xb": xb, "yo": yo, "H": H, "R": R, "mean": mean, "std": std, "std_tr": std_tr}


def free_amount(obs_type: str) -> int:
    """The number of observed cells of obs_type free_* (get_obs_mask, da_4dvar.py:277-280): nine characters mean
    thousands (free_0015 -> 15000), any other length hundreds of the five digits (free_00150 -> 15000)."""
    if obs_type[:4] != "free":
        raise ValueError(f"obs_type {obs_type!r} is not one of the free_* types")
    if len(obs_type) == 9:
        return int(obs_type[5:9]) * 1000
    return int(obs_type[5:10]) * 100


def r_table(obs_var, q=None, T: int = 1) -> np.ndarray:
    """The static R of get_static_info (da_4dvar.py:630-634) before its broadcast over the grid: the (T, C) fp32 table
    with row 0 = obs_var and row t = obs_var + q[t-1], the sum in fp32 as on the reference's fp32 tensors. q: (T-1, C)
    or more rows, None for zeros (q_type -1). vv_obs_synth broadcasts the table on the device."""
    ov = np.asarray(obs_var, np.float32).reshape(-1)
    tab = np.empty((T, ov.size), np.float32)
    tab[0] = ov
    if T > 1:
        qm = np.zeros((T - 1, ov.size), np.float32) if q is None else np.asarray(q, np.float32).reshape(-1, ov.size)
        if qm.shape[0] < T - 1:
            raise ValueError(f"q has {qm.shape[0]} rows, a window of {T} needs {T - 1}")
        for t in range(1, T):
            tab[t] = ov + qm[t - 1]
    return tab


def init_q_matrix(coeff_dir, q_type: int, da_win: int, nch: int = 69) -> np.ndarray:
    """The model-error variances of init_q_matrix (da_4dvar.py:528-550) before their broadcast over the grid: the
    (da_win - 1, nch) float64 table whose row i-1 belongs to window slot i. q_type 0 (the reference's default): the
    mean over the grid of coeff_dir/q{i}.npy, a (nch, H, W) field as calculate_q / vaevar.calib.ErrorStats.save write
    it (:535-536); q_type -1: zeros (:541); q_type 1: the first da_win - 1 rows of coeff_dir/new_q.npy, a (rows, nch)
    table (:544). Any other q_type raises the reference's NotImplementedError; da_win 1 gives the empty table (:529-530,
    before q_type is looked at)."""
    import os

    if da_win == 1:
        return np.zeros((0, nch), np.float64)
    if q_type == 0:
        rows = []
        for i in range(1, da_win):
            q0 = np.load(os.path.join(coeff_dir, "q%d.npy" % i))
            if q0.ndim != 3 or q0.shape[0] != nch:
                raise ValueError(f"q{i}.npy has shape {q0.shape}, expected ({nch}, H, W)")
            rows.append(np.mean(q0, axis=(1, 2), dtype=np.float64))
        return np.stack(rows, 0)
    if q_type == -1:
        return np.zeros((da_win - 1, nch), np.float64)
    if q_type == 1:
        q = np.asarray(np.load(os.path.join(coeff_dir, "new_q.npy")), np.float64)
        if q.ndim != 2 or q.shape[1] != nch or q.shape[0] < da_win - 1:
            raise ValueError(f"new_q.npy has shape {q.shape}, a window of {da_win} needs ({da_win - 1}+, {nch})")
        return q[:da_win - 1].copy()
    raise NotImplementedError("not implemented q type")


def static_r_table(obs_var, q, T: int) -> np.ndarray:
    """The static R of get_static_info (da_4dvar.py:630-634) as its (T, C) fp32 table, with the reference's rounding:
    row 0 = obs_var, row t = obs_var + q[t-1] summed in the promoted dtype of the fp32 obs_var and q -- float64 for the
    float64 q that np.load of a q%d.npy file gives (:535), float32 for a float32 q -- and rounded to fp32 once, on the
    assignment into the fp32 R. (r_table rounds q to fp32 before the sum.) q: (T-1, C) or more rows, None for zeros;
    vaevar.calib.static_r / engine.r_fill broadcast the table on the device."""
    ov = np.asarray(obs_var, np.float32).reshape(-1)
    tab = np.empty((T, ov.size), np.float32)
    tab[0] = ov
    if T > 1:
        qm = np.zeros((T - 1, ov.size), np.float32) if q is None else np.asarray(q)
        if qm.dtype not in (np.float32, np.float64):
            qm = qm.astype(np.float64)
        qm = qm.reshape(-1, ov.size)
        if qm.shape[0] < T - 1:
            raise ValueError(f"q has {qm.shape[0]} rows, a window of {T} needs {T - 1}")
        for t in range(1, T):
            tab[t] = (ov + qm[t - 1]).astype(np.float32)
    return tab


# ---------------------------------------------------------------------------------------------------------------
# Real-observation operator: obs_interpolater (da_4dvar.py:62-94) maps the 13 model pressure
# levels to dim_out log-spaced levels; the loss compares observations with x_aug (da_4dvar.py:1196-1206) and
# R is interpolated the same way (get_R_matrix_from_gt, da_4dvar.py:729-756).
HEIGHT_LEVEL = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]


class ObsInterpolater:
    """obs_interpolater(dim_in, dim_out) (da_4dvar.py:62-94): interp (dim_out, dim_in) and interp_inv (dim_in,
    dim_out), weights linear in log-pressure, computed in float64 and stored as fp32 like the reference's
    torch.zeros(...) assignment."""

    def __init__(self, dim_in: int = 13, dim_out: int = 40):
        self.dim_in, self.dim_out = dim_in, dim_out
        self.height_level = HEIGHT_LEVEL
        self.height_level_new = np.round(np.exp(np.linspace(3.91202301, 6.90775528, dim_out)))
        self.interp = self._weights(self.height_level_new, self.height_level)
        self.interp_inv = self._weights(self.height_level, self.height_level_new)

    @staticmethod
    def _weights(dst, src) -> np.ndarray:
        w = np.zeros((len(dst), len(src)), np.float32)
        for i, h in enumerate(dst):
            for j, s in enumerate(src):
                if h == s:
                    w[i, j] = 1
                elif j + 1 < len(src) and s < h < src[j + 1]:
                    d = np.log(src[j + 1]) - np.log(s)
                    w[i, j] = (np.log(src[j + 1]) - np.log(h)) / d
                    w[i, j + 1] = (np.log(h) - np.log(s)) / d
        return w


def obs_augment_np(interp: np.ndarray, x: np.ndarray) -> np.ndarray:
    """x_aug for (T, 4 + 5*n_in, H, W) host fields (problem generation only; the closure runs it on the GPU)."""
    n_out, n_in = interp.shape
    parts = [x[:, :4]]
    for i in range(5):
        mat = x[:, 4 + i * n_in:4 + (i + 1) * n_in]
        parts.append(np.einsum("oj,tjhw->tohw", interp, mat, dtype=np.float32))
    return np.concatenate(parts, 1).astype(np.float32)


# quality control of real observations (get_obs_info, da_4dvar.py:764-800; vv_obs_qc): the VV_QC_* flag bits
QC_FILTER, QC_EXEMPT_Z, QC_YO_SIMU, QC_YO_SIMU_Z = 1, 2, 4, 8
OBS_TYPES_REAL = ("real", "real_simu", "real_simuz", "real_simu_nofiltering", "real_simu_nofilteringz")


def qc_flags(obs_type: str) -> int:
    """The vv_obs_qc flags of a real* obs_type by the reference's prefix tests in the reference's order (:778-798):
    the mask by :778 / :783 / else, the yo replacement by :795 / :797."""
    if obs_type[:4] != "real":
        raise ValueError(f"obs_type {obs_type!r} is not one of the real* types {OBS_TYPES_REAL}")
    if obs_type[:22] == "real_simu_nofilteringz" or obs_type[:10] == "real_simuz":
        flags = QC_FILTER | QC_EXEMPT_Z
    elif obs_type[:21] == "real_simu_nofiltering":
        flags = 0
    else:
        flags = QC_FILTER
    if obs_type[:10] == "real_simuz":
        flags |= QC_YO_SIMU_Z
    elif obs_type[:9] == "real_simu":
        flags |= QC_YO_SIMU
    return flags


def qc_threshold(filter_coeff: float, interp, std=None):
    """filter_coeff * torch.Tensor(std_layer_aug) (:779), std_layer_aug as data_reader builds it (:135-138): the first
    four of the float64 std, then the fp32 interp times each 13-level block in numpy. interp None: std itself (the
    identity operator). Returns the fp32 (C_obs,) CPU tensor."""
    import torch

    std = np.asarray(C.MODEL_STD if std is None else std, np.float64)
    if interp is None:
        aug = std
    else:
        interp = np.asarray(interp, np.float32)
        n_in = interp.shape[1]
        parts = [std[:4]]
        for i in range(5):
            parts.append(np.matmul(interp, std[4 + n_in * i:4 + n_in * (i + 1)]))
        aug = np.concatenate(parts, 0)
    return filter_coeff * torch.Tensor(aug)


def make_real_problem(nch: int = 69, Hs: int = 128, Ws: int = 256, T: int = 1, seed: int = 20250622,
                      dim_out: int = 40, obs_frac: float = 0.01, level_frac: float = 0.5, obs_std: float = 0.005,
                      modify_tp: int = 2) -> dict:
    """A synthetic 'real*' observation problem: yo = x_aug(gt) in the 4 + 5*dim_out observation channels, H marks
    observed (channel, lat, lon) entries as get_real_obs does (a random station column mask, each station
    reporting a random subset of the interpolated levels), R = get_R_matrix_from_gt of the static R."""
    assert nch == 69, "the level structure is the 69-channel ERA5 layout"
    p = make_problem(nch=nch, Hs=Hs, Ws=Ws, T=T, seed=seed, obs_frac=obs_frac, obs_std=obs_std, modify_tp=modify_tp)
    oi = ObsInterpolater(13, dim_out)
    ca = 4 + 5 * dim_out
    col = p["H"][0, 0]
    u = splitmix_uniform(seed + 3, ca * Hs * Ws).reshape(ca, Hs, Ws)
    H = np.broadcast_to((col[None] * (u < level_frac)).astype(np.float32), (T, ca, Hs, Ws)).copy()
    p.update(yo=obs_augment_np(oi.interp, p["gt"]), H=H, R=obs_augment_np(oi.interp, p["R"]), interp=oi.interp)
    return p
