"""sc4dvar — the static-B 4D-Var mode of cyclic_4dvar.one_step_DA (da_4dvar.py:1064-1177) on libvaevar.

  BMatrix          init_b_matrix (da_4dvar.py:520-526): the statistics of dataset/bq_info_lr/*.npy
  Sc4dvarProblem   get_static_info (:608-628) + loss / closure (:1071-1107): J(w) = sum(w^2)/2 +
                   obs_coeff * sum_t H (x_t - yo_t)^2 / R / 2 with x_0 = transform(w, xb) (:878-931) and
                   x_t = integrate(x_{t-1}) (detached, :1080); every FLOP in the HIP library (vv_sc4dvar_*)
  one_step_sc4dvar w = 0 (:1116), LBFGS(history_size=10, max_iter=5, strong_wolfe) (:1119), Nit outer steps
                   (:1124-1170), xhat = transform(w, xb) (:1173)
"""
from __future__ import annotations

import ctypes
import os
import time

import numpy as np
import torch

from ._lib import check, lib
from .da import _check_eval, _departure_tables
from .engine import Context, LGUnet, _obs_list_info, _ptr, _stream, integrate
from .lbfgs import LBFGS

KEYS = ("len_scale", "reg_coeff", "std_sur", "vert_eig_value", "vert_eig_vec")


class BMatrix:
    """The B-matrix statistics as float64 arrays (init_b_matrix; len_scale is multiplied by scale_factor)."""

    def __init__(self, len_scale, reg_coeff, std_sur, vert_eig_value, vert_eig_vec, scale_factor: float = 1.0):
        self.len_scale = np.ascontiguousarray(len_scale, np.float64)
        self.reg_coeff = np.ascontiguousarray(reg_coeff, np.float64)
        self.std_sur = np.ascontiguousarray(std_sur, np.float64)
        self.vert_eig_value = np.ascontiguousarray(vert_eig_value, np.float64)
        self.vert_eig_vec = np.ascontiguousarray(vert_eig_vec, np.float64)
        self.scale_factor = float(scale_factor)
        C = self.len_scale.shape[0]
        if (self.reg_coeff.shape[0] != C or self.reg_coeff.shape[1] not in (13, 26) or self.std_sur.shape != (4,)
                or self.vert_eig_value.shape != (5, 13) or self.vert_eig_vec.shape != (5, 13, 13)):
            raise ValueError("B-matrix statistics of unexpected shape")

    @classmethod
    def from_dir(cls, coeff_dir: str, scale_factor: float = 1.0) -> "BMatrix":
        """--coeff_dir (default dataset/bq_info_lr/): one .npy per statistic (loaded without pickle)."""
        return cls(*[np.load(os.path.join(coeff_dir, k + ".npy"), allow_pickle=False) for k in KEYS],
                   scale_factor=scale_factor)

    @classmethod
    def from_npz(cls, path: str, scale_factor: float = 1.0) -> "BMatrix":
        with np.load(path, allow_pickle=False) as z:
            return cls(*[z[k] for k in KEYS], scale_factor=scale_factor)


def _dp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class Sc4dvarProblem:
    """The sc4dvar closure bound to device buffers: prob = dict(xb (69,Hs,Ws), yo/H/R (T,C_obs,Hs,Ws), mean, std);
    flow: the networks_old LGUnet_all forecast model for T > 1; obs_interp: obs_interpolater.interp for 'real*'."""

    def __init__(self, bmat: BMatrix, prob: dict, flow: LGUnet | None = None, obs_coeff: float = 1.0,
                 device: int = 0, obs_interp=None, hpad: int = 112):
        dev = torch.device("cuda", device)

        def t(a):
            if isinstance(a, torch.Tensor):
                return a.to(device=dev, dtype=torch.float32).contiguous()
            return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)

        self.xb, self.yo, self.H, self.R = t(prob["xb"]), t(prob["yo"]), t(prob["H"]), t(prob["R"])
        self.mean, self.std = t(prob["mean"]), t(prob["std"])
        if self.xb.dim() != 3 or self.xb.shape[0] != 69:
            raise ValueError(f"xb must be (69, Hs, Ws), got {tuple(self.xb.shape)}")
        self.C, self.Hs, self.Ws = self.xb.shape
        if self.yo.dim() != 4 or self.yo.shape[-2:] != self.xb.shape[-2:]:
            raise ValueError(f"yo must be (T, C_obs, {self.Hs}, {self.Ws}), got {tuple(self.yo.shape)}")
        if self.H.shape != self.yo.shape or self.R.shape[-2:] != self.yo.shape[-2:] or self.R.shape[0] != self.yo.shape[0]:
            raise ValueError("H must match yo; R must be (T, C_obs, Hs, Ws)")
        self.T = self.yo.shape[0]
        if self.T > 1 and flow is None:
            raise ValueError("a window of T > 1 needs the flow model")
        self.ctx = flow.ctx if flow is not None else Context.get(device)
        self.obs_coeff = float(obs_coeff)
        self.bmat, self.flow = bmat, flow
        if obs_interp is None:
            obs_interp = prob.get("interp")
        self.interp = None if obs_interp is None else t(obs_interp)
        n_out = self.interp.shape[0] if self.interp is not None else 0
        c_obs = 4 + 5 * n_out if n_out else self.C
        if self.yo.shape[1] != c_obs or self.R.shape[1] != c_obs:
            raise ValueError(f"yo / R have {self.yo.shape[1]} / {self.R.shape[1]} channels, expected {c_obs}")
        self.w_shape = (self.C, 128, 256)
        b = bmat
        check(lib.vv_sc4dvar_bind(self.ctx.h, flow.id if flow is not None else -1, self.T, self.C, self.Hs, self.Ws,
                                  _ptr(self.xb), _ptr(self.yo), _ptr(self.H), _ptr(self.R), _ptr(self.mean),
                                  _ptr(self.std), self.obs_coeff,
                                  _ptr(self.interp) if self.interp is not None else None, n_out,
                                  _dp(b.len_scale), _dp(b.reg_coeff), b.reg_coeff.shape[1], _dp(b.std_sur),
                                  _dp(b.vert_eig_value), _dp(b.vert_eig_vec), b.scale_factor, hpad), "sc4dvar_bind")
        self.n_evals = 0

    def obs_list(self, on: bool = True):
        """vv_set_obs_list for the sc4dvar problem: the observation term from a compacted list of the entries with
        H != 0 (a snapshot of the bound yo / H / R, built on the device now); False restores the dense path. Needs
        the real-observation operator (obs_interp)."""
        check(lib.vv_set_obs_list(self.ctx.h, 1, 1 if on else 0), "set_obs_list")

    @property
    def obs_list_info(self) -> dict:
        """vv_get_obs_list: {"enabled", "units", "records", "bytes"} of this problem's observation list."""
        return _obs_list_info(self.ctx, 1)

    def closure(self, w: torch.Tensor, grad: torch.Tensor | None):
        """(J_b, J_o) as Python floats; grad <- dJ/dw if given."""
        jb, jo = ctypes.c_double(), ctypes.c_double()
        check(lib.vv_sc4dvar_closure(self.ctx.h, _ptr(w), _ptr(grad) if grad is not None else None,
                                     ctypes.byref(jb), ctypes.byref(jo), _stream()), "sc4dvar_closure")
        self.n_evals += 1
        return jb.value, jo.value

    def loss_f32(self, jb: float, jo: float) -> float:
        """cal_loss_bg(w) + obs_coeff * cal_loss_obs(xhat) with the reference's fp32 scalar arithmetic."""
        return float(np.float32(jb) + np.float32(np.float32(self.obs_coeff) * np.float32(jo)))

    def transform(self, w: torch.Tensor) -> torch.Tensor:
        """xhat (69,Hs,Ws) = transform(w, xb) (da_4dvar.py:878-931)."""
        out = torch.empty(self.C, self.Hs, self.Ws, device=w.device, dtype=torch.float32)
        check(lib.vv_sc4dvar_transform(self.ctx.h, _ptr(w.contiguous()), _ptr(out), _stream()), "sc4dvar_transform")
        return out

    def window(self, w: torch.Tensor) -> torch.Tensor:
        """x_t (T,69,Hs,Ws) of the control variable w: x_0 = transform(w), x_t = integrate(x_{t-1}) with the flow
        model (:1080). The engine does not expose the closure's own states; these are formed the same way by separate
        calls (vv_sc4dvar_transform, vv_integrate)."""
        out = torch.empty(self.T, self.C, self.Hs, self.Ws, device=w.device, dtype=torch.float32)
        out[0].copy_(self.transform(w))
        for t in range(1, self.T):
            integrate(self.flow, out[t - 1], self.mean, self.std, 1, out=out[t])
        return out


def one_step_sc4dvar(prob: Sc4dvarProblem, nit: int, history_size: int = 10, max_iter: int = 5,
                     log_terms: bool = True, replay=None, gt=None, metrics=None, mask_eval=None, H_old=None,
                     obs_stats: bool = False):
    """cyclic_4dvar.one_step_DA(..., 'sc4dvar') (da_4dvar.py:1114-1177): returns dict(xa, w, J=[(J_b, J_o) per outer
    pass], n_eval, n_iter, seconds). With gt (T,69,Hs,Ws) and a vaevar.metrics.Metrics also metrics=[(wrmse[69],
    bias[69]) per outer pass] of xhat = transform(w) against gt[0] on the device (:1125-1128; bg_* is pass 0, ana_*
    pass Nit, :1158-1163). With mask_eval (Hs,Ws) and H_old (T,C_obs,Hs,Ws) from vaevar.metrics.held_out — the
    problem bound with the reduced mask — the last pass's xhat is verified against the held-out observations
    (:1139-1155, Metrics.obs_error) and returned as error_obs (C_obs,) numpy fp32.
    obs_stats=True adds obs_stats, the (T, C_obs, 10) float64 numpy table of fields.obs_stats against the problem's
    own yo, H, R and operator, with the background window prob.window(0) and the analysis window prob.window(w) (T - 1
    flow steps each, outside n_eval), and with mask_eval / H_old also obs_stats_heldout over H_old * mask_eval."""
    if mask_eval is not None:
        _check_eval(1, metrics, H_old)
    log_metrics = gt is not None and metrics is not None
    w = torch.zeros(prob.w_shape, device=prob.xb.device, dtype=torch.float32)
    opt = LBFGS(prob.ctx, w, lr=1, history_size=history_size, max_iter=max_iter, line_search_fn="strong_wolfe")
    opt.replay = list(replay) if replay is not None else None

    def closure(ww, g):
        jb, jo = prob.closure(ww, g)
        return prob.loss_f32(jb, jo)

    js, ms, err = [], [], None
    n0 = prob.n_evals
    t0 = time.time()
    xb_win = prob.window(w) if obs_stats else None
    for kk in range(nit + 1):
        if log_metrics or (mask_eval is not None and kk == nit):
            xhat = prob.transform(w)  # :1125
            if log_metrics:
                wr, bi = metrics.wrmse_bias(xhat, gt[0])
                ms.append((wr.cpu().numpy(), bi.cpu().numpy()))
            if mask_eval is not None and kk == nit:
                err = metrics.obs_error(xhat, prob.yo[0], H_old[0], mask_eval, prob.interp)
        if log_terms:
            js.append(prob.closure(w, None))  # loss_total / loss_bg / loss_obs of the log line (:1132-1136)
        if kk < nit:
            opt.step(closure)
    xa = prob.transform(w)
    tabs = _departure_tables(prob, xb_win, prob.window(w), mask_eval, H_old) if obs_stats else {}
    torch.cuda.synchronize()
    n_log = (nit + 1) if log_terms else 0
    res = {"xa": xa, "w": w, "J": js, "n_eval": prob.n_evals - n0 - n_log, "n_iter": opt.state["n_iter"],
           "seconds": time.time() - t0}
    if log_metrics:
        res["metrics"] = ms
    if err is not None:
        res["error_obs"] = err.cpu().numpy()
    res.update({k: v.cpu().numpy() for k, v in tabs.items()})
    return res
