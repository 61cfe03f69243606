"""Latitude-weighted WRMSE / Bias on the device (vv_metrics) — the per-channel diagnostics one_step_DA logs at
every outer pass (da_4dvar.py:1256-1262): Metrics.WRMSE (utils/metrics.py:526-545 -> weighted_rmse_torch,
:282-294) and Metrics.Bias (:473-474 -> type_weighted_bias_torch 'all', :65-82, :265-267), both on fields
normalised by the model mean/std and scaled back by the float64 model std. Metrics.verify (vv_verify) is the whole
score family of utils/metrics.py for --forecast_eval: regional WRMSE / Bias, Activity, Anomaly, WACC, MSE, MAE."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import config as C
from ._lib import check, lib
from .engine import Context, _ptr, _stream

Z500 = 11  # channel index the reference prints as "RMSE (z500)" (da_4dvar.py:1254)

# vv_verify's statistic rows (VV_VERIFY_* of include/vaevar.h), named after the reference's Metrics methods
VERIFY_NAMES = ("WRMSE", "NWRMSE", "SWRMSE", "TWRMSE", "Bias", "NBias", "SBias", "TBias", "Channel_MSE", "MSE", "MAE",
                "Activity", "NActivity", "SActivity", "TActivity", "Anomaly", "NAnomaly", "SAnomaly", "TAnomaly",
                "WACC", "NWACC", "SWACC", "TWACC")
CLIM_SCORES = VERIFY_NAMES[11:]  # need a climatology


def _ptr64(t: torch.Tensor):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise ValueError("expected a contiguous float64 device tensor")
    return ctypes.c_void_p(t.data_ptr())


class Metrics:
    def __init__(self, ctx: Context, mean=None, std=None, device: int = 0):
        dev = torch.device("cuda", device)
        mean = C.MODEL_MEAN if mean is None else mean
        std = C.MODEL_STD if std is None else std
        self.ctx = ctx
        self.mean = torch.as_tensor(np.asarray(mean, np.float32)).to(dev)
        self.std = torch.as_tensor(np.asarray(std, np.float32)).to(dev)
        self.scale = torch.as_tensor(np.asarray(std, np.float64)).to(dev)  # data_std = model_std (float64)

    def wrmse_bias(self, pred: torch.Tensor, gt: torch.Tensor):
        """pred, gt (C,H,W) or (B,C,H,W) physical fields on the device -> (wrmse[C], bias[C]) float64 tensors."""
        if pred.dim() == 3:
            pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
        B, Cc, H, W = pred.shape
        if gt.shape != pred.shape or Cc != self.mean.numel():
            raise ValueError(f"shape mismatch {tuple(pred.shape)} {tuple(gt.shape)} C={self.mean.numel()}")
        pred, gt = pred.float().contiguous(), gt.to(pred.device, torch.float32).contiguous()
        w = torch.empty(Cc, device=pred.device, dtype=torch.float64)
        b = torch.empty_like(w)
        check(lib.vv_metrics(self.ctx.h, _ptr(pred), _ptr(gt), _ptr(self.mean), _ptr(self.std), _ptr64(self.scale), B,
                             Cc, H, W, _ptr64(w), _ptr64(b), _stream()), "metrics")
        return w, b

    def verify(self, pred: torch.Tensor, gt: torch.Tensor, clim=None) -> dict:
        """The forecast verification scores of --forecast_eval (vv_verify): pred, gt (C,H,W) or (B,C,H,W) physical
        fields on the device, clim None or the (C,H,W) climatology. Returns {name: float64 (C,) device tensor} keyed
        by the reference's Metrics method names (VERIFY_NAMES; utils/metrics.py on the normalised fields with
        data_std = the float64 model std). MSE and MAE, scalars in the reference, fill every channel's slot with the
        same value. The climatology scores (CLIM_SCORES) are present only with clim. One pass over the fields;
        queued, no synchronisation (the first call at a grid height uploads the latitude weights)."""
        if pred.dim() == 3:
            pred, gt = pred.unsqueeze(0), gt.unsqueeze(0) if gt.dim() == 3 else gt
        if pred.dim() != 4:
            raise ValueError(f"pred must be (C,H,W) or (B,C,H,W), got {tuple(pred.shape)}")
        B, Cc, H, W = pred.shape
        if gt.shape != pred.shape or Cc != self.mean.numel():
            raise ValueError(f"shape mismatch {tuple(pred.shape)} {tuple(gt.shape)} C={self.mean.numel()}")
        pred, gt = pred.float().contiguous(), gt.to(pred.device, torch.float32).contiguous()
        if clim is not None:
            clim = torch.as_tensor(clim).to(pred.device, torch.float32).contiguous()
            if tuple(clim.shape) != (Cc, H, W):
                raise ValueError(f"clim must be {(Cc, H, W)}, got {tuple(clim.shape)}")
        out = torch.empty(len(VERIFY_NAMES), Cc, device=pred.device, dtype=torch.float64)
        check(lib.vv_verify(self.ctx.h, _ptr(pred), _ptr(gt), _ptr(clim) if clim is not None else None,
                            _ptr(self.mean), _ptr(self.std), _ptr64(self.scale), B, Cc, H, W, _ptr64(out), _stream()),
              "verify")
        n = len(VERIFY_NAMES) if clim is not None else VERIFY_NAMES.index(CLIM_SCORES[0])
        return {k: out[i] for i, k in enumerate(VERIFY_NAMES[:n])}

    def mse(self, pred: torch.Tensor, gt: torch.Tensor) -> float:
        """torch.mean((x_norm - gt_norm)**2) over all channels (da_4dvar.py:948, :1131) of (C,H,W) physical fields
        on the device. x_norm - gt_norm = (pred - gt) / std: the difference is formed once in fp32 (vv_axpby), each
        channel's sum of squares is an fp64 device reduction (vv_reduce_batch, 8 channels per round trip) and the
        1 / std^2 weights and the mean are applied to those C scalars; no field leaves the device."""
        Cc = self.mean.numel()
        if pred.dim() != 3 or gt.shape != pred.shape or pred.shape[0] != Cc:
            raise ValueError(f"shape mismatch {tuple(pred.shape)} {tuple(gt.shape)} C={Cc}")
        pred, gt = pred.float().contiguous(), gt.to(pred.device, torch.float32).contiguous()
        d = torch.empty_like(pred)
        self.ctx.axpby(d, pred, 1.0, gt, -1.0)
        ss = []
        for c0 in range(0, Cc, 8):
            ss += self.ctx.reduce_batch([(0, d[c], d[c]) for c in range(c0, min(Cc, c0 + 8))])
        sd = self.std.cpu().numpy().astype(np.float64)  # the fp32 model std the reference normalises with
        return float(np.float32(np.sum(np.asarray(ss) / sd ** 2) / d.numel()))

    def obs_error(self, x: torch.Tensor, yo: torch.Tensor, H: torch.Tensor, mask_eval: torch.Tensor, interp=None,
                  return_sums: bool = False):
        """error_obs of --use_eval (da_4dvar.py:1154-1155, :1285-1286; vv_obs_error): the state x (C,Hs,Ws) against
        the observations yo (C_obs,Hs,Ws) at the pixels mask_eval (Hs,Ws) held out of the assimilation, H (C_obs,
        Hs,Ws) being the ORIGINAL station mask (H_old). interp: None (C_obs = C) or the (n_out, n_in) operator,
        applied inside the kernel. Returns err (C_obs,) fp32 on the device (NaN where nothing was held out); with
        return_sums also the (C_obs, 2) float64 {numerator, denominator} sums. Queued, no synchronisation."""
        if x.dim() != 3 or yo.dim() != 3:
            raise ValueError("obs_error verifies one analysis: x (C,Hs,Ws), yo / H (C_obs,Hs,Ws)")
        dev = x.device

        def t(a):
            return torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()

        x, yo, H, mask_eval = t(x), t(yo), t(H), t(mask_eval)
        Cc, Hs, Ws = x.shape
        n_out = n_in = 0
        if interp is not None:
            interp = t(interp)
            n_out, n_in = interp.shape
            if Cc != 4 + 5 * n_in:
                raise ValueError(f"{Cc} channels, the operator expects {4 + 5 * n_in}")
        c_obs = 4 + 5 * n_out if interp is not None else Cc
        if yo.shape != (c_obs, Hs, Ws) or H.shape != yo.shape or mask_eval.shape != (Hs, Ws):
            raise ValueError(f"yo / H must be ({c_obs}, {Hs}, {Ws}) and mask_eval ({Hs}, {Ws}); got "
                             f"{tuple(yo.shape)} {tuple(H.shape)} {tuple(mask_eval.shape)}")
        err = torch.empty(c_obs, device=dev, dtype=torch.float32)
        sums = torch.empty(c_obs, 2, device=dev, dtype=torch.float64) if return_sums else None
        check(lib.vv_obs_error(self.ctx.h, _ptr(x), _ptr(yo), _ptr(H), _ptr(mask_eval),
                               _ptr(interp) if interp is not None else None, n_out, n_in, Cc, Hs, Ws, _ptr(err),
                               _ptr64(sums) if sums is not None else None, _stream()), "obs_error")
        return (err, sums) if return_sums else err


def held_out(H: torch.Tensor, mask_eval: torch.Tensor):
    """one_step_DA's --use_eval split (da_4dvar.py:934-937): returns (H * (1 - mask_eval), H_old) on H's device, the
    (Hs,Ws) pixel mask broadcast over the leading (T, C_obs) axes. Bind the problem with the first, verify against
    the second (one_step_da / one_step_sc4dvar, H_old=)."""
    if not isinstance(H, torch.Tensor):
        H = torch.as_tensor(np.asarray(H, np.float32))
    if not H.is_cuda:
        H = H.cuda()
    H = H.float()
    m = torch.as_tensor(mask_eval).to(device=H.device, dtype=torch.float32)
    if m.dim() != 2 or tuple(m.shape) != tuple(H.shape[-2:]):
        raise ValueError(f"mask_eval must be {tuple(H.shape[-2:])}, got {tuple(m.shape)}")
    return H * (1 - m), H
