"""Model-error calibration on the HIP engine: the Q of the 4D-Var window and the static R built from it.

  calculate_q     model/model.py:469-490   stream a data set through the flow model, accumulate the squared one-step
                                           error per grid cell, divide by the sample count -> q1.npy
  ErrorStats                               the same for leads 1 .. L in one pass (q1.npy .. qL.npy: the files
                                           init_q_matrix reads, da_4dvar.py:528-550), plus the per-channel error
                                           moments err_std / stdTr are made of (model/model.py:538-593)
  static_r        da_4dvar.py:630-634      R[0] = obs_var, R[t] = obs_var + q[t-1] as a dense device field
                  da_4dvar.py:729-756      and get_R_matrix_from_gt of it when the level operator is given

The forwards run with the network's batch B (vv_model_forward); the accumulation (vv_err_accum), the division and the
plane means (vv_err_finalize) and the broadcast (vv_r_fill) are HIP kernels; the accumulators stay on the device in
float64 and nothing synchronises until a result is fetched.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .engine import Context, LGUnet, err_accum, err_finalize, r_fill
from .problem import static_r_table


class ErrorStats:
    """Forecast-error statistics of `model` at the leads 1 .. `leads`, in the model's normalised space.

    model: an LGUnet of either arch with in_ch == C and out_ch >= C (the flow network's 138 outputs: the first C are
    the state, as the reference's `[:, :69]`), of batch B. add(window) takes a (B, leads + 1, C, H, W) float32 device
    tensor: window[:, 0] is the initial state, window[:, k] the truth k steps later. The samples of successive add
    calls enter every accumulator in the order (call, b), so q_fields() is the reference's numpy loop over those
    samples bit for bit (given the network's outputs)."""

    def __init__(self, model: LGUnet, leads: int = 1, C: int | None = None):
        C = model.in_ch if C is None else int(C)
        if model.in_ch != C or model.out_ch < C:
            raise ValueError(f"the network maps {model.in_ch} to {model.out_ch} channels: it cannot be rolled out on "
                             f"{C} state channels")
        if leads < 1:
            raise ValueError(f"leads = {leads}: at least one")
        self.model, self.ctx, self.leads, self.C = model, model.ctx, int(leads), C
        self.B, self.H, self.W = model.batch, model.H, model.W
        dev = model.device
        self.cell = torch.zeros(self.leads, C, self.H, self.W, device=dev, dtype=torch.float64)
        self.chan = torch.zeros(self.leads, C, device=dev, dtype=torch.float64)
        self.n = 0
        self._out = torch.empty(self.B, model.out_ch, self.H, self.W, device=dev, dtype=torch.float32)
        self._z = torch.empty(self.B, C, self.H, self.W, device=dev, dtype=torch.float32)

    def add(self, window: torch.Tensor) -> None:
        shape = (self.B, self.leads + 1, self.C, self.H, self.W)
        if not (isinstance(window, torch.Tensor) and window.is_cuda and window.dtype == torch.float32 and
                tuple(window.shape) == shape and window.is_contiguous()):
            raise ValueError(f"window must be a contiguous float32 device tensor {shape}")
        self._z.copy_(window[:, 0])
        for k in range(1, self.leads + 1):
            out = self.model.forward_raw(self._z, out=self._out)
            err_accum(self.ctx, out, window[:, k], self.cell[k - 1], self.chan[k - 1], C=self.C)
            if k < self.leads:
                self._z.copy_(out[:, :self.C])  # z = model(z)[:, :C]
        self.n += self.B

    def _need_samples(self):
        if self.n < 1:
            raise ValueError("no samples yet: add() a window first")

    def q_fields(self) -> torch.Tensor:
        """(leads, C, H, W) float64 on the device: cell / n, calculate_q's `error_var / total_step` per lead."""
        self._need_samples()
        out = torch.empty_like(self.cell)
        for k in range(self.leads):
            err_finalize(self.ctx, self.cell[k], self.n, q_field=out[k], table=False)
        return out

    def q_table(self) -> torch.Tensor:
        """(leads, C) float64 on the device: the grid means of q_fields(), the rows init_q_matrix (q_type 0) computes
        from the saved files."""
        self._need_samples()
        return torch.stack([err_finalize(self.ctx, self.cell[k], self.n, q_field=False)[1]
                            for k in range(self.leads)], 0)

    def moments(self):
        """(mean, std), each (leads, C) float64 numpy: the error's mean chan / N and standard deviation
        sqrt(sum(cell) / N - mean^2) per lead and channel over the N = n H W differences seen."""
        self._need_samples()
        N = float(self.n) * self.H * self.W
        mean = self.chan.cpu().numpy() / N
        m2 = self.q_table().cpu().numpy()  # sum(cell / n) / (H W)
        return mean, np.sqrt(m2 - mean * mean)

    def save(self, coeff_dir: str) -> None:
        """q1.npy .. q{leads}.npy, float64 (C, H, W), under coeff_dir: what problem.init_q_matrix(coeff_dir, 0, ...)
        loads."""
        os.makedirs(coeff_dir, exist_ok=True)
        q = self.q_fields().cpu().numpy()
        for k in range(self.leads):
            np.save(os.path.join(coeff_dir, "q%d.npy" % (k + 1)), q[k])


def calculate_q(model: LGUnet, batches) -> np.ndarray:
    """calculate_q (model/model.py:469-490) on the engine: `batches` yields (B, 2, C, H, W) windows (state, state one
    step later; numpy or torch, a host window is uploaded), B the network's batch; returns the (C, H, W) float64 mean
    squared one-step error, the content of q1.npy. The reference takes one sample per step; here a step holds B."""
    stats = ErrorStats(model, 1)
    for w in batches:
        if not isinstance(w, torch.Tensor):
            w = torch.from_numpy(np.ascontiguousarray(w, np.float32))
        stats.add(w.to(device=model.device, dtype=torch.float32).contiguous())
    return stats.q_fields()[0].cpu().numpy()


def static_r(ctx: Context, obs_var, q, T: int, Hs: int, Ws: int, interp=None, device: int | None = None):
    """The static R of get_static_info (da_4dvar.py:630-634) as a device tensor (T, C, Hs, Ws) from obs_var (C,) and
    the q table (T-1, C) of problem.init_q_matrix or ErrorStats.q_table (numpy or torch; None: zeros), rounded as the
    reference rounds it (problem.static_r_table); with the (n_out, n_in) level operator `interp` the observation-space
    R (T, 4 + 5*n_out, Hs, Ws) of get_R_matrix_from_gt (:729-756). Only the (T, C) table crosses PCIe."""
    if isinstance(q, torch.Tensor):
        q = q.detach().cpu().numpy()
    tab = static_r_table(obs_var, q, T)
    return r_fill(ctx, tab, Hs, Ws, interp=interp, device=ctx.device if device is None else device)
