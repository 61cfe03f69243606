"""Model-error calibration on the HIP engine: the Q of the 4D-Var window and the static R built from it.

  calculate_q     model/model.py:469-490   stream a data set through the flow model, accumulate the squared one-step
                                           error per grid cell, divide by the sample count -> q1.npy
  ErrorStats                               the same for leads 1 .. L in one pass (q1.npy .. qL.npy: the files
                                           init_q_matrix reads, da_4dvar.py:528-550), plus the per-channel error
                                           moments err_std / stdTr are made of (model/model.py:538-593)
  static_r        da_4dvar.py:630-634      R[0] = obs_var, R[t] = obs_var + q[t-1] as a dense device field
                  da_4dvar.py:729-756      and get_R_matrix_from_gt of it when the level operator is given
  ErrorSamples    model/model.py:580-596   the VAE's samples: (truth - `lead`-step forecast) / err_std, resampled
  VAEStats        nf_model/vae.py:99-107   a VAE checkpoint on such samples: ELBO terms, reconstruction error, KL per
                                           latent channel and the aggregate posterior's moments
  DepartureStats  (not in the reference)   the check of that R: O-B / O-A departure moments per time level and
                                           observation channel over cycles (vv_obs_stats) and the consistency estimates
                                           of Desroziers et al. (2005) made from them

The forwards run with the network's batch B (vv_model_forward); the accumulation (vv_err_accum), the division and the
plane means (vv_err_finalize) and the broadcast (vv_r_fill) are HIP kernels; the accumulators stay on the device in
float64 and nothing synchronises until a result is fetched.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import config
from . import fields as F
from .engine import Context, LGUnet, err_accum, err_finalize, err_sample, r_fill, vae_sample, vae_sse
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


class ErrorSamples:
    """The error samples a VAE_lr is trained and evaluated on (vae_nmc_model.train, model/model.py:580-596): the
    truth minus the `lead`-step forecast of `model` from the window's first state, divided by err_std per channel and
    nearest-resampled to `size` (default: the model grid). model: as for ErrorStats."""

    def __init__(self, model: LGUnet, lead: int = 4, err_std=config.STD_TR, size=None):
        C = model.in_ch
        if model.out_ch < C:
            raise ValueError(f"the network maps {C} to {model.out_ch} channels: it cannot be rolled out")
        if lead < 1:
            raise ValueError(f"lead = {lead}: at least one")
        sd = np.asarray(err_std.detach().cpu() if isinstance(err_std, torch.Tensor) else err_std, np.float32)
        if sd.shape != (C,):
            raise ValueError(f"err_std must hold {C} values, got {sd.shape}")
        self.model, self.ctx, self.lead, self.C = model, model.ctx, int(lead), C
        self.size = (model.H, model.W) if size is None else (int(size[0]), int(size[1]))
        self.err_std = torch.from_numpy(sd.copy()).to(model.device)
        self._out = torch.empty(model.batch, model.out_ch, model.H, model.W, device=model.device, dtype=torch.float32)
        self._z = torch.empty(model.batch, C, model.H, model.W, device=model.device, dtype=torch.float32)

    def make(self, first: torch.Tensor, last: torch.Tensor, out=None) -> torch.Tensor:
        """first, last: (B, C, H, W) fp32 device tensors or views with contiguous samples (window[:, 0] and
        window[:, lead]). Returns the (B, C, Hn, Wn) samples; no synchronisation."""
        self._z.copy_(first)
        for k in range(self.lead):
            o = self.model.forward_raw(self._z, out=self._out)
            if k + 1 < self.lead:
                self._z.copy_(o[:, :self.C])  # pred1 = fengwu(pred1)[:, :69]
        return err_sample(self.ctx, self._out, last, self.err_std, self.size, out=out, C=self.C)


class VAEStats:
    """How well a VAE checkpoint fits a set of error samples: what a user needs before trusting J_b = |z|^2 / 2.

    vae: a vaevar.vae.VAE_lr of batch B; sigma: the sigma of loss_function (nf_model/vae.py:104-107). add(err, seed,
    draw) runs encoder -> sample -> decoder twice (a posterior draw and the posterior mean) and adds the B samples'
    tables to float64 device accumulators one sample after the other, in the order (call, b), so two runs over the same
    samples agree bit for bit. Nothing synchronises before summary()."""

    def __init__(self, vae, sigma: float):
        self.vae, self.ctx, self.sigma = vae, vae.ctx, float(sigma)
        dev = vae.device
        self.n = 0
        self.sse = torch.zeros(vae.C, device=dev, dtype=torch.float64)       # sampled z
        self.sse_mean = torch.zeros(vae.C, device=dev, dtype=torch.float64)  # z = mu
        self.stat = torch.zeros(vae.L, 4, device=dev, dtype=torch.float64)
        self._enc = torch.empty(vae.batch, 2 * vae.L, vae.H, vae.W, device=dev, dtype=torch.float32)
        self._z = torch.empty(vae.batch, vae.L, vae.H, vae.W, device=dev, dtype=torch.float32)
        self._rec = torch.empty(vae.batch, vae.C, vae.H, vae.W, device=dev, dtype=torch.float32)
        self._sse = torch.empty(vae.batch, vae.C, device=dev, dtype=torch.float64)
        self._stat = torch.empty(vae.batch, vae.L, 4, device=dev, dtype=torch.float64)

    def add(self, err: torch.Tensor, seed: int, draw: int) -> None:
        v = self.vae
        v.encode(err, out=self._enc)
        vae_sample(self.ctx, self._enc, seed, draw, z=self._z, stat=self._stat)
        vae_sse(self.ctx, v.dec.forward_raw(self._z, out=self._rec), err, out=self._sse)
        for b in range(v.batch):
            self.sse += self._sse[b]
            self.stat += self._stat[b]
        vae_sample(self.ctx, self._enc, mean=True, z=self._z)
        vae_sse(self.ctx, v.dec.forward_raw(self._z, out=self._rec), err, out=self._sse)
        for b in range(v.batch):
            self.sse_mean += self._sse[b]
        self.n += v.batch

    def summary(self, threshold: float = 0.01) -> dict:
        """numpy values over the n samples seen:
          loss, rec, kld          the means per sample of loss_function's three outputs
          rmse, rmse_mean (C,)    reconstruction RMSE per state channel, with z sampled and at the posterior mean
          kl_channel (L,)         the mean KL per latent channel (summed over the plane)
          active_units            latent channels whose KL per latent element exceeds `threshold` nats
          agg_mean, agg_var (L,)  the aggregate posterior's mean E[mu] and variance E[sigma^2] + E[mu^2] - E[mu]^2;
                                  the closer to 0 and 1, the better |z|^2 / 2 fits"""
        if self.n < 1:
            raise ValueError("no samples yet: add() some first")
        return vae_summary(self.sse.cpu().numpy(), self.sse_mean.cpu().numpy(), self.stat.cpu().numpy(), self.n,
                           self.vae.H * self.vae.W, self.sigma, threshold)

    def active_units(self, threshold: float = 0.01) -> int:
        return int(self.summary(threshold)["active_units"])


class DepartureStats:
    """O-B / O-A departure statistics over cycles and the consistency check of R (Desroziers et al. 2005): what a user
    needs before trusting --obs_std, --filter_coeff, --q_type or --modify_tp.

    add(table) takes a (T, C_obs, 10) float64 table of fields.obs_stats (a device tensor, or numpy) and adds it to a
    float64 accumulator that stays where the first table lives, in the order of the calls; nothing synchronises before
    summary(). `table` is the accumulated table."""

    def __init__(self):
        self.table = None
        self.cycles = 0

    def add(self, table) -> None:
        if not isinstance(table, torch.Tensor):
            table = torch.from_numpy(np.ascontiguousarray(table, np.float64))
        if table.dim() != 3 or table.shape[2] != F.OSTAT_N or table.dtype != torch.float64:
            raise ValueError(f"table must be (T, C_obs, {F.OSTAT_N}) float64, got {tuple(table.shape)} {table.dtype}")
        if self.table is None:
            self.table = table.clone()
        elif self.table.shape != table.shape:
            raise ValueError(f"table {tuple(table.shape)} does not match the accumulated {tuple(self.table.shape)}")
        else:
            self.table += table.to(self.table.device)
        self.cycles += 1

    def _need_table(self):
        if self.table is None:
            raise ValueError("no table yet: add() one first")

    def summary(self, centred: bool = False) -> dict:
        """(T, C_obs) numpy arrays, NaN where no entry was observed (departure_summary)."""
        self._need_table()
        return departure_summary(self.table.cpu().numpy(), centred)

    def suggested_obs_std(self, std_aug) -> np.ndarray:
        """sqrt(max(r_desroziers[0], 0)) / std_aug per observation channel: the --obs_std (in units of the channel's
        standard deviation std_aug, (C_obs,)) that the departures of time level 0 are consistent with."""
        r = self.summary()["r_desroziers"][0]
        sd = np.asarray(std_aug.detach().cpu() if isinstance(std_aug, torch.Tensor) else std_aug, np.float64)
        if sd.shape != r.shape:
            raise ValueError(f"std_aug must hold {r.shape[0]} values, got {sd.shape}")
        with np.errstate(invalid="ignore"):
            return np.sqrt(np.where(np.isnan(r), np.nan, np.maximum(r, 0.0))) / sd

    def save(self, path: str) -> None:
        """The accumulated table and the number of tables in it, as an .npz file."""
        self._need_table()
        with open(path, "wb") as f:
            np.savez(f, table=self.table.cpu().numpy(), cycles=np.int64(self.cycles))

    @classmethod
    def load(cls, path: str, device=None) -> "DepartureStats":
        with np.load(path) as z:
            out = cls()
            out.table = torch.from_numpy(z["table"].astype(np.float64))
            out.cycles = int(z["cycles"])
        if device is not None:
            out.table = out.table.to(device)
        return out


def departure_summary(table: np.ndarray, centred: bool = False) -> dict:
    """DepartureStats.summary from an accumulated (T, C_obs, 10) table (rows fields.OSTAT_*), with N = row COUNT:
      n                       N
      mean_ob, mean_oa        OB / N, OA / N
      std_ob, std_oa          sqrt(max(OB2 / N - mean_ob^2, 0)) and the same of the analysis
      rms_ob, rms_oa          sqrt(OB2 / N), sqrt(OA2 / N)
      r_prescribed            R / N, the mean prescribed error variance at the observed entries
      r_desroziers            OAOB / N ~ R; centred: minus mean_oa * mean_ob
      hbht_desroziers         (OB2 - OAOB) / N ~ H B H^T
      chi2_b, chi2_a          JB / N, JA / N = 2 J_o / N; chi2_a < 1 for a consistent analysis
    Every entry but n is NaN where N == 0."""
    t = np.asarray(table, np.float64)
    n = t[..., F.OSTAT_COUNT]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(n > 0, 1.0 / n, np.nan)
        m = {k: t[..., i] * inv for k, i in (("ob", F.OSTAT_OB), ("oa", F.OSTAT_OA), ("ob2", F.OSTAT_OB2),
                                             ("oa2", F.OSTAT_OA2), ("oaob", F.OSTAT_OAOB), ("r", F.OSTAT_R),
                                             ("jb", F.OSTAT_JB), ("ja", F.OSTAT_JA))}
        clip = lambda v: np.where(np.isnan(v), np.nan, np.maximum(v, 0.0))  # noqa: E731
        return {"n": n, "mean_ob": m["ob"], "mean_oa": m["oa"],
                "std_ob": np.sqrt(clip(m["ob2"] - m["ob"] * m["ob"])),
                "std_oa": np.sqrt(clip(m["oa2"] - m["oa"] * m["oa"])),
                "rms_ob": np.sqrt(m["ob2"]), "rms_oa": np.sqrt(m["oa2"]),
                "r_prescribed": m["r"],
                "r_desroziers": m["oaob"] - (m["oa"] * m["ob"] if centred else 0.0),
                "hbht_desroziers": m["ob2"] - m["oaob"],
                "chi2_b": m["jb"], "chi2_a": m["ja"]}


def vae_summary(sse: np.ndarray, sse_mean: np.ndarray, stat: np.ndarray, n: int, HW: int, sigma: float,
                threshold: float = 0.01) -> dict:
    """VAEStats.summary from the accumulated tables: sse, sse_mean (C,), stat (L, 4) as vv_vae_sample defines it."""
    N = float(n) * HW
    rec = sse.sum() / n
    kl_channel = -0.5 * stat[:, 0] / n
    kld = kl_channel.sum()
    e_mu, e_mu2, e_var = stat[:, 1] / N, stat[:, 2] / N, stat[:, 3] / N
    return {"n": n, "loss": rec / (2.0 * sigma ** 2) + kld, "rec": rec, "kld": kld,
            "rmse": np.sqrt(sse / N), "rmse_mean": np.sqrt(sse_mean / N), "kl_channel": kl_channel,
            "active_units": int((kl_channel / HW > threshold).sum()),
            "agg_mean": e_mu, "agg_var": e_var + e_mu2 - e_mu * e_mu}
