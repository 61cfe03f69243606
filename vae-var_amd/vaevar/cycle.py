"""The assimilation cycle of cyclic_4dvar on the HIP engine, da_mode vae4dvar, sc4dvar or free_run
(CyclicDA) and interpolation (CyclicInterpolation).

  run_assimilation        da_4dvar.py:1314-1342  obs -> one_step_DA -> save results -> xb = integrate(xa, fcst, 1)
  one_step_DA             da_4dvar.py:933-1306   the mode's analysis, --use_eval split and held-out verification
  get_current_states      da_4dvar.py:683-696    resume from da_cycle_results/<name>/{current_time.txt, xb.npy}
  save_ckpt               da_4dvar.py:698-702
  save_eval_result        da_4dvar.py:704-714    metrics_list entries as <key>.npy (+ xb_/xa_ fields on request)
  get_state (layout)      da_4dvar.py:148-166    ERA5 channel order and per-variable .npy file names

The state stays on the device for the whole cycle: analysis, forecast (vv_integrate) and the WRMSE/Bias
diagnostics (vv_metrics, vv_obs_error, vv_verify) run on the GPU; only checkpoints and metric vectors go to the host.
Observation and truth access is a provider object (the reference reads them from petrel/S3, out of scope here);
RealObs runs get_obs_info's quality control of real observations (:764-800, vv_obs_qc) on the device; StationObs and
ReportMaskObs also grid the station reports there (get_real_obs :301-440, get_obs_mask :190-274, vv_obs_grid); FreeObs
draws the random networks of obs_type free_* and the observation noise there (:276-292, :449, vv_obs_synth).
"""
from __future__ import annotations

import datetime as _dt
import os

import numpy as np
import torch

from . import config as C
from .da import one_step_da
from .engine import DAProblem, LGUnet, integrate
from .fields import OSTAT_N, obs_stats
from .metrics import CLIM_SCORES, VERIFY_NAMES, Metrics, held_out
from .sc4dvar import Sc4dvarProblem, one_step_sc4dvar

SINGLE_LEVEL = ["u10", "v10", "t2m", "msl"]
MULTI_LEVEL = ["z", "q", "u", "v", "t"]
HEIGHT_LEVEL = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
CHANNELS = SINGLE_LEVEL + [f"{v}{h}" for v in MULTI_LEVEL for h in HEIGHT_LEVEL]  # the 69 state channels


def _stamp(t: _dt.datetime) -> str:
    return t.strftime("%Y-%m-%dT%H:%M:%S")


class StateFiles:
    """data_reader.get_state's layout (da_4dvar.py:148-166) under a local root instead of the S3 bucket:
    single/<year>/<YYYY-MM-DD>/<HH:MM:SS>-<vname>.npy and <year>/<YYYY-MM-DD>/<HH:MM:SS>-<vname>-<level>.0.npy,
    each one (H, W) float32 field; channels stacked in CHANNELS order."""

    def __init__(self, root: str, shape=(721, 1440)):
        self.root, self.shape = root, tuple(shape)

    def _paths(self, t: _dt.datetime):
        day, hms = _stamp(t).split("T")
        for v in SINGLE_LEVEL:
            yield os.path.join(self.root, "single", str(t.year), day, f"{hms}-{v}.npy")
        for v in MULTI_LEVEL:
            for h in HEIGHT_LEVEL:
                yield os.path.join(self.root, str(t.year), day, f"{hms}-{v}-{float(h)}.npy")

    def get_state(self, t: _dt.datetime) -> np.ndarray:
        return np.concatenate([np.load(p).reshape(1, *self.shape) for p in self._paths(t)], 0).astype(np.float32)

    def put_state(self, t: _dt.datetime, x: np.ndarray) -> None:
        for p, f in zip(self._paths(t), np.asarray(x, np.float32)):
            os.makedirs(os.path.dirname(p), exist_ok=True)
            np.save(p, f)


class SyntheticObs:
    """get_obs_info for the non-'real' observation types (da_4dvar.py:758-763): gt = the truth states of the window
    (get_obs_gt, :445-455: current time and da_win-1 steps of step_int_time), yo = gt, H a fixed mask, R the static
    R. `truth(t)` returns the (C,Hs,Ws) truth at time t (e.g. StateFiles.get_state)."""

    def __init__(self, truth, H: np.ndarray, R: np.ndarray, da_win: int = 1,
                 step_int_time: _dt.timedelta = _dt.timedelta(hours=1)):
        self.truth, self.H, self.R = truth, H, R
        self.da_win, self.step = da_win, step_int_time

    def get_obs_info(self, t: _dt.datetime):
        gt = np.stack([self.truth(t + i * self.step) for i in range(self.da_win)], 0).astype(np.float32)
        return gt, self.H, self.R, gt  # yo, H, R, gt


def _device_r(R, dev, interp, aug):
    """The providers' R argument as the device field the analysis binds: a host array is uploaded and, with the level
    operator, interpolated (get_R_matrix_from_gt, da_4dvar.py:729-756), as before; a device tensor (calib.static_r)
    that already has the 4 + 5*n_out observation channels is used as is, one in the state's channels is interpolated."""
    if isinstance(R, torch.Tensor) and R.is_cuda:
        R = R.to(device=dev, dtype=torch.float32).contiguous()
        if interp is None or R.shape[1] == 4 + 5 * interp.shape[0]:
            return R
        return aug(R)
    R = torch.as_tensor(np.asarray(R, np.float32)).to(dev)
    return R if interp is None else aug(R)


class SyntheticRealObs:
    """get_obs_info for obs_type 'real_simu_nofiltering' (da_4dvar.py:764-792): the truth window gt, its level
    interpolation gt_aug = x_aug(gt) (obs_interpolater, :770-776), yo = gt_aug * H (no filtering mask, :783-792),
    R = get_R_matrix_from_gt (:729-756), all in the 4 + 5*n_out observation channels; x_aug runs on the GPU
    (vv_obs_augment). H: (da_win, 4 + 5*n_out, Hs, Ws) station mask; R: the static (da_win, 69, Hs, Ws) R, or a device
    tensor that is already the (da_win, 4 + 5*n_out, Hs, Ws) observation-space R (calib.static_r with the operator)."""

    def __init__(self, ctx, truth, H, R, interp, da_win: int = 1,
                 step_int_time: _dt.timedelta = _dt.timedelta(hours=1), device: int = 0):
        from .engine import obs_augment

        self.dev = torch.device("cuda", device)
        self.truth, self.da_win, self.step = truth, da_win, step_int_time
        self.interp = torch.as_tensor(np.asarray(interp, np.float32)).to(self.dev)
        self.H = torch.as_tensor(np.asarray(H, np.float32)).to(self.dev)
        self._aug = lambda x: obs_augment(ctx, self.interp, x)
        self.R = _device_r(R, self.dev, self.interp, self._aug)

    def get_obs_info(self, t: _dt.datetime):
        gt = np.stack([self.truth(t + i * self.step) for i in range(self.da_win)], 0).astype(np.float32)
        gt_d = torch.from_numpy(gt).to(self.dev)
        yo = self._aug(gt_d) * self.H
        return yo, self.H, self.R, gt_d


class RealObs:
    """get_obs_info for the obs_type real* family (da_4dvar.py:764-800): `reader(t)` returns the window's gridded
    station observations (yo, H), numpy or torch, each (da_win, C_obs, Hs, Ws) (get_real_obs; StationObs below takes
    the reports and grids them on the device); they are uploaded and quality-controlled in place on the device by vv_obs_qc against
    the truth window: H <- H * mask with the departure filter |yo - gt_aug| < filter_coeff * std_layer_aug, and
    yo <- gt_aug * H where the obs_type simulates observations (problem.qc_flags). R = get_R_matrix_from_gt of the
    static (da_win, C, Hs, Ws) R (a device tensor that already has the C_obs channels -- calib.static_r with the
    operator -- is used as is). interp None: the identity operator (C_obs = C). self.counts: the (da_win, 2)
    observation amounts before / after filtering of the last window (:768, :793), on the host."""

    def __init__(self, ctx, truth, reader, R, interp, obs_type: str, filter_coeff: float, std=None, da_win: int = 1,
                 step_int_time: _dt.timedelta = _dt.timedelta(hours=1), device: int = 0):
        from .engine import obs_augment
        from .problem import qc_flags, qc_threshold

        self.ctx, self.dev = ctx, torch.device("cuda", device)
        self.truth, self.reader, self.da_win, self.step = truth, reader, da_win, step_int_time
        self.obs_type, self.flags = obs_type, qc_flags(obs_type)
        self.interp = None if interp is None else torch.as_tensor(np.asarray(interp, np.float32)).to(self.dev)
        R = _device_r(R, self.dev, self.interp, lambda x: obs_augment(ctx, self.interp, x))
        if std is None:
            std = C.MODEL_STD[:R.shape[1] if self.interp is None else 4 + 5 * self.interp.shape[1]]
        self.thr = qc_threshold(filter_coeff, interp, std).to(self.dev)
        self.R = R
        self.counts = None

    def _upload(self, a):
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, np.float32))
        # always a fresh device copy: vv_obs_qc works in place and the reader's arrays stay the reader's
        return a.to(device=self.dev, dtype=torch.float32, copy=True).contiguous()

    def get_obs_info(self, t: _dt.datetime):
        from .engine import obs_qc

        gt = np.stack([self.truth(t + i * self.step) for i in range(self.da_win)], 0).astype(np.float32)
        gt_d = torch.from_numpy(gt).to(self.dev)
        yo, H = (self._upload(a) for a in self.reader(t))
        self.counts = obs_qc(self.ctx, gt_d, yo, H, self.interp, self.thr, self.flags).cpu().numpy()
        return yo, H, self.R, gt_d


class StationObs(RealObs):
    """RealObs fed with station reports instead of gridded arrays: `reports(t)` returns the window's (N, 12) float64
    table (reports.pack_reports of the file at t, and for da_win 6 of the file at t + cycle_time with src = 1). The
    table is uploaded, gridded on the device by vv_obs_grid (get_real_obs, da_4dvar.py:301-440) to yo and H
    (da_win, 4 + 5*n_out, Hs, Ws), and those are quality-controlled by vv_obs_qc as in RealObs; nothing dense crosses
    PCIe. levels: an ObsInterpolater (or the observation space's pressure levels) whose interp is `interp`.
    self.counts as in RealObs; self.grid_stats: (4,) int64 on the host, rows used / skipped / dropped and cells
    observed of the last window (vv_obs_grid's stats)."""

    def __init__(self, ctx, truth, reports, R, interp, levels, obs_type: str, filter_coeff: float, std=None,
                 da_win: int = 1, step_int_time: _dt.timedelta = _dt.timedelta(hours=1), device: int = 0):
        super().__init__(ctx, truth, None, R, interp, obs_type, filter_coeff, std=std, da_win=da_win,
                         step_int_time=step_int_time, device=device)
        if self.interp is None:
            raise ValueError("station reports are gridded in the interpolated observation channels: interp is needed")
        self.reports, self.levels = reports, levels
        self.grid_stats = None

    def get_obs_info(self, t: _dt.datetime):
        from .engine import obs_grid, obs_qc
        from .reports import GRID_REAL

        gt = np.stack([self.truth(t + i * self.step) for i in range(self.da_win)], 0).astype(np.float32)
        gt_d = torch.from_numpy(gt).to(self.dev)
        yo, H, stats = obs_grid(self.ctx, self.reports(t), GRID_REAL, self.da_win, self.levels, gt.shape[2],
                                gt.shape[3], device=self.dev.index)
        counts = obs_qc(self.ctx, gt_d, yo, H, self.interp, self.thr, self.flags)
        self.grid_stats, self.counts = stats.cpu().numpy(), counts.cpu().numpy()
        return yo, H, self.R, gt_d


class ReportMaskObs(SyntheticObs):
    """get_obs_info for obs_type prepbufr* (da_4dvar.py:760-763 with get_obs_mask, :190-274): SyntheticObs whose H is
    built every cycle from the window's station reports by vv_obs_grid in mask mode: (da_win, 69, Hs, Ws) on the
    device, 1 where a report observes the state channel. `reports(t)` as for StationObs; the grid is the truth's.
    self.grid_stats as in StationObs."""

    def __init__(self, ctx, truth, reports, R: np.ndarray, da_win: int = 1,
                 step_int_time: _dt.timedelta = _dt.timedelta(hours=1), device: int = 0):
        super().__init__(truth, None, R, da_win, step_int_time)
        self.ctx, self.reports, self.device = ctx, reports, device
        self.grid_stats = None

    def get_obs_info(self, t: _dt.datetime):
        from .engine import obs_grid
        from .reports import GRID_MASK

        gt, _, R, _ = super().get_obs_info(t)
        _, self.H, stats = obs_grid(self.ctx, self.reports(t), GRID_MASK, self.da_win, None, gt.shape[2], gt.shape[3],
                                    device=self.device)
        self.grid_stats = stats.cpu().numpy()
        return gt, self.H, R, gt


_EPOCH = _dt.datetime(1970, 1, 1)


class FreeObs:
    """get_obs_info for obs_type free_NNNN (da_4dvar.py:758-763 with get_obs_mask :276-292, get_obs_gt :442-452 and
    the static R :630-634) on the device (vv_obs_synth): every cycle a fresh random network of exactly
    problem.free_amount(obs_type) cells, shared by all channels and time slots; yo = gt, or with noise=True
    yo = gt + sqrt(obs_var) * eps (the reference's commented-out term, :449; obs_var (C,) is then required); R
    broadcast from r_table (T, C) (problem.r_table). Only the truth window crosses PCIe. The network and the noise are
    a function of (seed, noise_seed, t): the draw number is the whole hours from 1970-01-01 to t modulo 2^32, so a
    resumed cycle redraws what an uninterrupted one drew. Returns device (yo, H, R, gt) as RealObs does.
    self.amount: the cells per network; self.stats: (2,) int64 on the host after a window, cells selected and cells
    that share the threshold key (vv_obs_synth's stats)."""

    def __init__(self, ctx, truth, obs_type: str, r_table, da_win: int = 1,
                 step_int_time: _dt.timedelta = _dt.timedelta(hours=1), seed: int = 0, noise: bool = False,
                 obs_var=None, noise_seed=None, device: int = 0):
        from .problem import free_amount

        self.ctx, self.dev = ctx, torch.device("cuda", device)
        self.truth, self.obs_type, self.da_win, self.step = truth, obs_type, da_win, step_int_time
        self.amount = free_amount(obs_type)
        self.r_table = np.asarray(r_table, np.float32)
        if self.r_table.ndim != 2 or self.r_table.shape[0] != da_win:
            raise ValueError(f"r_table must be (da_win = {da_win}, C), got {self.r_table.shape}")
        self.seed, self.noise_seed, self.noise = seed, noise_seed, bool(noise)
        self.sd = None
        if self.noise:
            if obs_var is None:
                raise ValueError("noise=True needs obs_var (C,): yo = gt + sqrt(obs_var) * eps")
            self.sd = np.sqrt(np.asarray(obs_var, np.float32).reshape(-1))
        self.stats = None

    @staticmethod
    def draw_number(t: _dt.datetime) -> int:
        return ((t - _EPOCH) // _dt.timedelta(hours=1)) % 2 ** 32

    def get_obs_info(self, t: _dt.datetime):
        from .engine import obs_synth

        gt = np.stack([self.truth(t + i * self.step) for i in range(self.da_win)], 0).astype(np.float32)
        cells = gt.shape[2] * gt.shape[3]
        if self.amount > cells:
            raise ValueError(f"obs_type {self.obs_type!r} asks for {self.amount} observed cells, the "
                             f"{gt.shape[2]} x {gt.shape[3]} grid has {cells}")
        gt_d = torch.from_numpy(gt).to(self.dev)
        yo, H, R, stats = obs_synth(self.ctx, gt_d, self.amount, self.seed, self.draw_number(t), sd=self.sd,
                                    r_table=self.r_table, noise_seed=self.noise_seed)
        self.stats = stats.cpu().numpy()
        return yo, H, R, gt_d


DA_MODES = ("vae4dvar", "sc4dvar", "free_run")


class CyclicDA:
    """cyclic_4dvar (da_4dvar.py:933-1306, 1314-1342) for --da_mode

      vae4dvar   the latent-space analysis (:1179-1306): `decoder` (and `flow` for a window of T > 1);
      sc4dvar    the static-B analysis (:1064-1177): `bmatrix` (vaevar.sc4dvar.BMatrix), no decoder; 69 channels;
      free_run   no assimilation (:942-966): xa = xb, the background's WRMSE / Bias / MSE logged as bg_* and ana_*.

    --use_eval (:934-937): with use_eval and the (Hs,Ws) pixel mask mask_eval (dataset/mask_eval1.npy) the analysis
    is bound with H * (1 - mask_eval) and, on the last outer pass, verified against the held-out station
    observations (error_obs, :1154-1155 / :1285-1286) on the device; one vector per cycle, saved as error_obs.npy.
    --forecast_eval (:529, :1336-1338): with forecast_eval the forecast started from every analysis is scored
    against obs.truth at the leads 1 .. forecast_steps cycle times (forecast_rollout; Metrics.verify on the device),
    one (forecast_steps, C) array per cycle and per name in forecast_scores (metrics.VERIFY_NAMES), saved as
    forecast_wrmse.npy -- the reference's file -- and forecast_<name lowercased>.npy and reloaded on resume. clim: a
    callable t -> (C,H,W), needed by the climatology scores (metrics.CLIM_SCORES). Off by default: xb, xa and every
    other file are the same bits with it on.
    obs_list: with observation-space fields (obs_interp, obs_type real*) every cycle's problem turns the observation
    list on right after binding (DAProblem.obs_list / Sc4dvarProblem.obs_list: the observation term from the compacted
    entries with H != 0, here H * (1 - mask_eval) under use_eval since the split precedes the bind). Off by default,
    and then every file a cycle writes is unchanged; without observation-space fields it does nothing.
    obs_stats: every cycle's O-B / O-A departure table (fields.obs_stats; (T, C_obs, 10) float64) against the cycle's
    own yo, H, R is kept in departure_tables["obs_stats"], saved as obs_stats.npy (n_cycles, T, C_obs, 10) and reloaded
    on resume as the forecast scores are; under use_eval also obs_stats_heldout.npy, the same over the held-out
    observations H_old * mask_eval. self.departures (calib.DepartureStats) accumulates the tables for the Desroziers
    check of R. free_run records time level 0 of the background (no analysis: its rows and the other time levels are
    NaN). Off by default, and then no file appears or changes and metrics_list keeps the reference's key set.
    Checkpoint, resume and the save_field layout are the same for every mode. Any other da_mode raises
    NotImplementedError (the reference's one_step_DA, :1308-1309)."""

    _MODES = DA_MODES

    def __init__(self, forecast: LGUnet, obs, start_time: _dt.datetime, end_time: _dt.datetime, Nit: int, name: str,
                 da_mode: str = "vae4dvar", decoder: LGUnet | None = None, bmatrix=None,
                 out_dir: str = "da_cycle_results", cycle_time=_dt.timedelta(hours=6), flow: LGUnet | None = None,
                 obs_coeff: float = 1.0, save_interval: int = 1, xb0=None, mean=None, std=None, std_tr=None,
                 obs_interp=None, save_field: bool = False, device: int = 0, use_eval: bool = False,
                 mask_eval=None, forecast_eval: bool = False, forecast_steps: int | None = None,
                 forecast_scores=("WRMSE",), clim=None, obs_list: bool = False, obs_stats: bool = False):
        if da_mode not in self._MODES:
            hint = " (da_mode 'interpolation' is the class CyclicInterpolation)" if da_mode == "interpolation" else ""
            raise NotImplementedError(f"da_mode {da_mode!r}: expected one of {self._MODES}{hint}")
        if da_mode == "vae4dvar" and decoder is None:
            raise ValueError("da_mode 'vae4dvar' needs the decoder")
        if da_mode == "sc4dvar" and (bmatrix is None or decoder is not None):
            raise ValueError("da_mode 'sc4dvar' takes a BMatrix and no decoder")
        if da_mode == "free_run" and (bmatrix is not None or decoder is not None):
            raise ValueError("da_mode 'free_run' takes only the forecast model")
        if use_eval and mask_eval is None:
            raise ValueError("use_eval needs mask_eval (Hs, Ws)")
        self.da_mode, self.bmat = da_mode, bmatrix
        self.dec, self.fcst, self.flow, self.obs = decoder, forecast, flow, obs
        self.start_time, self.end_time, self.cycle_time = start_time, end_time, cycle_time
        self.Nit, self.name, self.obs_coeff, self.save_interval = Nit, name, obs_coeff, save_interval
        self.dir = os.path.join(out_dir, name)
        self.obs_interp, self.save_field = obs_interp, save_field
        self.obs_list = bool(obs_list)
        dev = torch.device("cuda", device)
        if decoder is not None:
            nch = decoder.out_ch if hasattr(decoder, "out_ch") else C.NCHANNEL
        else:
            nch = C.NCHANNEL if mean is None else len(mean)
        self.mean = np.asarray(C.MODEL_MEAN[:nch] if mean is None else mean, np.float32)
        self.std = np.asarray(C.MODEL_STD[:nch] if std is None else std, np.float32)
        self.std_tr = np.asarray(C.STD_TR[:nch] if std_tr is None else std_tr, np.float32)
        self.mean_d = torch.from_numpy(self.mean).to(dev)
        self.std_d = torch.from_numpy(self.std).to(dev)
        ctx = decoder.ctx if decoder is not None else forecast.ctx
        self.metric = Metrics(ctx, self.mean, C.MODEL_STD[:nch] if std is None else std, device)
        self.use_eval = bool(use_eval)
        self.mask_eval = None
        if self.use_eval:
            self.mask_eval = torch.as_tensor(np.asarray(mask_eval, np.float32)).to(dev)
        # the reference's full key set (da_4dvar.py:511), so da_cycle_results/<name>/*.npy match file for file:
        # every mode fills bg_/ana_ wrmse and bias (:1158-1163, :1285-1291; free_run :950-961), free_run also
        # bg_/ana_ mse (:952, :962; the analysis modes compute no MSE they keep), use_eval adds error_obs per cycle
        # (:1164-1165, :1295-1296); a key nothing fills is saved as an empty array
        self.metrics_list = {"bg_wrmse": [], "ana_wrmse": [], "bg_mse": [], "ana_mse": [], "bg_bias": [],
                             "ana_bias": [], "error_obs": []}
        self.dev = dev
        # --forecast_eval (da_4dvar.py:529, :1336-1338; the reference's evaluate() is an empty stub): per cycle one
        # (forecast_steps, C) array per score, saved as forecast_<score>.npy
        self.forecast_eval = bool(forecast_eval)
        self.forecast_steps, self.clim = forecast_steps, clim
        self.forecast_names = tuple(forecast_scores) if self.forecast_eval else ()
        if self.forecast_eval:
            if not isinstance(forecast_steps, (int, np.integer)) or forecast_steps < 1:
                raise ValueError(f"forecast_eval needs forecast_steps >= 1, got {forecast_steps!r}")
            unknown = [n for n in self.forecast_names if n not in VERIFY_NAMES]
            if unknown or not self.forecast_names:
                raise ValueError(f"forecast_scores {unknown or '()'}: expected names out of {VERIFY_NAMES}")
            need = [n for n in self.forecast_names if n in CLIM_SCORES]
            if need and clim is None:
                raise ValueError(f"forecast_scores {need} need a climatology: clim = callable t -> (C,H,W)")
        self.forecast_scores = {n: [] for n in self.forecast_names}
        self.obs_stats = bool(obs_stats)
        names = ("obs_stats",) + (("obs_stats_heldout",) if self.use_eval else ())
        self.departure_tables = {n: [] for n in names} if self.obs_stats else {}
        os.makedirs(self.dir, exist_ok=True)  # init_file_dir (:605-606)
        self._xb0 = xb0
        self.load_eval_ckpts()
        self.get_current_states()

    # -- checkpoint / resume ---------------------------------------------------------------------------------
    def get_current_states(self):
        p = os.path.join(self.dir, "current_time.txt")
        self.current_time = _dt.datetime.fromisoformat(open(p).read().strip()) if os.path.exists(p) else self.start_time
        p = os.path.join(self.dir, "xb.npy")
        if os.path.exists(p):
            self.xb = torch.from_numpy(np.load(p)).to(self.dev)
        else:
            if self._xb0 is None:
                raise ValueError("no checkpoint and no initial background (get_initial_state reads ERA5)")
            self.xb = torch.as_tensor(np.asarray(self._xb0, np.float32)).to(self.dev)
        return self.current_time, self.xb

    def save_ckpt(self, finish: bool = False):
        if not finish:
            np.save(os.path.join(self.dir, "xb"), self.xb.cpu().numpy())
            with open(os.path.join(self.dir, "current_time.txt"), "w") as f:
                f.write(self.current_time.isoformat(sep=" "))

    def load_eval_ckpts(self):
        for k in self.metrics_list:
            p = os.path.join(self.dir, k + ".npy")
            if os.path.exists(p):
                self.metrics_list[k] = list(np.load(p))
        # the reference forgets forecast_wrmse on resume (:511-523 reload metrics_list only); here a resumed run ends
        # with the files of an uninterrupted one. Without forecast_eval the files are neither read nor written.
        for k in self.forecast_names:
            p = self._forecast_file(k)
            if os.path.exists(p):
                self.forecast_scores[k] = list(np.load(p))
        for k in self.departure_tables:
            p = os.path.join(self.dir, k + ".npy")
            if os.path.exists(p):
                self.departure_tables[k] = list(np.load(p))
        if self.obs_stats:
            from .calib import DepartureStats

            self.departures = DepartureStats()
            for tab in self.departure_tables["obs_stats"]:
                self.departures.add(torch.from_numpy(np.asarray(tab, np.float64)).to(self.dev))

    def _forecast_file(self, score: str) -> str:
        # forecast_wrmse.npy is the reference's file name (:1338)
        return os.path.join(self.dir, f"forecast_{score.lower()}.npy")

    def save_eval_result(self, finish: bool = False):
        for k, v in self.metrics_list.items():
            np.save(os.path.join(self.dir, k), np.asarray(v))
        self.save_forecast_scores()
        for k, v in self.departure_tables.items():
            np.save(os.path.join(self.dir, k), np.asarray(v, np.float64))
        if not finish and self.save_field:
            stamp = self.current_time.isoformat(sep=" ")
            np.save(os.path.join(self.dir, f"xb_{stamp}"), self.xb.cpu().numpy())
            np.save(os.path.join(self.dir, f"xa_{stamp}"), self.xa.cpu().numpy())

    def save_forecast_scores(self):
        for k, v in self.forecast_scores.items():
            np.save(self._forecast_file(k),
                    np.asarray(v, np.float64).reshape(len(v), self.forecast_steps, len(self.mean)))

    # -- the cycle ---------------------------------------------------------------------------------------------
    def one_step_DA(self, gt, xb, yo, H, R):
        gt_d = torch.as_tensor(np.asarray(gt, np.float32)).to(self.dev) if not isinstance(gt, torch.Tensor) else gt
        ev = {}
        if self.use_eval:  # :934-937: the analysis sees H * (1 - mask_eval), the verification H_old
            H, H_old = held_out(H, self.mask_eval)
            ev = {"mask_eval": self.mask_eval, "H_old": H_old}
        if self.da_mode == "free_run":  # :942-966
            w0, b0 = self.metric.wrmse_bias(xb, gt_d[0])
            w0, b0, mse = w0.cpu().numpy(), b0.cpu().numpy(), self.metric.mse(xb, gt_d[0])
            for k, v in (("wrmse", w0), ("bias", b0), ("mse", mse)):
                self.metrics_list["bg_" + k].append(v)
                self.metrics_list["ana_" + k].append(v)
            self.last = {"xa": xb, "metrics": [(w0, b0)], "mse": mse}
            if self.obs_stats:
                self.last.update(self._free_run_tables(xb, yo, H, R, ev))
                self._keep_tables(self.last)
            return xb
        prob = {"xb": xb, "yo": yo, "H": H, "R": R, "mean": self.mean, "std": self.std, "std_tr": self.std_tr}
        if self.da_mode == "vae4dvar":
            p = DAProblem(self.dec, prob, flow=self.flow, obs_coeff=self.obs_coeff, obs_interp=self.obs_interp)
            if self.obs_list and p.interp is not None:
                p.obs_list(True)
            res = one_step_da(p, self.Nit, gt=gt_d, metrics=self.metric, obs_stats=self.obs_stats, **ev)
        else:
            p = Sc4dvarProblem(self.bmat, prob, flow=self.flow, obs_coeff=self.obs_coeff, device=self.dev.index,
                               obs_interp=self.obs_interp)
            if self.obs_list and p.interp is not None:
                p.obs_list(True)
            res = one_step_sc4dvar(p, self.Nit, gt=gt_d, metrics=self.metric, obs_stats=self.obs_stats, **ev)
        # da_4dvar.py:1285-1291 / :1158-1165: pass kk == 0 -> bg_*, `elif kk == Nit` -> ana_* and error_obs (so
        # Nit = 0 records only bg_*)
        w0, b0 = res["metrics"][0]
        self.metrics_list["bg_wrmse"].append(w0)
        self.metrics_list["bg_bias"].append(b0)
        if self.Nit > 0:
            w1, b1 = res["metrics"][self.Nit]
            self.metrics_list["ana_wrmse"].append(w1)
            self.metrics_list["ana_bias"].append(b1)
            if self.use_eval:
                self.metrics_list["error_obs"].append(res["error_obs"])
        self._keep_tables(res)
        self.last = res
        return res["xa"]

    def _keep_tables(self, res):
        for k in self.departure_tables:
            self.departure_tables[k].append(res[k])
        if self.obs_stats:  # accumulated on the device, in the order of the cycles
            self.departures.add(torch.from_numpy(np.asarray(res["obs_stats"], np.float64)).to(self.dev))

    def _free_run_tables(self, xb, yo, H, R, ev) -> dict:
        """free_run's departure tables: time level 0 of the background against yo[0], no analysis; the other time
        levels stay NaN."""

        def dev(a):
            a = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, np.float32))
            return a.to(device=self.dev, dtype=torch.float32)

        yo, H, R = dev(yo), dev(H), dev(R)
        interp = None if self.obs_interp is None else dev(self.obs_interp)
        masks = {"obs_stats": H}
        if ev:
            masks["obs_stats_heldout"] = ev["H_old"] * ev["mask_eval"]
        out = {}
        for k, m in masks.items():
            tab = np.full((yo.shape[0], yo.shape[1], OSTAT_N), np.nan)
            tab[0] = obs_stats(self.fcst.ctx, xb[None].contiguous(), None, yo[:1].contiguous(), m[:1].contiguous(),
                               R[:1].contiguous(), interp)[0].cpu().numpy()
            out[k] = tab
        return out

    def forecast_rollout(self, t: _dt.datetime, x1: torch.Tensor):
        """--forecast_eval: the forecast started from the analysis of time t, scored against the truth at every
        lead k = 1 .. forecast_steps (Metrics.verify). x1 is lead 1 -- the cycle's own background of t + cycle_time,
        not recomputed --, leads 2.. continue from it one integrate step each, and each state is scored as it is
        produced (two forecast states alive at most). A truth the provider does not have (FileNotFoundError,
        KeyError) ends the rollout BEFORE the step to that lead: that lead and the later ones stay NaN. Appends one
        (forecast_steps, C) array per score to self.forecast_scores."""
        K, nch = self.forecast_steps, x1.shape[0]
        rows = {n: torch.full((K, nch), float("nan"), device=self.dev, dtype=torch.float64)
                for n in self.forecast_names}
        with_clim = any(n in CLIM_SCORES for n in self.forecast_names)
        x = x1
        for k in range(1, K + 1):
            tk = t + k * self.cycle_time
            try:
                truth = self.obs.truth(tk)
            except (FileNotFoundError, KeyError):
                break
            if k > 1:
                x = integrate(self.fcst, x, self.mean_d, self.std_d, 1)
            if not isinstance(truth, torch.Tensor):
                truth = torch.from_numpy(np.asarray(truth, np.float32))
            res = self.metric.verify(x, truth.to(self.dev), self.clim(tk) if with_clim else None)
            for n in self.forecast_names:
                rows[n][k - 1] = res[n]
        for n in self.forecast_names:
            self.forecast_scores[n].append(rows[n].cpu().numpy())

    def run_assimilation(self, log=None):
        epoch = 0
        while self.current_time + self.cycle_time <= self.end_time:
            yo, H, R, gt = self.obs.get_obs_info(self.current_time)
            self.xa = self.one_step_DA(gt, self.xb, yo, H, R)
            self.save_eval_result(finish=False)
            self.xb = integrate(self.fcst, self.xa, self.mean_d, self.std_d, 1)
            if self.forecast_eval:
                self.forecast_rollout(self.current_time, self.xb)
                self.save_forecast_scores()  # before the checkpoint, so a resumed run misses no cycle
            if log is not None:
                log(self.current_time, self.last)
            self.current_time = self.current_time + self.cycle_time
            if epoch % self.save_interval == 0:
                self.save_ckpt(finish=False)
            epoch += 1
        self.save_eval_result(finish=True)


class CyclicVAE4DVar(CyclicDA):
    """cyclic_4dvar restricted to da_mode 'vae4dvar' (da_4dvar.py:1179-1306, 1314-1342): CyclicDA with the decoder as
    the first argument."""

    def __init__(self, decoder: LGUnet, forecast: LGUnet, obs, start_time: _dt.datetime, end_time: _dt.datetime,
                 Nit: int, name: str, **kw):
        super().__init__(forecast, obs, start_time, end_time, Nit, name, da_mode="vae4dvar", decoder=decoder, **kw)


class CyclicInterpolation(CyclicDA):
    """cyclic_4dvar for --da_mode interpolation (da_4dvar.py:968-1061, 1314-1342): the no-model baseline. Every cycle
    the observed cells of time level 0 are triangulated per observation channel on the host and the unobserved cells
    inside their hull are filled by linear interpolation on the device (vaevar.interp.one_step_interpolation); the
    forecast model carries the result to the next cycle. Checkpoint, resume, save_field and run_assimilation are
    CyclicDA's. obs_interp: an ObsInterpolater for obs_type real* (69 state channels, 4 + 5*dim_out observation
    channels), None when the observations are of the state's channels. bg_/ana_ wrmse, bias and mse are filled
    (:978-980, :1056-1058); the mode computes no error_obs, so that key stays empty. use_eval / mask_eval reduce the
    mask as in the other modes (:934-937). triangulate: see interp.pack_triangles."""

    _MODES = ("interpolation",)

    def __init__(self, forecast: LGUnet, obs, start_time: _dt.datetime, end_time: _dt.datetime, name: str,
                 triangulate=None, **kw):
        for k in ("decoder", "bmatrix", "flow", "da_mode", "Nit"):
            if kw.get(k) is not None:
                raise ValueError(f"da_mode 'interpolation' takes no {k}")
            kw.pop(k, None)
        if kw.get("obs_stats"):
            raise ValueError("da_mode 'interpolation' keeps no departure statistics (obs_stats)")
        self.triangulate = triangulate
        super().__init__(forecast, obs, start_time, end_time, 0, name, da_mode="interpolation", **kw)

    def one_step_DA(self, gt, xb, yo, H, R):
        from .interp import one_step_interpolation

        gt_d = torch.as_tensor(np.asarray(gt, np.float32)).to(self.dev) if not isinstance(gt, torch.Tensor) else gt
        res = one_step_interpolation(self.fcst.ctx, xb, yo, H, obs_interp=self.obs_interp, gt=gt_d,
                                     metrics=self.metric, mask_eval=self.mask_eval if self.use_eval else None,
                                     triangulate=self.triangulate)
        for side in ("bg", "ana"):
            for k, v in zip(("wrmse", "bias", "mse"), res["metrics"][side]):
                self.metrics_list[f"{side}_{k}"].append(v)
        self.last = res
        return res["xa"]
