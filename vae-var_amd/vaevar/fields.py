"""The stand-alone field operations of libvaevar (csrc/vv_fieldapi.hip): entry points that take device fields and touch
no model and no bound problem. Every name here is importable from vaevar.engine as well."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import check, lib
from .engine import Context, _ptr, _stream  # noqa: F401  (Context: annotations)


def _dev_table(a, dev, dtype=torch.float32):
    """A numpy or torch table as a contiguous device tensor of `dtype` (a host table is uploaded)."""
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a, np.float64 if dtype == torch.float64 else np.float32))
    return a.to(device=dev, dtype=dtype).contiguous()


def _level_operator(interp, C: int, dev, what: str = ""):
    """The (n_out, n_in) level operator as (fp32 device tensor, n_out, n_in) for fields of C == 4 + 5*n_in channels;
    (None, 0, 0) without one."""
    if interp is None:
        return None, 0, 0
    n_out, n_in = interp.shape
    if C != 4 + 5 * n_in:
        raise ValueError(f"{what}{C} channels, the operator expects {4 + 5 * n_in}")
    return _dev_table(interp, dev), n_out, n_in


def obs_augment(ctx: Context, interp: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """x_aug (da_4dvar.py:1196-1206) of (T, 4 + 5*n_in, H, W) device fields on the GPU; applied to R it is
    get_R_matrix_from_gt (da_4dvar.py:729-756)."""
    T, C, Hs, Ws = x.shape
    interp, n_out, n_in = _level_operator(interp, C, x.device)
    x = x.contiguous()
    out = torch.empty(T, 4 + 5 * n_out, Hs, Ws, device=x.device, dtype=torch.float32)
    check(lib.vv_obs_augment(ctx.h, _ptr(interp), n_out, n_in, _ptr(x), _ptr(out), T, Hs, Ws, _stream()),
          "obs_augment")
    return out


def obs_qc(ctx: Context, gt: torch.Tensor, yo: torch.Tensor, H: torch.Tensor, interp, thr: torch.Tensor, flags: int,
           counts: bool = True):
    """The departure filter of get_obs_info for obs_type real* (da_4dvar.py:764-800; vv_obs_qc) IN PLACE on the
    device fields yo, H (T, C_obs, Hs, Ws) against the truth window gt (T, C, Hs, Ws): H <- H * mask and, on the simu
    channels of `flags` (VV_QC_* bits, problem.qc_flags), yo <- gt_aug * H. interp (n_out, n_in) or None (identity);
    thr (C_obs,) = problem.qc_threshold. Returns the (T, 2) float64 device tensor of the observation amounts before
    and after (:768, :793), or None with counts=False. No synchronisation."""
    for name, t in (("gt", gt), ("yo", yo), ("H", H)):
        if t.dim() != 4:
            raise ValueError(f"{name} must be (T, channels, Hs, Ws)")
    T, C, Hs, Ws = gt.shape
    interp, n_out, n_in = _level_operator(interp, C, gt.device)
    c_obs = 4 + 5 * n_out if interp is not None else C
    if tuple(yo.shape) != (T, c_obs, Hs, Ws) or yo.shape != H.shape:
        raise ValueError(f"yo / H must be {(T, c_obs, Hs, Ws)}, got {tuple(yo.shape)} / {tuple(H.shape)}")
    if thr.numel() != c_obs:
        raise ValueError(f"thr has {thr.numel()} entries for {c_obs} observation channels")
    thr = _dev_table(thr, gt.device)
    out = torch.empty(T, 2, device=gt.device, dtype=torch.float64) if counts else None
    check(lib.vv_obs_qc(ctx.h, _ptr(gt), _ptr(yo), _ptr(H), None if interp is None else _ptr(interp), n_out, n_in,
                        _ptr(thr), int(flags), T, C, Hs, Ws,
                        None if out is None else ctypes.c_void_p(out.data_ptr()), _stream()), "obs_qc")
    return out


def obs_grid(ctx: Context, reports, mode: int, da_win: int, levels, Hs: int, Ws: int, out=None, device: int = 0):
    """Grid station reports on the device (vv_obs_grid): get_real_obs (mode reports.GRID_REAL, da_4dvar.py:301-440)
    or get_obs_mask of obs_type prepbufr* (reports.GRID_MASK, :190-274). reports: the (N, 12) float64 table of
    reports.pack_reports, numpy or torch (a host table is uploaded: the only transfer). levels: an ObsInterpolater or
    the pressure levels of the observation space (real mode); in mask mode the level bounds, None for the reference's
    twelve (reports.MASK_BOUNDS). out: optional (yo, H) device buffers (da_win, 4 + 5*n_lev, Hs, Ws) to overwrite
    (yo may be None in mask mode). Returns (yo, H, stats): yo is `out`'s (None if not given) in mask mode; stats the
    (4,) int64 device tensor rows used / skipped / dropped, cells observed. No synchronisation."""
    from . import reports as R

    dev = torch.device("cuda", device)
    rep = _dev_table(reports, dev, torch.float64)
    if rep.dim() != 2 or rep.shape[1] != 12:
        raise ValueError(f"reports must be (N, 12), got {tuple(rep.shape)}")
    if mode == R.GRID_REAL:
        tabs = [_dev_table(t, dev, torch.float64) for t in R.level_tables(levels)]
        n_lev = tabs[1].numel()
    elif mode == R.GRID_MASK:
        tabs = [_dev_table(R.MASK_BOUNDS if levels is None else levels, dev, torch.float64), None, None, None]
        n_lev = tabs[0].numel() + 1
    else:
        raise ValueError(f"mode {mode!r}: expected reports.GRID_REAL or reports.GRID_MASK")
    shape = (da_win, 4 + 5 * n_lev, Hs, Ws)
    yo, H = out if out is not None else (None, None)
    if H is None:
        H = torch.empty(shape, device=dev)
    if yo is None and mode == R.GRID_REAL:
        yo = torch.empty(shape, device=dev)
    for name, t in (("yo", yo), ("H", H)):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    stats = torch.empty(4, device=dev, dtype=torch.int64)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    check(lib.vv_obs_grid(ctx.h, vp(rep) if rep.numel() else None, rep.shape[0], int(mode), da_win, n_lev, Hs, Ws,
                          vp(tabs[0]) if tabs[0].numel() else None, vp(tabs[1]), vp(tabs[2]), vp(tabs[3]),
                          None if yo is None else _ptr(yo), _ptr(H), vp(stats), _stream()), "obs_grid")
    return yo, H, stats


def obs_synth(ctx: Context, gt: torch.Tensor, n_obs: int, seed: int, draw: int, sd=None, r_table=None,
              noise_seed=None, out=None):
    """Synthetic observations of obs_type free_* on the device (vv_obs_synth; da_4dvar.py:276-292, :449, :630-634):
    from the truth window gt (T, C, Hs, Ws) a network of exactly n_obs cells drawn without replacement (Philox keys
    under `seed` and the 32-bit `draw` number; shared by every channel and time slot), yo = gt + sd[c] * eps with
    Gaussian eps under `noise_seed` (default: seed) when sd (C,) is given, else yo = gt bit for bit, and R broadcast
    from r_table (T, C) (problem.r_table; None: no R). out: optional (yo, H, R) device buffers to overwrite, each may
    be None; yo may be gt itself. Returns (yo, H, R, stats): stats the (2,) int64 device tensor cells selected, cells
    with the threshold key. No synchronisation."""
    if gt.dim() != 4:
        raise ValueError(f"gt must be (T, C, Hs, Ws), got {tuple(gt.shape)}")
    T, C, Hs, Ws = gt.shape
    dev = gt.device
    yo, H, R = out if out is not None else (None, None, None)
    yo = torch.empty_like(gt) if yo is None else yo
    H = torch.empty_like(gt) if H is None else H
    if r_table is None:
        if R is not None:
            raise ValueError("an R buffer needs r_table")
        rt = None
    else:
        rt = _dev_table(r_table, dev)
        if tuple(rt.shape) != (T, C):
            raise ValueError(f"r_table must be {(T, C)}, got {tuple(rt.shape)}")
        R = torch.empty_like(gt) if R is None else R
    for name, t in (("yo", yo), ("H", H), ("R", R)):
        if t is not None and t.shape != gt.shape:
            raise ValueError(f"{name} must be {tuple(gt.shape)}, got {tuple(t.shape)}")
    if sd is not None:
        sd = _dev_table(sd, dev).reshape(-1)
        if sd.numel() != C:
            raise ValueError(f"sd has {sd.numel()} entries for {C} channels")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    noise_seed = seed if noise_seed is None else int(noise_seed) & 0xFFFFFFFFFFFFFFFF
    stats = torch.empty(2, device=dev, dtype=torch.int64)
    check(lib.vv_obs_synth(ctx.h, _ptr(gt), T, C, Hs, Ws, int(n_obs), seed, noise_seed, int(draw) & 0xFFFFFFFF,
                           None if sd is None else _ptr(sd), None if rt is None else _ptr(rt), _ptr(yo), _ptr(H),
                           None if R is None else _ptr(R), ctypes.c_void_p(stats.data_ptr()), _stream()), "obs_synth")
    return yo, H, R, stats


def select_smallest(ctx: Context, keys: torch.Tensor, k: int, out=None):
    """The selection of obs_synth on the caller's keys (vv_select_smallest): keys (n,) int32 or uint32 device tensor
    read as unsigned; returns (mask, stats): mask (n,) fp32 with 1.0 at the k entries smallest in (key, position),
    stats as in obs_synth. No synchronisation."""
    if not (keys.is_cuda and keys.dim() == 1 and keys.is_contiguous() and keys.element_size() == 4 and
            not keys.dtype.is_floating_point):
        raise ValueError("keys must be a contiguous 1-d device tensor of 32-bit integers")
    n = keys.numel()
    mask = torch.empty(n, device=keys.device, dtype=torch.float32) if out is None else out
    if mask.numel() != n:
        raise ValueError(f"out must hold {n} floats")
    stats = torch.empty(2, device=keys.device, dtype=torch.int64)
    check(lib.vv_select_smallest(ctx.h, ctypes.c_void_p(keys.data_ptr()), n, int(k), _ptr(mask),
                                 ctypes.c_void_p(stats.data_ptr()), _stream()), "select_smallest")
    return mask, stats


def normal_fill(ctx: Context, n: int, seed: int, draw: int, first: int = 0, out=None, device: int = 0):
    """out[i] = eps(first + i) of obs_synth's noise stream under the noise seed `seed` and `draw` (vv_normal_fill): n
    standard normal fp32 draws on the device, the bits the fill adds. No synchronisation."""
    if out is None:
        out = torch.empty(int(n), device=torch.device("cuda", device), dtype=torch.float32)
    if out.numel() != n:
        raise ValueError(f"out must hold {n} floats")
    check(lib.vv_normal_fill(ctx.h, _ptr(out) if n else None, int(n), int(first), int(seed) & 0xFFFFFFFFFFFFFFFF,
                             int(draw) & 0xFFFFFFFF, _stream()), "normal_fill")
    return out


def _sample_view(name: str, t: torch.Tensor, C: int):
    """(pointer, batch stride) of a (B, >= C, H, W) fp32 device tensor whose samples are C-contiguous planes: a
    contiguous tensor, a channel slice [:, :C] or a time slice window[:, k] of one."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] >= C):
        raise ValueError(f"{name} must be a (B, >= {C}, H, W) float32 device tensor, got {tuple(t.shape)} {t.dtype}")
    B, _, H, W = t.shape
    if W > 1 and t.stride(3) != 1 or H > 1 and t.stride(2) != W or t.shape[1] > 1 and t.stride(1) != H * W:
        raise ValueError(f"{name}: the (channel, H, W) planes of a sample must be contiguous")
    bs = t.stride(0) if B > 1 else C * H * W
    return ctypes.c_void_p(t.data_ptr()), bs


def _f64_buf(name: str, t, shape):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name} must be a contiguous float64 device tensor {tuple(shape)}")
    return ctypes.c_void_p(t.data_ptr())


def err_accum(ctx: Context, pred: torch.Tensor, tgt: torch.Tensor, cell=None, chan=None, C: int | None = None):
    """One step of calculate_q's `error_var += (output - target)**2` (model/model.py:485-486; vv_err_accum) for the B
    samples of pred and tgt, (B, >= C, H, W) fp32 device tensors or views whose samples hold contiguous planes (the
    network's (B, 138, H, W) output, a time slice window[:, k]); the first C channels are read (default: tgt's).
    cell (C, H, W) += (double)((pred - tgt)^2 in fp32), samples in order, and chan (C,) += the fp64 sum of pred - tgt,
    both float64 device accumulators updated IN PLACE; either may be None. No synchronisation."""
    C = int(tgt.shape[1] if C is None else C)
    pp, ps = _sample_view("pred", pred, C)
    tp, ts = _sample_view("tgt", tgt, C)
    B, _, H, W = tgt.shape
    if pred.shape[0] != B or tuple(pred.shape[2:]) != (H, W):
        raise ValueError(f"pred {tuple(pred.shape)} and tgt {tuple(tgt.shape)} differ in batch or grid")
    check(lib.vv_err_accum(ctx.h, pp, ps, tp, ts, B, C, H, W, _f64_buf("cell", cell, (C, H, W)),
                           _f64_buf("chan", chan, (C,)), _stream()), "err_accum")


def err_finalize(ctx: Context, cell: torch.Tensor, n_samples: int, q_field=None, table: bool = True):
    """`error_var / total_step` (model/model.py:490) and its plane means (init_q_matrix q_type 0, da_4dvar.py:535-536)
    on the device (vv_err_finalize): returns (q_field, q_tab); q_field (C, H, W) float64 = cell / n_samples -- `q_field`
    when given (it may be `cell` itself), a new tensor for None, not computed for False --, q_tab (C,) float64 or None
    with table=False. No synchronisation."""
    C, H, W = cell.shape
    cp = _f64_buf("cell", cell, (C, H, W))
    if q_field is None:
        q_field = torch.empty_like(cell)
    elif q_field is False:
        q_field = None
    q_tab = torch.empty(C, device=cell.device, dtype=torch.float64) if table else None
    check(lib.vv_err_finalize(ctx.h, cp, int(n_samples), C, H, W, _f64_buf("q_field", q_field, (C, H, W)),
                              _f64_buf("q_tab", q_tab, (C,)), _stream()), "err_finalize")
    return q_field, q_tab


def r_fill(ctx: Context, rtab, Hs: int, Ws: int, interp=None, out=None, device: int = 0):
    """The dense static R on the device from its (T, C) fp32 table (vv_r_fill; get_static_info, da_4dvar.py:630-634):
    R (T, C, Hs, Ws), or with the (n_out, n_in) level operator `interp` R (T, 4 + 5*n_out, Hs, Ws), the bits of
    obs_augment of the broadcast field (get_R_matrix_from_gt, :729-756). rtab: numpy or torch (a host table is
    uploaded: T*C floats). out: an optional device buffer to overwrite. No synchronisation."""
    dev = out.device if out is not None else (rtab.device if isinstance(rtab, torch.Tensor) and rtab.is_cuda
                                              else torch.device("cuda", device))
    rt = _dev_table(rtab, dev)
    if rt.dim() != 2:
        raise ValueError(f"rtab must be (T, C), got {tuple(rt.shape)}")
    T, C = rt.shape
    interp, n_out, n_in = _level_operator(interp, C, dev, "the table has ")
    shape = (T, 4 + 5 * n_out if interp is not None else C, int(Hs), int(Ws))
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != shape:
        raise ValueError(f"out must be {shape}, got {tuple(out.shape)}")
    check(lib.vv_r_fill(ctx.h, _ptr(rt), None if interp is None else _ptr(interp), n_out, n_in, T, C, int(Hs), int(Ws),
                        _ptr(out), _stream()), "r_fill")
    return out


# rows of an obs_stats table (include/vaevar.h VV_OSTAT_*)
(OSTAT_COUNT, OSTAT_H, OSTAT_OB, OSTAT_OA, OSTAT_OB2, OSTAT_OA2, OSTAT_OAOB, OSTAT_R, OSTAT_JB,
 OSTAT_JA) = range(10)
OSTAT_N = 10
OSTAT_NAMES = ("count", "h", "ob", "oa", "ob2", "oa2", "oaob", "r", "jb", "ja")


def obs_stats(ctx: Context, xb_win: torch.Tensor, xa_win, yo: torch.Tensor, H: torch.Tensor, R: torch.Tensor,
              interp=None, out=None):
    """The departure moments of a window on the device (vv_obs_stats): per time level and observation channel the fp64
    sums, over the entries with H != 0, of 1, h, d_b, d_a, d_b^2, d_a^2, d_a d_b, r and the J_o terms h d^2 / r (rows
    OSTAT_*), d_b = yo - Op(xb_win), d_a = yo - Op(xa_win). xb_win, xa_win: (T, C, Hs, Ws) fp32 device states, xa_win
    may be None (its four rows are NaN); yo, H, R: (T, C_obs, Hs, Ws); interp (n_out, n_in) or None (identity).
    Returns the (T, C_obs, 10) float64 device tensor, `out` when given. calib.DepartureStats turns tables into the
    Desroziers estimates. No synchronisation."""
    for name, t in (("xb_win", xb_win), ("xa_win", xa_win), ("yo", yo), ("H", H), ("R", R)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dim() == 4 and t.dtype == torch.float32):
            raise ValueError(f"{name} must be a (T, channels, Hs, Ws) float32 tensor")
    T, C, Hs, Ws = xb_win.shape
    if xa_win is not None and xa_win.shape != xb_win.shape:
        raise ValueError(f"xa_win {tuple(xa_win.shape)} and xb_win {tuple(xb_win.shape)} differ")
    interp, n_out, n_in = _level_operator(interp, C, xb_win.device)
    c_obs = 4 + 5 * n_out if interp is not None else C
    shape = (T, c_obs, Hs, Ws)
    for name, t in (("yo", yo), ("H", H), ("R", R)):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    if out is None:
        out = torch.empty(T, c_obs, OSTAT_N, device=xb_win.device, dtype=torch.float64)
    check(lib.vv_obs_stats(ctx.h, _ptr(xb_win), None if xa_win is None else _ptr(xa_win), _ptr(yo), _ptr(H), _ptr(R),
                           None if interp is None else _ptr(interp), n_out, n_in, T, C, Hs, Ws,
                           _f64_buf("out", out, (T, c_obs, OSTAT_N)), _stream()), "obs_stats")
    return out


VAE_MEAN = 1  # include/vaevar.h VV_VAE_MEAN


def vae_sample(ctx: Context, enc_out: torch.Tensor, seed: int = 0, draw: int = 0, mean: bool = False, z=None,
               stat=None, want_z: bool = True):
    """`sampling` of nf_model/vae.py:78-81 and the KLD summand of :106 in one pass over the encoder output
    (vv_vae_sample). enc_out: a contiguous (B, 2L, H, W) fp32 device tensor, mu = enc_out[:, :L], log_var =
    enc_out[:, L:]. Returns (z, stat): z (B, L, H, W) fp32 = eps * exp(log_var / 2) + mu with eps the stream of
    normal_fill(seed, draw), or mu itself with mean=True (a new tensor, `z` when given, None with want_z=False);
    stat a (B, L, 4) float64 device tensor to OVERWRITE with the plane sums of 1 + lv - mu^2 - e^lv, mu, mu^2 and e^lv,
    or None. No synchronisation."""
    if not (enc_out.is_cuda and enc_out.dtype == torch.float32 and enc_out.dim() == 4 and enc_out.is_contiguous() and
            enc_out.shape[1] % 2 == 0):
        raise ValueError(f"enc_out must be a contiguous (B, 2L, H, W) float32 device tensor, got "
                         f"{tuple(enc_out.shape)} {enc_out.dtype}")
    B, L2, H, W = enc_out.shape
    L = L2 // 2
    if z is None and want_z:
        z = torch.empty(B, L, H, W, device=enc_out.device, dtype=torch.float32)
    if z is not None and tuple(z.shape) != (B, L, H, W):
        raise ValueError(f"z must be {(B, L, H, W)}, got {tuple(z.shape)}")
    check(lib.vv_vae_sample(ctx.h, _ptr(enc_out), B, L, H, W, int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF,
                            VAE_MEAN if mean else 0, None if z is None else _ptr(z),
                            _f64_buf("stat", stat, (B, L, 4)), _stream()), "vae_sample")
    return z, stat


def vae_sse(ctx: Context, recon: torch.Tensor, x: torch.Tensor, out=None, C: int | None = None):
    """The reconstruction term of loss_function (nf_model/vae.py:105; vv_vae_sse) per sample and channel: a (B, C)
    float64 device tensor of sum((recon - x)^2), the squares formed in fp32 as the reference forms them, the sum in
    fp64. recon, x: (B, >= C, H, W) fp32 device tensors or views with contiguous samples (err_accum's layouts).
    No synchronisation."""
    C = int(x.shape[1] if C is None else C)
    rp, rs = _sample_view("recon", recon, C)
    xp, xs = _sample_view("x", x, C)
    B, _, H, W = x.shape
    if recon.shape[0] != B or tuple(recon.shape[2:]) != (H, W):
        raise ValueError(f"recon {tuple(recon.shape)} and x {tuple(x.shape)} differ in batch or grid")
    if out is None:
        out = torch.empty(B, C, device=x.device, dtype=torch.float64)
    check(lib.vv_vae_sse(ctx.h, rp, rs, xp, xs, B, C, H, W, _f64_buf("out", out, (B, C)), _stream()), "vae_sse")
    return out


def err_sample(ctx: Context, pred: torch.Tensor, tgt: torch.Tensor, err_std: torch.Tensor, size=None, out=None,
               C: int | None = None):
    """The VAE's training sample (model/model.py:593-596; vv_err_sample): (tgt - pred) / err_std[c], nearest-resampled
    to `size` (default: the input grid), as a (B, C, Hn, Wn) fp32 device tensor holding the reference's bits. pred,
    tgt: (B, >= C, Hs, Ws) fp32 device tensors or views with contiguous samples; err_std: (C,) fp32 on the device.
    No synchronisation."""
    C = int(tgt.shape[1] if C is None else C)
    pp, ps = _sample_view("pred", pred, C)
    tp, ts = _sample_view("tgt", tgt, C)
    B, _, Hs, Ws = tgt.shape
    if pred.shape[0] != B or tuple(pred.shape[2:]) != (Hs, Ws):
        raise ValueError(f"pred {tuple(pred.shape)} and tgt {tuple(tgt.shape)} differ in batch or grid")
    if tuple(err_std.shape) != (C,):
        raise ValueError(f"err_std must be ({C},), got {tuple(err_std.shape)}")
    Hn, Wn = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))
    if out is None:
        out = torch.empty(B, C, Hn, Wn, device=tgt.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, C, Hn, Wn):
        raise ValueError(f"out must be {(B, C, Hn, Wn)}, got {tuple(out.shape)}")
    check(lib.vv_err_sample(ctx.h, pp, ps, tp, ts, B, C, Hs, Ws, _ptr(err_std), Hn, Wn, _ptr(out), _stream()),
          "err_sample")
    return out


def tri_interp(ctx: Context, tris: torch.Tensor, yo: torch.Tensor, H: torch.Tensor, xa: torch.Tensor,
               stats: bool = True):
    """The linear griddata analysis of da_mode 'interpolation' (da_4dvar.py:1016-1030; vv_tri_interp) IN PLACE on xa
    (C, Hs, Ws), which holds the background in observation space: the simplices of `tris` (the int32 device table of
    interp.pack_triangles, (n, interp.TRI_COLS)) are rasterised into the cells with H == 0 from the vertex values in
    yo; yo, H (C, Hs, Ws) are time level 0 of the observations and their mask. Returns the (3,) int64 device tensor
    rows used / rows skipped / cells written, or None with stats=False. No synchronisation."""
    from .interp import TRI_COLS

    if not (tris.is_cuda and tris.dtype == torch.int32 and tris.is_contiguous() and tris.dim() == 2 and
            tris.shape[1] == TRI_COLS):
        raise ValueError(f"tris must be a contiguous (n, {TRI_COLS}) int32 device tensor")
    if xa.dim() != 3 or yo.shape != xa.shape or H.shape != xa.shape:
        raise ValueError(f"yo, H and xa must share one (C, Hs, Ws) shape, got {tuple(yo.shape)} {tuple(H.shape)} "
                         f"{tuple(xa.shape)}")
    C, Hs, Ws = xa.shape
    out = torch.empty(3, device=xa.device, dtype=torch.int64) if stats else None
    n = tris.shape[0]
    check(lib.vv_tri_interp(ctx.h, ctypes.c_void_p(tris.data_ptr()) if n else None, n, _ptr(yo), _ptr(H), _ptr(xa), C,
                            Hs, Ws, None if out is None else ctypes.c_void_p(out.data_ptr()), _stream()), "tri_interp")
    return out


def obs_project(ctx: Context, interp_inv: torch.Tensor, x_aug: torch.Tensor) -> torch.Tensor:
    """x (T, 4 + 5*n_out, H, W) from the observation-space fields x_aug (T, 4 + 5*n_in, H, W) with the (n_out, n_in)
    obs_interpolater.interp_inv (da_4dvar.py:1033-1044; vv_obs_project), the inverse direction of obs_augment."""
    T, C, Hs, Ws = x_aug.shape
    interp_inv, n_out, n_in = _level_operator(interp_inv, C, x_aug.device)
    x_aug = x_aug.contiguous()
    out = torch.empty(T, 4 + 5 * n_out, Hs, Ws, device=x_aug.device, dtype=torch.float32)
    check(lib.vv_obs_project(ctx.h, _ptr(interp_inv), n_out, n_in, _ptr(x_aug), _ptr(out), T, Hs, Ws, _stream()),
          "obs_project")
    return out
