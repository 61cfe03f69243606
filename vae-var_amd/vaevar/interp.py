"""da_mode 'interpolation' (one_step_DA, da_4dvar.py:968-1061): the no-model baseline the analyses are judged
against. Per observation channel the reference triangulates the observed cells of time level 0 and fills every
unobserved cell inside their hull with scipy.interpolate.griddata(..., method='linear'); for obs_type real* the
background goes to the 40 observation levels first (obs_interp.interp) and the result comes back to the 13 model
levels with obs_interp.interp_inv.

The split: the host triangulates (scipy.spatial.Delaunay of a channel's observed cells, exactly what griddata runs
inside LinearNDInterpolator; only the cells' coordinates come back from the device), the device does everything
dense: the augmentation (vv_obs_augment), the rasterisation of the simplices into the field with exact integer edge
functions (vv_tri_interp), the back-projection (vv_obs_project) and the metrics (vv_metrics).

Quirks of the reference that are kept:
  * an observed cell keeps the BACKGROUND, not its observation (xa[i][b == 0] = ..., :1027);
  * a channel with <= 10 observed cells is left alone (:1025);
  * the coordinates are plain (row, column) indices: no longitude wrap, no metric on the sphere;
  * only time level 0 of yo and H is used (:983-984).
The one divergence: without an observation operator the reference's `for i in range(204)` (:1017) raises IndexError
on a state of fewer channels; here every channel of the state is interpolated."""
from __future__ import annotations

import time

import numpy as np
import torch

from .engine import Context, obs_augment, obs_project, tri_interp

TRI_COLS, TRI_BAND, TRI_SEG = 12, 16, 64  # VV_TRI_COLS, VV_TRI_BAND, VV_TRI_SEG (include/vaevar.h)
MIN_CELLS = 10                            # `if len(known_values) > 10` (:1025)


def delaunay(points: np.ndarray):
    """(simplices, neighbors) of scipy.spatial.Delaunay(points) with its default options, as griddata builds it.
    scipy is imported here, on the first use. A QhullError (all cells collinear) propagates, as in the reference."""
    from scipy.spatial import Delaunay

    tri = Delaunay(points)
    return tri.simplices, tri.neighbors


def pack_triangles(coords_by_channel, triangulate=None) -> np.ndarray:
    """The simplex table of vv_tri_interp: an (n, TRI_COLS) int32 array

        ch r0 c0 r1 c1 r2 c2 nb0 nb1 nb2 work_begin work_end

    coords_by_channel[ch] is the (k, 2) integer array of the channel's observed (row, column) cells in np.argwhere
    (row-major) order, or None / empty. A channel with <= MIN_CELLS cells gets no rows. triangulate(points) returns
    (simplices (m, 3), neighbors (m, 3)) as scipy.spatial.Delaunay has them (neighbors[i][k] across the edge opposite
    vertex k, -1 on the hull); default `delaunay`. Channels with the same cell list share one triangulation. The rows
    of a channel are contiguous and in the triangulation's order; nbk is offset to table rows. The last two columns
    number the (simplex, tile) work items of the device: a bounding box is cut into TRI_BAND x TRI_SEG tiles."""
    if triangulate is None:
        triangulate = delaunay
    shared: dict = {}
    blocks, tiles, n_rows = [], [], 0
    for ch, pts in enumerate(coords_by_channel):
        if pts is None:
            continue
        pts = np.ascontiguousarray(pts, np.int64)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError(f"channel {ch}: cells must be (k, 2) (row, column), got {pts.shape}")
        if len(pts) <= MIN_CELLS:
            continue
        key = pts.tobytes()
        if key not in shared:  # the vertex columns and the tile counts are the triangulation's, whatever the channel
            simp, nbr = triangulate(pts)
            simp, nbr = np.asarray(simp, np.int64).reshape(-1, 3), np.asarray(nbr, np.int64).reshape(-1, 3)
            base = np.zeros((len(simp), TRI_COLS), np.int32)
            for k in range(3):
                base[:, 1 + 2 * k], base[:, 2 + 2 * k] = pts[simp[:, k], 0], pts[simp[:, k], 1]
            rows, cols = base[:, 1:7:2].astype(np.int64), base[:, 2:7:2].astype(np.int64)
            shared[key] = (base, nbr, ((rows.max(1) - rows.min(1)) // TRI_BAND + 1)
                           * ((cols.max(1) - cols.min(1)) // TRI_SEG + 1))
        base, nbr, t = shared[key]
        blk = base.copy()
        blk[:, 0] = ch
        blk[:, 7:10] = np.where(nbr >= 0, nbr + n_rows, -1)
        blocks.append(blk)
        tiles.append(t)
        n_rows += len(blk)
        if n_rows >= 2 ** 31:
            raise ValueError(f"{n_rows} simplices: the table is int32")
    if not blocks:
        return np.zeros((0, TRI_COLS), np.int32)
    tab, tiles = np.concatenate(blocks), np.concatenate(tiles)
    end = np.cumsum(tiles)
    if end[-1] >= 2 ** 31:
        raise ValueError(f"{n_rows} simplices in {int(end[-1])} tiles: the table is int32")
    tab[:, 10], tab[:, 11] = end - tiles, end
    return tab


def observed_cells(H0: torch.Tensor):
    """The observed cells of H0 (C, Hs, Ws) on the device, `np.argwhere(b == 1)` per channel (:1022): only the
    coordinates cross PCIe. Returns a list of C (k, 2) int64 arrays (row-major order)."""
    nz = torch.nonzero(H0 == 1).cpu().numpy()  # sorted by (channel, row, column)
    cut = np.searchsorted(nz[:, 0], np.arange(H0.shape[0] + 1))
    return [nz[cut[c]:cut[c + 1], 1:] for c in range(H0.shape[0])]


def one_step_interpolation(ctx: Context, xb, yo, H, obs_interp=None, gt=None, metrics=None, mask_eval=None,
                           triangulate=None) -> dict:
    """one_step_DA(gt, xb, yo, H, R, 'interpolation') (da_4dvar.py:968-1061) on the device.

    xb (C, Hs, Ws) the background; yo, H (T, C_obs, Hs, Ws), of which time level 0 is used; mask_eval (Hs, Ws): the
    --use_eval split H <- H * (1 - mask_eval) (:934-937). obs_interp: an ObsInterpolater (obs_type real*: C = 4 +
    5*dim_in, C_obs = 4 + 5*dim_out; the background is augmented, interpolated in observation space and projected
    back with interp_inv) or None (C_obs = C, every channel interpolated as it is: the one divergence, module
    docstring). With gt (T, C, Hs, Ws) and metrics (vaevar.metrics.Metrics) the bg_* and ana_* WRMSE / Bias / MSE of
    :972-980 and :1049-1058 are returned in "metrics" as {"bg": (wrmse, bias, mse), "ana": ...}; there is no error_obs
    in this mode. Returns xa (C, Hs, Ws), xa_aug (C_obs, Hs, Ws), stats (the (3,) int64 device tensor rows used / rows
    skipped / cells written), metrics, and the host seconds spent triangulating ("seconds_triangulate")."""
    dev = torch.device("cuda", ctx.device)

    def t(a):
        if isinstance(a, torch.Tensor):
            return a.to(device=dev, dtype=torch.float32).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)

    xb, yo, H = t(xb), t(yo), t(H)
    if xb.dim() != 3 or yo.dim() != 4 or H.shape != yo.shape:
        raise ValueError(f"xb (C, Hs, Ws) and yo, H (T, C_obs, Hs, Ws) expected, got {tuple(xb.shape)} "
                         f"{tuple(yo.shape)} {tuple(H.shape)}")
    H0 = H[0]
    if mask_eval is not None:
        H0 = H0 * (1 - t(mask_eval))
    out = {"metrics": None}
    if gt is not None and metrics is not None:
        gt0 = t(gt)[0]
        w, b = metrics.wrmse_bias(xb, gt0)
        out["metrics"] = {"bg": (w.cpu().numpy(), b.cpu().numpy(), metrics.mse(xb, gt0))}
    if obs_interp is not None:
        xa_aug = obs_augment(ctx, torch.as_tensor(obs_interp.interp), xb.unsqueeze(0))[0]
    else:
        xa_aug = xb.clone()
    if xa_aug.shape != yo.shape[1:]:
        raise ValueError(f"yo has channels and grid {tuple(yo.shape[1:])}, the background in observation space "
                         f"{tuple(xa_aug.shape)}: pass the observation operator (obs_interp)")
    t0 = time.time()
    table = pack_triangles(observed_cells(H0), triangulate)
    out["seconds_triangulate"] = time.time() - t0
    out["stats"] = tri_interp(ctx, torch.from_numpy(table).to(dev), yo[0].contiguous(), H0.contiguous(), xa_aug)
    if obs_interp is not None:
        xa = obs_project(ctx, torch.as_tensor(obs_interp.interp_inv), xa_aug.unsqueeze(0))[0]
    else:
        xa = xa_aug
    out["xa"], out["xa_aug"] = xa, xa_aug
    if out["metrics"] is not None:
        w, b = metrics.wrmse_bias(xa, gt0)
        out["metrics"]["ana"] = (w.cpu().numpy(), b.cpu().numpy(), metrics.mse(xa, gt0))
    return out
