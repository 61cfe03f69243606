"""Make tests/golden/g18_interpolation.npz: what scipy's griddata(method='linear') and the REFERENCE's own
one_step_DA(..., 'interpolation') (da_4dvar.py:968-1061) make of small observation sets, stored sparsely. CPU only;
needs scipy and the reference tree that oracle.ref_harness imports (it is not part of this repository).

    python tools/make_interp_fixture.py

(a) Kernel cases, three grids (33 x 47, 67 x 131, 19 x 200) of eight channels each (CASES below). Per channel: the
    observed cells in np.argwhere order, their fp32 values, scipy.spatial.Delaunay's simplices and neighbors of those
    cells, and the genuine griddata result at the cells np.argwhere(mask == 0), cast to fp32 (NaN outside the hull);
    for the channel with a mask value that is neither 0 nor 1, that cell.
(b) One run of the reference's one_step_DA in mode 'interpolation', called unbound on a stub `self` with obs_type
    'real' and the reference's own obs_interpolater(13, 40): 204 observation channels on a 19 x 23 grid, most of them
    empty or with <= 10 cells, seven with masks of their own and two sharing one. torch.Tensor.cuda is the identity for
    the call (the reference moves its operator and its result to the GPU; nothing else of it needs one); the metric
    object is a stub, the mode's analysis does not depend on it (nor on the truth, which is not stored). Stored: xb, the
    sparse yo / H, both operator matrices, the triangulation of every mask with more than 10 cells, and the returned
    xa.
(c) The station masks of the cycle test (four channels on 32 x 64) with their triangulations, so that the GPU tests
    never run scipy."""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vae-var_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GRIDS = ((33, 47), (67, 131), (19, 200))
CASES = ("dense50", "clusters", "tracks", "corners", "few", "nan_vertex", "nonbinary", "clusters_again")


def clusters(rng, Hs, Ws, k, per, spread):
    m = np.zeros((Hs, Ws), bool)
    for _ in range(k):
        r0, c0 = rng.uniform(0, Hs), rng.uniform(0, Ws)
        rr = np.clip(np.round(rng.normal(r0, spread, per)), 0, Hs - 1).astype(int)
        cc = np.clip(np.round(rng.normal(c0, spread * 1.5, per)), 0, Ws - 1).astype(int)
        m[rr, cc] = True
    return m


def case_mask(name, rng, Hs, Ws):
    if name == "dense50":
        return rng.random((Hs, Ws)) < 0.5
    if name in ("clusters", "clusters_again"):
        return clusters(np.random.default_rng(4242 + Hs), Hs, Ws, 6, 14, 2.0)  # the same mask for both channels
    if name == "tracks":  # a ship along a row, one along a column, one on a diagonal, and a few stations
        m = clusters(rng, Hs, Ws, 2, 6, 1.5)
        m[Hs // 3, 2:Ws - 3:2] = True
        m[1:Hs - 1:3, (2 * Ws) // 3] = True
        k = np.arange(min(Hs, Ws) - 2)
        m[k + 1, k + 1] = True
        return m
    if name == "corners":  # 12 clustered cells and three far grid corners: one simplex box covers the grid
        m = np.zeros((Hs, Ws), bool)
        r0, c0 = Hs // 4, Ws // 2  # inside the corners' triangle, whose long edge then bounds a simplex
        for k in range(12):
            m[r0 + (k * 5) % 4, c0 + (k * 3) % 7] = True
        assert m.sum() == 12
        m[0, 0] = m[0, Ws - 1] = m[Hs - 1, Ws - 1] = True
        return m
    if name == "few":  # <= 10 cells: the channel must stay untouched
        m = np.zeros((Hs, Ws), bool)
        idx = rng.choice(Hs * Ws, 8, replace=False)
        m.flat[idx] = True
        return m
    if name == "nan_vertex":
        return rng.random((Hs, Ws)) < 0.05
    if name == "nonbinary":
        m = rng.random((Hs, Ws)) < 0.2
        m[0, 0] = m[Hs - 1, 0] = True  # hull corners
        return m
    raise KeyError(name)


def kernel_cases(out):
    from scipy.interpolate import griddata
    from scipy.spatial import Delaunay

    from _interp_ref import nan_safe_vertex

    for gi, (Hs, Ws) in enumerate(GRIDS):
        for ci, name in enumerate(CASES):
            rng = np.random.default_rng(1800 + 100 * gi + ci)
            m = case_mask(name, rng, Hs, Ws)
            H = m.astype(np.float32)
            key = f"a{gi}_c{ci}_"
            if name == "nonbinary":
                free = np.argwhere(~m)
                r, c = free[len(free) // 2]
                H[r, c] = 0.5
                out[key + "other"] = np.array([[r, c, 0.5]], np.float64)
            cells = np.argwhere(H == 1)
            scale, offset = ((30.0, 250.0), (3.0e3, 5.5e4), (8.0, 0.0))[ci % 3]
            vals = (offset + scale * rng.standard_normal(len(cells))).astype(np.float32)
            tri = Delaunay(cells) if len(cells) > 10 else None
            if name == "nan_vertex":  # at a vertex where griddata's answer does not depend on its walk
                vals[nan_safe_vertex(cells, tri.simplices, H)] = np.nan
            out[key + "cells"] = cells.astype(np.int16)
            out[key + "vals"] = vals
            if tri is not None:
                assert len(tri.coplanar) == 0
                out[key + "simp"] = tri.simplices.astype(np.int16)
                out[key + "nbr"] = tri.neighbors.astype(np.int16)
                lin = griddata(cells, vals, np.argwhere(H == 0), method="linear")
                out[key + "lin"] = lin.astype(np.float32)
            print(key, name, "cells", len(cells), "simplices", len(out.get(key + "simp", ())))


B_GRID = (19, 23)
# channel: density, > 10 cells each. 4 + 40 i + j is level j of variable i; all but channel 11 are levels that
# obs_interpolater.interp_inv reads (a non-zero column), so their interpolated cells reach xa
B_MASKS = {2: 0.3, 3: 0.12, 4: 0.5, 11: 0.2, 63: 0.08, 104: 0.25, 197: 0.15, 203: 0.2}
B_SHARED = (104, 144)    # u and v at level 20: channel 144 takes channel 104's mask
B_FEW = {0: 10, 60: 3, 120: 10, 202: 1}  # <= 10 cells: untouched


def reference_run(out):
    import torch
    from scipy.spatial import Delaunay

    from oracle import ref_harness

    ref_harness.import_reference()
    da = importlib.import_module("da_4dvar")
    from vaevar import config as C

    Hs, Ws = B_GRID
    rng = np.random.default_rng(1899)
    mean = np.asarray(C.MODEL_MEAN, np.float32)
    std = np.asarray(C.MODEL_STD, np.float32)
    xb = (mean[:, None, None] + std[:, None, None] * rng.standard_normal((69, Hs, Ws))).astype(np.float32)
    gt = (mean[:, None, None] + std[:, None, None] * rng.standard_normal((1, 69, Hs, Ws))).astype(np.float32)
    H = np.zeros((1, 204, Hs, Ws), np.float32)
    for ch, dens in B_MASKS.items():
        H[0, ch] = rng.random((Hs, Ws)) < dens
        assert H[0, ch].sum() > 10
    H[0, B_SHARED[1]] = H[0, B_SHARED[0]]
    for ch, k in B_FEW.items():
        H[0, ch].flat[rng.choice(Hs * Ws, k, replace=False)] = 1
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        oi = da.obs_interpolater(13, 40)
        # observations: the augmented truth plus noise, in observation space
        g = torch.from_numpy(gt)
        aug = [g[:, :4]] + [torch.nn.functional.linear(g[:, 4 + 13 * i:17 + 13 * i].transpose(1, 3),
                                                       oi.interp).transpose(1, 3) for i in range(5)]
        yo = (torch.cat(aug, 1).numpy() * (1 + 0.01 * rng.standard_normal(H.shape)).astype(np.float32)) * H
        yo = yo.astype(np.float32)
        zeros = lambda *a, **k: torch.zeros(69, dtype=torch.float64)  # noqa: E731
        stub = types.SimpleNamespace(
            use_eval=False, model_mean=torch.from_numpy(mean), model_std=torch.from_numpy(std),
            metric=types.SimpleNamespace(WRMSE=zeros, Bias=zeros), obs_type="real", nlev=13, obs_interp=oi,
            current_time="fixture",
            metrics_list={k: [] for k in ("bg_wrmse", "bg_bias", "bg_mse", "ana_wrmse", "ana_bias", "ana_mse")})
        xa = da.cyclic_4dvar.one_step_DA(stub, torch.from_numpy(gt), torch.from_numpy(xb), torch.from_numpy(yo),
                                         torch.from_numpy(H), None, "interpolation")
        interp, interp_inv = oi.interp.numpy().copy(), oi.interp_inv.numpy().copy()
    finally:
        torch.Tensor.cuda = cuda
    assert xa.shape == (69, Hs, Ws) and xa.dtype == torch.float32
    idx = np.flatnonzero(H)
    out.update(b_xb=xb, b_idx=idx.astype(np.int32), b_yo=yo.reshape(-1)[idx], b_xa=xa.numpy(),
               b_interp=interp, b_interp_inv=interp_inv, b_grid=np.array(B_GRID, np.int64))
    chans = []
    for ch in range(204):
        cells = np.argwhere(H[0, ch] == 1)
        if len(cells) > 10:
            tri = Delaunay(cells)
            assert len(tri.coplanar) == 0
            out[f"b_c{ch}_cells"] = cells.astype(np.int16)
            out[f"b_c{ch}_simp"], out[f"b_c{ch}_nbr"] = tri.simplices.astype(np.int16), tri.neighbors.astype(np.int16)
            chans.append(ch)
    out["b_channels"] = np.array(chans, np.int64)
    print("reference run: channels with rows", chans, "xa differs from xb in",
          int((xa.numpy() != xb).sum()), "cells")


def cycle_masks(out):
    """(c) station masks of a 4-channel 32 x 64 state for the cycle test: clusters, the same again, 10 % random, and a
    channel of 9 cells."""
    from scipy.spatial import Delaunay

    Hs, Ws = 32, 64
    rng = np.random.default_rng(1877)
    cl = clusters(rng, Hs, Ws, 5, 12, 2.0)
    few = np.zeros((Hs, Ws), bool)
    few.flat[rng.choice(Hs * Ws, 9, replace=False)] = True
    for ch, m in enumerate((cl, cl, rng.random((Hs, Ws)) < 0.1, few)):
        cells = np.argwhere(m)
        out[f"c_c{ch}_cells"] = cells.astype(np.int16)
        if len(cells) > 10:
            tri = Delaunay(cells)
            assert len(tri.coplanar) == 0
            out[f"c_c{ch}_simp"], out[f"c_c{ch}_nbr"] = tri.simplices.astype(np.int16), tri.neighbors.astype(np.int16)


def main():
    out = {}
    kernel_cases(out)
    cycle_masks(out)
    reference_run(out)
    path = os.path.join(ROOT, "tests", "golden", "g18_interpolation.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
