"""vv_obs_stats timing (development tool): the call time of the departure statistics of a T = 6 window at
204 x 721 x 1440 observation channels (13 -> 40 levels), by device events, for masks of 1 % random entries
(station-like) and 100 %, with and without the analysis window. Next to it, in the same run, the baseline: the same table composed on
the device from vv_obs_augment and torch fp64 reductions, which is what a user would write without the kernel, with
its peak temporary memory. Every call is timed on its own (25 calls after 3 warm-up calls, buffers allocated once):
median (min .. max). One box, one run. Writes profiles/r13/obs_stats.json, or $VV_OUT/obs_stats.json when VV_OUT is
set."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-var_amd"))
import numpy as np
import torch

from vaevar import config as Cf
from vaevar._lib import lib
from vaevar.engine import Context, obs_augment, obs_stats
from vaevar.problem import ObsInterpolater

T, Hs, Ws, C, CA, NOUT = int(os.environ.get("VV_OSTAT_T", 6)), 721, 1440, 69, 204, 40
CALLS, WARM = 25, 3
ctx = Context.get(0)
g = torch.Generator(device="cuda").manual_seed(1)
interp_np = ObsInterpolater(13, NOUT).interp
interp = torch.from_numpy(interp_np).cuda()
mean = torch.tensor(Cf.MODEL_MEAN, device="cuda").reshape(1, -1, 1, 1)
std = torch.tensor(Cf.MODEL_STD, device="cuda").reshape(1, -1, 1, 1)
xb = mean + std * torch.randn(T, C, Hs, Ws, device="cuda", generator=g)
xa = xb + 0.1 * std * torch.randn(T, C, Hs, Ws, device="cuda", generator=g)
s_aug = obs_augment(ctx, interp, std.expand(1, C, 1, 1).contiguous()).abs()
yo = obs_augment(ctx, interp, xa)
yo += 0.1 * s_aug * torch.randn(T, CA, Hs, Ws, device="cuda", generator=g)
R = ((0.1 * s_aug) ** 2).expand(T, CA, Hs, Ws).contiguous()
masks = {"1pct": (torch.rand(T, CA, Hs, Ws, device="cuda", generator=g) < 0.01).float(),
         "100pct": torch.ones(T, CA, Hs, Ws, device="cuda")}
out_buf = torch.empty(T, CA, 10, device="cuda", dtype=torch.float64)


def composed(H, with_a):
    """The table from the existing pieces: obs_augment, torch element-wise ops and fp64 reductions."""
    obs = H != 0
    f64 = dict(dim=(2, 3), dtype=torch.float64)
    zero = torch.zeros((), device=H.device)
    nan = torch.full((T, CA), float("nan"), device=H.device, dtype=torch.float64)
    rows = {"count": obs.sum(**f64), "h": H.sum(**f64), "r": torch.where(obs, R, zero).sum(**f64)}
    d = {}
    for k, x in (("b", xb), ("a", xa if with_a else None)):
        if x is None:
            rows.update({"oa": nan, "oa2": nan, "oaob": nan, "ja": nan})
            continue
        dk = torch.where(obs, yo - obs_augment(ctx, interp, x), zero)
        d[k] = dk.double()
        rows["o" + k] = d[k].sum((2, 3))
        rows[f"o{k}2"] = (d[k] * d[k]).sum((2, 3))
        rows["j" + k] = torch.where(obs, (H * (dk * dk)) / R, zero).sum(**f64)
    if with_a:
        rows["oaob"] = (d["a"] * d["b"]).sum((2, 3))
    return torch.stack([rows[k] for k in ("count", "h", "ob", "oa", "ob2", "oa2", "oaob", "r", "jb", "ja")], 2)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls": CALLS}


out = {"shape": {"T": T, "C": C, "C_obs": CA, "Hs": Hs, "Ws": Ws}, "device": torch.cuda.get_device_name(0),
       "lib_version": lib.vv_version(), "note": "one box, one run; every call timed on its own by device events",
       "cases": {}}
for name, H in masks.items():
    for with_a in (True, False):
        a_win = xa if with_a else None
        tab = obs_stats(ctx, xb, a_win, yo, H, R, interp, out=out_buf).clone()
        ref = composed(H, with_a)
        scale = ref.abs().amax((0, 1), keepdim=True).clamp_min(1e-300)
        diff = float(((tab - ref).abs() / scale).nan_to_num(0.0).max())
        nan_same = bool(torch.equal(tab.isnan(), ref.isnan()))
        del ref
        k = timed(lambda: obs_stats(ctx, xb, a_win, yo, H, R, interp, out=out_buf))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        c = timed(lambda: composed(H, with_a))
        peak = torch.cuda.max_memory_allocated() - base
        r = {"observed_share": float(H.mean()), "with_xa": with_a, "kernel": k, "composition": c,
             "composition_over_kernel": c["median_ms"] / k["median_ms"],
             "composition_peak_temporary_bytes": int(peak),
             "kernel_algorithmic_bytes_fully_observed": 4.0 * Hs * Ws * T * (3 * CA + (2 if with_a else 1) * C),
             "max_difference_over_largest_row_entry": diff, "nan_rows_agree": nan_same}
        out["cases"][f"{name}/{'xa' if with_a else 'no_xa'}"] = r
        print(name, "with xa" if with_a else "without xa", r, flush=True)
out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "profiles", "r13"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "obs_stats.json"), "w") as f:
    json.dump(out, f, indent=1)
