"""vv_obs_qc timing (development tool): the call time of the real-observation quality control at
204 x 721 x 1440 (13 -> 40 levels), T = 1, by device events, for station masks of 1 % random entries, 1 % in 8 x 8 pixel
clusters and 100 %, with the flags of obs_type 'real' and 'real_simu'; next to it, in the same run, the device
composition of the same steps from the existing pieces (vv_obs_augment + torch element-wise ops) with its peak
temporary memory. Median of five repeats of 200 queued calls. The kernel works in place, so a repeated call sees the
filtered mask of the one before: it is timed both that way ("steady") and with yo and H restored before every call, the
time of the restoring copies alone subtracted ("fresh"); the composition is not in place and is timed plainly.
Writes $VV_OUT/obs_qc_time.json (default bench_out/)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-var_amd"))
import numpy as np
import torch

from vaevar import config as Cf
from vaevar._lib import lib
from vaevar.engine import Context, obs_augment, obs_qc
from vaevar.problem import ObsInterpolater, qc_flags, qc_threshold

Hs, Ws, C, CA, NOUT = 721, 1440, 69, 204, 40
N, REPS = int(os.environ.get("VV_QC_CALLS", 200)), 5
ctx = Context.get(0)
g = torch.Generator(device="cuda").manual_seed(1)
interp_np = ObsInterpolater(13, NOUT).interp
interp = torch.from_numpy(interp_np).cuda()
thr = qc_threshold(0.1, interp_np, Cf.MODEL_STD).cuda()
mean = torch.tensor(Cf.MODEL_MEAN, device="cuda").reshape(1, -1, 1, 1)
std = torch.tensor(Cf.MODEL_STD, device="cuda").reshape(1, -1, 1, 1)
gt = mean + std * torch.randn(1, C, Hs, Ws, device="cuda", generator=g)
# departures of 0 .. 2 thresholds, either sign: half of the observed entries are rejected
yo0 = obs_augment(ctx, interp, gt)
yo0 += (4 * torch.rand(1, CA, Hs, Ws, device="cuda", generator=g) - 2) * thr.reshape(1, -1, 1, 1)
masks = {"1pct": (torch.rand(1, CA, Hs, Ws, device="cuda", generator=g) < 0.01).float()}
ub = torch.rand(1, CA, (Hs + 7) // 8, (Ws + 7) // 8, device="cuda", generator=g) < 0.01
masks["1pct_8x8"] = ub.repeat_interleave(8, 2).repeat_interleave(8, 3)[..., :Hs, :Ws].float().contiguous()
del ub
masks["100pct"] = torch.ones(1, CA, Hs, Ws, device="cuda")


def composed(yo, H, flags):
    """get_obs_info's steps (da_4dvar.py:770-798) from the existing pieces; returns (yo', H', counts)."""
    gt_aug = obs_augment(ctx, interp, gt)
    before = H.sum((1, 2, 3), dtype=torch.float64)
    if flags & 1:
        t = thr.reshape(1, -1, 1, 1)
        d = yo - gt_aug
        mask = ((d < t) & (d > -t)).float()
    else:
        mask = torch.ones_like(yo)
    Hn = H * mask
    after = Hn.sum((1, 2, 3), dtype=torch.float64)
    if flags & 4:
        yo = gt_aug * Hn
    return yo, Hn, torch.stack([before, after], 1)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(N):
            fn()
        b.record()
        torch.cuda.synchronize()
        reps.append(a.elapsed_time(b) / N * 1e3)
    return reps


out = {"shape": [1, CA, Hs, Ws], "device": torch.cuda.get_device_name(0), "lib_version": lib.vv_version(),
       "calls_per_repeat": N, "cases": {}}
yo, H = torch.empty_like(yo0), torch.empty_like(yo0)


def restore(H0):
    H.copy_(H0)
    yo.copy_(yo0)


for name, H0 in masks.items():
    share = float(H0.mean())
    t_restore = timed(lambda: restore(H0))
    for obs_type in ("real", "real_simu"):
        flags = qc_flags(obs_type)
        restore(H0)
        cnt = obs_qc(ctx, gt, yo, H, interp, thr, flags)
        yo_c, H_c, cnt_c = composed(yo0, H0, flags)
        same = bool(torch.equal(H, H_c) and torch.equal(yo, yo_c) and torch.equal(cnt, cnt_c))
        del yo_c, H_c
        t_steady = timed(lambda: obs_qc(ctx, gt, yo, H, interp, thr, flags))
        t_fresh = timed(lambda: (restore(H0), obs_qc(ctx, gt, yo, H, interp, thr, flags)))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t_comp = timed(lambda: composed(yo0, H0, flags))
        peak = torch.cuda.max_memory_allocated() - base
        fresh = float(np.median(t_fresh) - np.median(t_restore))
        field = 4.0 * CA * Hs * Ws
        simu, filt = bool(flags & 4), bool(flags & 1)
        # H densely; per observed entry its yo (filter) and, at worst, one level column per entry; yo' densely (simu)
        # or H' at the rejected entries only
        kernel_bytes = field * (1 + share * (filt + 13.0 / NOUT) + (1.0 if simu else 0.0) + 0.5 * share * filt)
        r = {"station_share": share, "flags": flags, "counts": cnt.cpu().tolist(), "bitwise_equal_to_composition": same,
             "kernel_us_steady_reps": t_steady, "kernel_us_steady_median": float(np.median(t_steady)),
             "restore_us_median": float(np.median(t_restore)), "kernel_plus_restore_us_median": float(np.median(t_fresh)),
             "kernel_us_fresh": fresh, "composition_us_reps": t_comp, "composition_us_median": float(np.median(t_comp)),
             "composition_over_kernel_fresh": float(np.median(t_comp)) / fresh,
             "composition_over_kernel_steady": float(np.median(t_comp) / np.median(t_steady)),
             "composition_peak_temporary_bytes": int(peak), "kernel_algorithmic_bytes": kernel_bytes,
             "field_bytes": field}
        out["cases"][f"{name}/{obs_type}"] = r
        print(name, obs_type, r, flush=True)
out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "bench_out"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "obs_qc_time.json"), "w") as f:
    json.dump(out, f, indent=1)
