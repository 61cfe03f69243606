"""vv_obs_error timing (development tool): the call time of the held-out verification at 204 x 721 x 1440
(13 -> 40 levels) by device events, for masks of 5 %, 30 % and 100 % of the pixels (random pixels) and a 5 % mask of
8 x 8 pixel clusters, with the algorithmic bytes of each; writes $VV_OUT/obs_error_time.json (default bench_out/)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-var_amd"))
import numpy as np
import torch

from vaevar.engine import Context
from vaevar.metrics import Metrics
from vaevar.problem import ObsInterpolater

Hs, Ws, C, CA = 721, 1440, 69, 204
g = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn(C, Hs, Ws, device="cuda", generator=g)
yo = torch.randn(CA, Hs, Ws, device="cuda", generator=g)
H = (torch.rand(CA, Hs, Ws, device="cuda", generator=g) < 0.3).float()
interp = torch.from_numpy(ObsInterpolater(13, 40).interp).cuda()
m = Metrics(Context.get(0))
u = torch.rand(Hs, Ws, device="cuda", generator=g)
masks = {"5pct": (u < 0.05).float(), "30pct": (u < 0.3).float(), "100pct": torch.ones(Hs, Ws, device="cuda")}
ub = torch.rand((Hs + 7) // 8, (Ws + 7) // 8, device="cuda", generator=g) < 0.05
masks["5pct_8x8"] = ub.repeat_interleave(8, 0).repeat_interleave(8, 1)[:Hs, :Ws].float().contiguous()
out = {"shape": [CA, Hs, Ws], "device": torch.cuda.get_device_name(0), "lib_version": None, "cases": {}}
from vaevar._lib import lib

out["lib_version"] = lib.vv_version()
N = 200
for name, mask in masks.items():
    for _ in range(10):
        e = m.obs_error(x, yo, H, mask, interp)
    torch.cuda.synchronize()
    reps = []
    for r in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(N):
            e = m.obs_error(x, yo, H, mask, interp)
        b.record()
        torch.cuda.synchronize()
        reps.append(a.elapsed_time(b) / N * 1e3)
    frac = float(mask.mean())
    npx = Hs * Ws
    bytes_skip = 4.0 * npx + 4.0 * frac * npx * (1 + C + 2 * CA)
    bytes_dense = 4.0 * npx * (1 + C + 2 * CA)
    out["cases"][name] = {"mask_fraction": frac, "us_per_call_reps": reps, "us_per_call_median": float(np.median(reps)),
                          "algorithmic_bytes_with_skip": bytes_skip, "algorithmic_bytes_without_skip": bytes_dense,
                          "finite_channels": int(torch.isfinite(e).sum())}
    print(name, out["cases"][name], flush=True)
out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "bench_out"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "obs_error_time.json"), "w") as f:
    json.dump(out, f, indent=1)
