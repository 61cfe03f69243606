"""vv_obs_synth timing (development tool) at (T, 69, 721, 1440), T in {1, 6}, n_obs in {15000, 500000},
noise off and on: the median of VV_SYNTH_REPS (default 25, at least 20) event-timed calls after warm-up, buffers
allocated once. The selection is timed on its own as the same call on a (1, 1, 721, 1440) field (its fill moves 1/69
of one slot: an upper bound on the selection), the fill as the whole call minus that; bytes and GB/s for each. The host
path it replaces is timed in the same process by a host clock around a synchronised run: np.random.choice without
replacement, np.put, the stack over 69 channels and the broadcast over the window (da_4dvar.py:282-292), torch.randn
times sqrt(obs_var) when the noise is on (:449), the static R (:630-634), and the uploads of yo, H and R. No threshold
is asserted. Writes $VV_OUT/obs_synth.json (default profiles/r10/)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-var_amd"))
import numpy as np
import torch

from vaevar import config as Cf
from vaevar._lib import lib
from vaevar.engine import Context, obs_synth
from vaevar.problem import obs_variance, r_table

Hs, Ws, C = 721, 1440, 69
HW = Hs * Ws
REPS = max(20, int(os.environ.get("VV_SYNTH_REPS", 25)))
HOST_REPS = int(os.environ.get("VV_SYNTH_HOST_REPS", 2))
WINS = [int(x) for x in os.environ.get("VV_SYNTH_WINS", "1,6").split(",")]
AMOUNTS = [int(x) for x in os.environ.get("VV_SYNTH_AMOUNTS", "15000,500000").split(",")]
ctx = Context.get(0)
std = np.asarray(Cf.MODEL_STD, np.float32)
ov = obs_variance(C, 0.005, 2, std)
sd = np.sqrt(ov)


def events(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def host_path(gt, T, n_obs, noise):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    matrix = np.zeros((Hs, Ws), dtype=int)  # da_4dvar.py:282-292
    indices = np.random.choice(matrix.size, n_obs, replace=False)
    np.put(matrix, indices, 1)
    x = np.stack([matrix] * C)
    H = torch.zeros(T, C, Hs, Ws)
    H = H + torch.from_numpy(x)
    obs_var = torch.from_numpy(ov).reshape(C, 1, 1)
    yo = gt + torch.sqrt(obs_var) * torch.randn(T, C, Hs, Ws) if noise else gt  # :449
    R = torch.zeros(T, C, Hs, Ws)  # :630-634
    R[0] = obs_var
    for i in range(T - 1):
        R[i + 1] = obs_var + 0.0
    t1 = time.perf_counter()
    out = [a.to(torch.float32).cuda() for a in (yo, H, R)]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    del out
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


out = {"device": torch.cuda.get_device_name(0), "lib_version": lib.vv_version(), "repeats": REPS,
       "host_repeats": HOST_REPS,
       "note": "selection_ms: the same call on a (1, 1, 721, 1440) field; fill_ms = call_ms - selection_ms; "
               "fill bytes: gt read, yo, H and R written, plus the 0/1 plane read once",
       "cases": {}}
small = torch.zeros(1, 1, Hs, Ws, device="cuda")
small_out = (torch.empty_like(small), torch.empty_like(small), None)
for T in WINS:
    gt_h = torch.from_numpy(np.random.default_rng(7).standard_normal((T, C, Hs, Ws), dtype=np.float32))
    gt = gt_h.cuda()
    bufs = tuple(torch.empty_like(gt) for _ in range(3))
    rt = torch.from_numpy(r_table(ov, None, T)).cuda()
    sd_d = torch.from_numpy(sd).cuda()
    n = T * C * HW
    for n_obs in AMOUNTS:
        sel_ms, _ = events(lambda: obs_synth(ctx, small, n_obs, 1, 2, out=small_out))
        for noise in (False, True):
            call_ms, reps = events(lambda: obs_synth(ctx, gt, n_obs, 1, 2, sd=sd_d if noise else None, r_table=rt,
                                                     out=bufs))
            stats = obs_synth(ctx, gt, n_obs, 1, 2, r_table=rt, out=bufs)[3].cpu().tolist()
            host = [host_path(gt_h, T, n_obs, noise) for _ in range(HOST_REPS)]
            fill_ms = call_ms - sel_ms
            fill_bytes = 4 * n * 4 + 4 * HW
            sel_bytes = 4 * HW + 2 * 4 * ((HW + 1023) // 1024) + 3 * 2048 * 4
            r = {"shape": [T, C, Hs, Ws], "n_obs": n_obs, "noise": noise, "stats": stats,
                 "call_ms_median": call_ms, "call_ms_min": float(min(reps)), "call_ms_max": float(max(reps)),
                 "selection_ms_median": sel_ms, "selection_bytes": sel_bytes,
                 "selection_GBps": sel_bytes / sel_ms * 1e-6, "selection_keys_per_us": 5 * HW / sel_ms * 1e-3,
                 "fill_ms": fill_ms, "fill_bytes": fill_bytes, "fill_GBps": fill_bytes / fill_ms * 1e-6,
                 "fill_fraction_of_8TBps": fill_bytes / fill_ms * 1e-6 / 8000.0,
                 "host_build_ms_reps": [h[0] for h in host], "host_upload_ms_reps": [h[1] for h in host],
                 "host_total_ms_median": float(np.median([h[0] + h[1] for h in host])),
                 "host_dense_bytes_uploaded": 3 * 4 * n}
            r["host_over_device"] = r["host_total_ms_median"] / call_ms
            out["cases"][f"T{T}/n{n_obs}/noise{int(noise)}"] = r
            print(f"T{T}/n{n_obs}/noise{int(noise)}", r, flush=True)
    del gt, bufs, gt_h
out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "profiles", "r10"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "obs_synth.json"), "w") as f:
    json.dump(out, f, indent=1)
