"""vv_err_accum and vv_r_fill timing (development tool): the median of VV_ERR_REPS (default 25, at least
20) event-timed calls after warm-up, buffers allocated once.

err_accum at 69 x 128 x 256, B = 4, pred the network's (B, 138, H, W) output and tgt the slice [:, 1] of a
(B, 2, 69, H, W) window, against the torch expression of calculate_q (model/model.py:485-486) on the device,
`acc += ((pred[:, :69] - tgt)**2).double()` -- as written, with one accumulator per sample, and summed over the
batch into the (69, H, W) accumulator the kernel updates -- and against the same with the channel totals
(`chan += (pred[:, :69] - tgt).double().sum((0, 2, 3))`); cell only, and cell with chan.
r_fill at (6, 204, 721, 1440) (the level operator, 69 -> 204 channels) and (6, 69, 721, 1440) against the path it
replaces, timed by a host clock around a synchronised run: the numpy broadcast of the (T, 69) table, the upload of the
dense field and vv_obs_augment. No threshold is asserted. Writes $VV_OUT/err_stats.json (default profiles/r11/)."""
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
from vaevar.engine import Context, err_accum, err_finalize, obs_augment, r_fill
from vaevar.problem import ObsInterpolater, obs_variance, static_r_table

REPS = max(20, int(os.environ.get("VV_ERR_REPS", 25)))
HOST_REPS = int(os.environ.get("VV_ERR_HOST_REPS", 3))
ctx = Context.get(0)


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
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


out = {"device": torch.cuda.get_device_name(0), "lib_version": lib.vv_version(), "repeats": REPS,
       "host_repeats": HOST_REPS, "err_accum": {}, "r_fill": {}}

# --- err_accum ------------------------------------------------------------------------------------------------
B, C, H, W = 4, 69, 128, 256
g = torch.Generator().manual_seed(3)
pred = torch.randn((B, 138, H, W), generator=g).cuda()
win = torch.randn((B, 2, C, H, W), generator=g).cuda()
tgt = win[:, 1]
cell = torch.zeros(C, H, W, device="cuda", dtype=torch.float64)
chan = torch.zeros(C, device="cuda", dtype=torch.float64)
acc = torch.zeros_like(cell)
acc_c = torch.zeros_like(chan)
n = B * C * H * W


acc4 = torch.zeros(B, C, H, W, device="cuda", dtype=torch.float64)


def torch_literal():  # one accumulator per sample: the expression as written, without the sum over the batch
    global acc4
    acc4 += ((pred[:, :C] - tgt) ** 2).double()


def torch_cell():
    acc.add_(((pred[:, :C] - tgt) ** 2).double().sum(0))


def torch_both():
    d = pred[:, :C] - tgt
    acc.add_((d ** 2).double().sum(0))
    acc_c.add_(d.double().sum((0, 2, 3)))


e = out["err_accum"]
e["shape"] = [B, C, H, W]
e["bytes"] = 2 * 4 * n + 16 * C * H * W  # pred and tgt read once, cell read and written
e["kernel_cell"] = events(lambda: err_accum(ctx, pred, tgt, cell, None, C=C))
e["kernel_cell_chan"] = events(lambda: err_accum(ctx, pred, tgt, cell, chan, C=C))
e["kernel_chan"] = events(lambda: err_accum(ctx, pred, tgt, None, chan, C=C))
e["torch_literal_per_sample_acc"] = events(torch_literal)
e["torch_cell"] = events(torch_cell)
e["torch_cell_chan"] = events(torch_both)
e["finalize_field_and_table"] = events(lambda: err_finalize(ctx, cell, 100, q_field=acc))
e["kernel_cell_GBps"] = e["bytes"] / e["kernel_cell"]["ms_median"] * 1e-6
e["torch_literal_over_kernel_cell"] = e["torch_literal_per_sample_acc"]["ms_median"] / e["kernel_cell"]["ms_median"]
e["torch_over_kernel_cell"] = e["torch_cell"]["ms_median"] / e["kernel_cell"]["ms_median"]
e["torch_over_kernel_cell_chan"] = e["torch_cell_chan"]["ms_median"] / e["kernel_cell_chan"]["ms_median"]
print("err_accum", e, flush=True)
del pred, win, cell, acc, acc4

# --- r_fill ---------------------------------------------------------------------------------------------------
T, Hs, Ws = 6, 721, 1440
oi = ObsInterpolater(13, 40)
ov = obs_variance(69, 0.005, 2, np.asarray(Cf.MODEL_STD, np.float32))
tab = static_r_table(ov, np.random.default_rng(4).random((T - 1, 69)) * ov, T)
tab_d = torch.from_numpy(tab).cuda()
interp_d = torch.from_numpy(oi.interp).cuda()


def host_path(op):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dense = np.broadcast_to(tab[:, :, None, None], (T, 69, Hs, Ws)).astype(np.float32).copy()
    t1 = time.perf_counter()
    d = torch.from_numpy(dense).cuda()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if op:
        d = obs_augment(ctx, interp_d, d)
        torch.cuda.synchronize()
    t3 = time.perf_counter()
    del d
    return {"broadcast_ms": (t1 - t0) * 1e3, "upload_ms": (t2 - t1) * 1e3, "augment_ms": (t3 - t2) * 1e3,
            "total_ms": (t3 - t0) * 1e3}


for name, op, ca in (("operator_6x204x721x1440", True, 204), ("identity_6x69x721x1440", False, 69)):
    R = torch.empty(T, ca, Hs, Ws, device="cuda")
    r = {"shape": [T, ca, Hs, Ws], "bytes": 4 * T * ca * Hs * Ws}
    r["kernel"] = events(lambda: r_fill(ctx, tab_d, Hs, Ws, interp=interp_d if op else None, out=R))
    r["kernel_GBps"] = r["bytes"] / r["kernel"]["ms_median"] * 1e-6
    r["kernel_fraction_of_8TBps"] = r["kernel_GBps"] / 8000.0
    host = [host_path(op) for _ in range(HOST_REPS)]
    r["host_reps"] = host
    r["host_total_ms_median"] = float(np.median([h["total_ms"] for h in host]))
    r["host_dense_bytes_uploaded"] = 4 * T * 69 * Hs * Ws
    r["host_over_kernel"] = r["host_total_ms_median"] / r["kernel"]["ms_median"]
    out["r_fill"][name] = r
    print(name, r, flush=True)
    del R

out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "profiles", "r11"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "err_stats.json"), "w") as f:
    json.dump(out, f, indent=1)
