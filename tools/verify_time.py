"""vv_verify timing (development tool): the call time of the forecast verification at 69 x 721 x 1440 by
device events, with and without a climatology, next to vv_metrics (WRMSE / Bias only) on the same fields, in one
process. After a warm-up the three are timed in alternation: REPS windows of N calls each, the median window and the
spread (min, max) per variant, and the achieved GB/s over the algorithmic bytes 4*C*H*W*(2 or 3). With --cycle also
the wall time of one free_run cycle of the 0.25-degree forecast model (synthetic weights, truth held in host memory)
with forecast_steps = 4 against the same cycle with forecast_eval off. Writes $VV_OUT/verify_time.json (default
bench_out/)."""
import argparse
import datetime as dt
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-var_amd"))
import numpy as np
import torch

from vaevar import config as Cf
from vaevar._lib import lib
from vaevar.engine import Context
from vaevar.metrics import Metrics

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--cycle", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "verify_time needs the GPU"

C, H, W = 69, 721, 1440
g = torch.Generator(device="cuda").manual_seed(1)
mean = torch.tensor(Cf.MODEL_MEAN, dtype=torch.float32, device="cuda").reshape(-1, 1, 1)
std = torch.tensor(Cf.MODEL_STD, dtype=torch.float32, device="cuda").reshape(-1, 1, 1)
gt = mean + std * torch.randn(C, H, W, device="cuda", generator=g)
pred = gt + 0.3 * std * torch.randn(C, H, W, device="cuda", generator=g)
clim = mean + 0.5 * std * torch.randn(C, H, W, device="cuda", generator=g)
m = Metrics(Context.get(0))
variants = {"verify": lambda: m.verify(pred, gt), "verify_clim": lambda: m.verify(pred, gt, clim),
            "metrics": lambda: m.wrmse_bias(pred, gt)}
nbytes = {"verify": 8.0 * C * H * W, "verify_clim": 12.0 * C * H * W, "metrics": 8.0 * C * H * W}
for f in variants.values():
    for _ in range(5):
        f()
torch.cuda.synchronize()
reps = {k: [] for k in variants}
for r in range(args.reps):
    for k, f in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            f()
        b.record()
        torch.cuda.synchronize()
        reps[k].append(a.elapsed_time(b) / args.calls * 1e3)
out = {"shape": [C, H, W], "device": torch.cuda.get_device_name(0), "lib_version": lib.vv_version(),
       "windows": args.reps, "calls_per_window": args.calls,
       "note": "vv_metrics ends every call with a stream synchronise, so its window holds no queued calls", "cases": {}}
for k, v in reps.items():
    med = float(np.median(v))
    out["cases"][k] = {"us_per_call_median": med, "us_per_call_min": float(min(v)), "us_per_call_max": float(max(v)),
                       "algorithmic_bytes": nbytes[k], "GBps_at_median": nbytes[k] / med * 1e-3}
    print(k, out["cases"][k], flush=True)
w0 = m.verify(pred, gt)["WRMSE"]
w1 = m.wrmse_bias(pred, gt)[0]
out["wrmse_rel_diff_verify_vs_metrics"] = float(((w0 - w1).abs() / w1.abs()).max())

if args.cycle:
    from vaevar.cycle import CyclicDA, SyntheticObs
    from vaevar.engine import LGUnet

    t0 = time.time()
    fc = LGUnet(Cf.FCST, 1, 1).load_synthetic()
    print(f"forecast model built in {time.time() - t0:.1f} s", flush=True)
    truth_np, T0, H6 = gt.cpu().numpy(), dt.datetime(2018, 1, 1), dt.timedelta(hours=6)
    obs = SyntheticObs(lambda t: truth_np, None, None)
    cyc = {}
    with tempfile.TemporaryDirectory() as d:
        for name, kw in (("off", {}), ("on", {"forecast_eval": True, "forecast_steps": 4}), ("off2", {}),
                         ("on2", {"forecast_eval": True, "forecast_steps": 4})):
            c = CyclicDA(fc, obs, T0, T0 + 2 * H6, 0, name, da_mode="free_run", out_dir=d, xb0=pred.cpu().numpy(), **kw)
            marks = []
            torch.cuda.synchronize()
            t0 = time.time()

            def log(t, res, marks=marks):
                torch.cuda.synchronize()
                marks.append(time.time())

            c.run_assimilation(log=log)
            # the second cycle alone (the first one warms the model up): from the first log call to the second
            cyc[name] = marks[1] - marks[0]
    # what the extra time is made of: one forecast step, one truth upload (host array -> device), one verify call
    from vaevar.engine import integrate

    def wall(f, n=5):
        f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.time()
            f()
            torch.cuda.synchronize()
            ts.append(time.time() - t0)
        return float(np.median(ts))

    parts = {"forecast_step_s": wall(lambda: integrate(fc, pred, mean.reshape(-1), std.reshape(-1), 1)),
             "truth_upload_s": wall(lambda: torch.from_numpy(truth_np).to("cuda")),
             "verify_call_s": wall(lambda: m.verify(pred, gt))}
    out["cycle_free_run_025deg"] = {"wall_s_second_cycle": cyc, "forecast_steps_on": 4,
                                    "extra_s": [cyc["on"] - cyc["off"], cyc["on2"] - cyc["off2"]], "parts": parts,
                                    "expected_extra_s": 3 * parts["forecast_step_s"] + 4 * parts["truth_upload_s"] +
                                    4 * parts["verify_call_s"]}
    print(out["cycle_free_run_025deg"], flush=True)

out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "bench_out"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "verify_time.json"), "w") as f:
    json.dump(out, f, indent=1)
