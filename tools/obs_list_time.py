"""Observation-list timing (development tool): the vae4dvar closure with gradient at 721 x 1440, T = 1,
with the full decoder and the real-observation operator (make_real_problem, 204 observation channels), evaluated from
the dense fields and from the observation list, for obs_frac in {0.001, 0.01, 0.05, 0.25}. In one process, per
density: after a warm-up of each path (the closure graph is re-captured after every switch) the two paths are timed in
alternation by device events, REPS windows of N evaluations each; the median window and the spread (min, max) per
path. Also the wall time of vv_set_obs_list(enable = 1) itself (synchronised, every switch of the run), the list's
size, and the misfit-class kernel time of one eager evaluation of each path (the live profiler). Writes
$VV_OUT/obs_list.json (default profiles/r09/)."""
import argparse
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
from vaevar.engine import DAProblem, LGUnet
from vaevar.problem import make_real_problem
from vaevar.synth import smooth_field

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--fracs", type=float, nargs="+", default=[0.001, 0.01, 0.05, 0.25])
args = ap.parse_args()
assert torch.cuda.is_available(), "obs_list_time needs the GPU"

Hs, Ws = 721, 1440
dec = LGUnet(Cf.DECODER, 1, 1).load_synthetic()
z = torch.from_numpy(0.3 * smooth_field(406, (1, 32, 128, 256))).cuda()
g = torch.empty_like(z)
out = {"shape": [1, 204, Hs, Ws], "device": torch.cuda.get_device_name(0), "lib_version": lib.vv_version(),
       "windows": args.reps, "calls_per_window": args.calls, "closure": "vae4dvar, full decoder, J + gradient, graphs on",
       "cases": {}}


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


for frac in args.fracs:
    t0 = time.time()
    p = make_real_problem(Hs=Hs, Ws=Ws, T=1, seed=20250623, obs_frac=frac)
    prob = DAProblem(dec, p)
    del p
    print(f"obs_frac {frac}: problem built and bound in {time.time() - t0:.1f} s", flush=True)
    builds, windows, misfit = [], {"dense": [], "list": []}, {}

    def switch(on):
        torch.cuda.synchronize()
        t = time.time()
        prob.obs_list(on)
        if on:
            builds.append((time.time() - t) * 1e3)
        for _ in range(3):  # eager, capture, replay
            prob.closure_lazy(z, g)
        torch.cuda.synchronize()

    for r in range(args.reps):
        for name, on in (("dense", False), ("list", True)):
            switch(on)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                prob.closure_lazy(z, g)
            b.record()
            torch.cuda.synchronize()
            windows[name].append(a.elapsed_time(b) / args.calls)
    info = prob.obs_list_info
    for name, on in (("dense", False), ("list", True)):
        switch(on)
        prob.ctx.profile_start()
        prob.closure(z, g)
        misfit[name] = prob.ctx.profile_stop()["misfit"]
    case = {"units": info["units"], "records": info["records"], "list_bytes": info["bytes"],
            "dense_bytes_yo_H_R": 3 * 4 * 204 * Hs * Ws, "set_obs_list_ms": stats(builds),
            "closure_ms": {k: stats(v) for k, v in windows.items()}, "misfit_class_one_eval": misfit}
    case["list_over_dense_median"] = case["closure_ms"]["list"]["median"] / case["closure_ms"]["dense"]["median"]
    out["cases"][str(frac)] = case
    print(frac, json.dumps(case), flush=True)
    prob.obs_list(False)
    del prob
    torch.cuda.empty_cache()

out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "profiles", "r09"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "obs_list.json"), "w") as f:
    json.dump(out, f, indent=1)
