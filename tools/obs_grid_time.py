"""vv_obs_grid timing (development tool): cycle.StationObs.get_obs_info (upload of the report table,
vv_obs_grid, vv_obs_qc) at (1, 204, 721, 1440) and (6, 204, 721, 1440), obs_type 'real', for 10^5 and 10^6 seeded
reports spread over the globe, by a host clock around the call and a device synchronise. The report counts of real
files are not known here; the two sizes bracket a guess. The yardstick, in the same run and alternating with it, is
cycle.RealObs.get_obs_info on the same shapes with a reader that returns READY host arrays (the grids the new path
produced, downloaded once): the old path with its host gridding left out entirely, so a lower bound on what it cost.
Both paths fetch the truth window the same way. Also vv_obs_grid alone by device events with the table already on the
device (median of five repeats of 20 queued calls), and whether the two paths' outputs are bitwise equal.
Writes $VV_OUT/obs_grid.json (default profiles/r07/)."""
import datetime as dt
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
from vaevar.cycle import RealObs, StationObs
from vaevar.engine import Context, obs_grid
from vaevar.problem import ObsInterpolater
from vaevar.reports import GRID_REAL

Hs, Ws, C, NOUT = 721, 1440, 69, 40
REPS = int(os.environ.get("VV_GRID_REPS", 3))
SIZES = [int(x) for x in os.environ.get("VV_GRID_SIZES", "100000,1000000").split(",")]
WINS = [int(x) for x in os.environ.get("VV_GRID_WINS", "1,6").split(",")]
T0 = dt.datetime(2018, 1, 1, 0)
ctx = Context.get(0)
oi = ObsInterpolater(13, NOUT)
rng = np.random.default_rng(7)
mean = np.asarray(Cf.MODEL_MEAN, np.float32)[:, None, None]
std = np.asarray(Cf.MODEL_STD, np.float32)[:, None, None]
gt0 = (mean + std * rng.standard_normal((C, Hs, Ws), dtype=np.float32)).astype(np.float32)
truth = lambda t: gt0  # noqa: E731


def table(n, da_win):
    t = np.empty((n, 12))
    t[:, 0] = rng.integers(0, 2, n) if da_win == 6 else 0
    t[:, 1], t[:, 2] = rng.uniform(0, 360, n), rng.uniform(-90, 90, n)
    t[:, 3] = t[:, 5] = np.exp(rng.uniform(np.log(40), np.log(1080), n))
    t[:, 4] = np.where(t[:, 0] == 0, rng.uniform(-0.5, 3.5, n), rng.uniform(-3.5, -0.5, n)) if da_win == 6 else \
        rng.uniform(-0.5, 0.5, n)
    t[:, 6], t[:, 7] = rng.uniform(100, 30000, n), rng.uniform(1, 20000, n)
    t[:, 8:10] = rng.normal(0, 15, (n, 2))
    t[:, 10], t[:, 11] = rng.uniform(-80, 40, n), rng.uniform(950, 1050, n)
    t[:, 6:][rng.random((n, 6)) < 0.1] = np.nan
    return t


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


out = {"device": torch.cuda.get_device_name(0), "lib_version": lib.vv_version(), "repeats": REPS,
       "note": "report counts of real files unknown; RealObs is timed with ready host arrays (no host gridding)",
       "cases": {}}
for da_win in WINS:
    shape = (da_win, 4 + 5 * NOUT, Hs, Ws)
    R = np.full((da_win, C, Hs, Ws), 1.0, np.float32)
    for n in SIZES:
        tab = table(n, da_win)
        kw = dict(filter_coeff=30.0, da_win=da_win)
        sta = StationObs(ctx, truth, lambda t: tab, R, oi.interp, oi, "real", **kw)
        yo, H, _, _ = sta.get_obs_info(T0)  # warm-up; its ungated grids feed the yardstick's reader
        yo_g, H_g, stats = obs_grid(ctx, tab, GRID_REAL, da_win, oi, Hs, Ws)
        ready = (yo_g.cpu().numpy(), H_g.cpu().numpy())
        del yo_g, H_g
        real = RealObs(ctx, truth, lambda t: ready, R, oi.interp, "real", **kw)
        yo_r, H_r, _, _ = real.get_obs_info(T0)  # warm-up
        same = bool(torch.equal(yo, yo_r) and torch.equal(H, H_r) and np.array_equal(sta.counts, real.counts))
        del yo, H, yo_r, H_r
        t_new, t_old = [], []
        for _ in range(REPS):  # alternating
            t_new.append(wall(lambda: sta.get_obs_info(T0))[0])
            t_old.append(wall(lambda: real.get_obs_info(T0))[0])
        t_truth = [wall(lambda: torch.from_numpy(np.stack([truth(T0)] * da_win, 0).astype(np.float32)).cuda())[0]
                   for _ in range(REPS)]
        tab_d = torch.from_numpy(tab).cuda()
        bufs = (torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda"))
        ev = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                obs_grid(ctx, tab_d, GRID_REAL, da_win, oi, Hs, Ws, out=bufs)
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b) / 20)
        del bufs
        r = {"shape": list(shape), "reports": n, "grid_stats": stats.cpu().tolist(),
             "station_obs_ms_reps": t_new, "station_obs_ms_median": float(np.median(t_new)),
             "real_obs_ready_arrays_ms_reps": t_old, "real_obs_ready_arrays_ms_median": float(np.median(t_old)),
             "truth_window_fetch_ms_median": float(np.median(t_truth)),
             "real_over_station": float(np.median(t_old) / np.median(t_new)),
             "obs_grid_device_ms_reps": ev, "obs_grid_device_ms_median": float(np.median(ev)),
             "table_bytes": int(tab.nbytes), "dense_bytes_per_cycle_old_path": int(2 * 4 * np.prod(shape)),
             "outputs_bitwise_equal": same}
        out["cases"][f"w{da_win}/n{n}"] = r
        print(f"w{da_win}/n{n}", r, flush=True)
        del sta, real, ready
out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "profiles", "r07"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "obs_grid.json"), "w") as f:
    json.dump(out, f, indent=1)
