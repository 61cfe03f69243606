"""Make tests/golden/g17_obs_grid.npz: station-report tables and what the REFERENCE's data_reader.get_real_obs and
get_obs_mask (da_4dvar.py:301-440, :190-274) make of them, stored sparsely. CPU only; needs the reference tree that
oracle.ref_harness imports (it is not part of this repository) and about 5 GB of memory.

    python tools/make_obs_grid_fixture.py

The two methods are called unbound on a stub `self` whose read_json returns hand-made dicts; nothing else of the
reference runs. Cases: real (da_win 1, n_out 40), real (da_win 6, n_out 7: the reference hard-codes 721 x 1440 and
dense tensors, three of 0.97 GB at 39 channels), mask (da_win 6). Per case the (N, 12) table (vaevar.reports), the flat
indices where H == 1 and yo there; both grids are asserted to be 0 elsewhere. The reports contain none the reference
raises on."""
import datetime as dt
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vae-var_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

T0 = dt.datetime(2018, 1, 1, 0)
CYCLE = dt.timedelta(hours=6)
HEIGHT_MASK = [75, 125, 175, 225, 275, 350, 450, 550, 650, 775, 887.5, 962.5]


def make_files(levels, seed, mask=False):
    """(d0, d1): the parsed report files at tstamp and tstamp + cycle_time."""
    rng = np.random.default_rng(seed)
    lev = [float(x) for x in levels]
    bounds = [float(np.sqrt(lev[i] * lev[i + 1])) for i in range(len(lev) - 1)]
    files = ({}, {})

    def msg(f, lon, lat, plev, dtm, p, z=5500.0, q=3000.0, u=4.5, v=-2.25, t=-12.5, msl=None, extra=7.0):
        files[f][f"m{f}_{len(files[f]):04d}"] = {"position": [lon, lat, plev, dtm],
                                                 "value": [p, z, q, u, v, t, extra, msl], "type": "ADPUPA"}

    # a None in each position slot
    msg(0, None, 10.0, 500.0, 0.0, 500.0)
    msg(0, 10.0, None, 500.0, 0.0, 500.0)
    msg(0, 10.0, 10.0, None, 0.0, 500.0)
    msg(0, 10.0, 10.0, 500.0, None, 500.0)
    msg(1, None, 10.0, 500.0, -2.0, 500.0)
    # None and 0.0 values, t = 0.0 among them
    msg(0, 20.0, 20.0, 500.0, 0.0, 500.0, z=None, q=0.0, u=3.0, v=None, t=0.0, msl=1013.25)
    msg(0, 21.0, 20.0, 500.0, 0.0, 500.0, z=5600.0, q=None, u=0.0, v=1.5, t=None, msl=0.0)
    msg(0, 22.0, 20.0, 1000.0, 0.0, 1040.0, z=0.0, q=9000.0, u=-0.0, v=2.0, t=0.0, msl=None)
    msg(0, 23.0, 20.0, 500.0, 0.0, 500.0, z=None, q=None, u=None, v=None, t=None, msl=None)
    # longitudes that round to Ws, the ties 0.125 (-> 0) and 0.375 (-> 2), the poles, a negative longitude
    for lon in (359.9, 359.875, 359.99, 0.125, 0.375, 0.0, 0.124, 0.126):
        msg(0, lon, 45.0, 300.0, 0.0, 300.0, msl=1000.0 + lon)
    for lat in (90.0, -90.0, 89.9, -89.9, 89.875, -89.8):
        msg(0, 100.0, lat, 700.0, 0.0, 700.0, msl=990.0)
    msg(0, -10.0, 5.0, 850.0, 0.0, 850.0, msl=1001.0)
    msg(0, -0.1, 5.0, 850.0, 0.0, 850.0)
    msg(0, -359.9, -5.0, 850.0, 0.0, 850.0)
    # dt on every bin edge and beside it, both files
    for k, d in enumerate((-0.5, 0.5, 1.5, 2.5, -0.500001, 0.499999, 1.499999, 2.499999, 3.7, 17.0, -3.0, -0.75)):
        msg(0, 40.0 + k, -30.0, 400.0, d, 400.0, msl=1002.0 + k)
    for k, d in enumerate((-2.5, -1.5, -0.5, -2.500001, -1.500001, -0.500001, -3.3, -40.0, 0.0, -0.25, 2.0)):
        msg(1, 60.0 + k, -30.0, 400.0, d, 400.0, msl=1003.0 + k)
    # p exactly on a bound, beside it, beyond both ends; plev on get_obs_mask's bounds
    for k, b in enumerate(bounds[:6]):
        msg(0, 80.0 + k, 12.0, HEIGHT_MASK[2 * k % 12], 0.2, b)
        msg(0, 80.0 + k, 13.0, HEIGHT_MASK[(2 * k + 1) % 12] - 1e-9, 0.2, float(np.nextafter(b, 0.0)))
        msg(0, 80.0 + k, 14.0, HEIGHT_MASK[(2 * k + 1) % 12] + 1e-9, 0.2, float(np.nextafter(b, 1e9)))
    for k, pp in enumerate((10.0, 49.0, 50.0, lev[0], lev[-1], 1000.0, 1013.0, 1100.0, 2000.0)):
        msg(0, 90.0 + k, 15.0, pp, 0.2, pp, msl=1010.0)
    # surface rows (h = n_lev - 1) with and without the three surface values
    msg(0, 110.0, 50.0, 1000.0, 0.0, 1020.0, u=7.0, v=-3.0, t=15.5, msl=1020.0)
    msg(0, 111.0, 50.0, 1000.0, 0.0, 1020.0, u=None, v=-3.0, t=0.0, msl=1020.0)
    msg(0, 112.0, 50.0, 1000.0, 0.0, float(lev[-1]), u=7.0, v=0.0, t=-5.0)
    # cells hit 2, 3 and 41 times, values of mixed magnitude: the order of the fp32 additions matters
    big = [1e8, 1.0, -1e8, 1.0, 3.3e7, -1.25e-3, 6e4, -3.3e7]
    for hits, lon in ((2, 130.0), (3, 131.0), (41, 132.0)):
        for k in range(hits):
            s = big[k % 8] * (1 + k // 8)
            msg(0, lon + 0.05 * (k % 3 - 1), 33.0 + 0.03 * (k % 2), 1000.0, 0.3, 1015.0 + 0.5 * (k % 5), z=s, q=s * 3,
                u=s, v=-s * 0.7, t=s * 1e-3 if k % 7 else 0.0, msl=s * 1e-2 if k % 4 else None)
    for k in range(17):  # an upper-air cell with a spread of pressures in one level
        msg(0, 140.0, -12.0, 500.0, 1.1, 500.0 + 1.7 * k, z=5400.0 + 9.1 * k, t=-20.0 + 0.37 * k)
    # one t = 3 cell fed from both files, in alternation of magnitude
    for k in range(5):
        msg(0, 150.0, 0.0, 700.0, 2.6 + k, 700.0, z=3000.0 + k, u=1e7 * (k % 2) + k, msl=1000.0 + k)
        msg(1, 150.0, 0.0, 700.0, -2.6 - k, 700.0, z=-2999.0 + k, u=-1e7 * (k % 2) + 0.5, msl=900.0 - k)
    if mask:  # get_obs_mask does not read value[0]
        msg(0, 160.0, 10.0, 925.0, 0.0, None)
        msg(1, 160.0, 10.0, 962.5, -1.0, None, msl=1000.0)
    # the bulk: seeded reports over the globe
    for k in range(120):
        f = int(rng.integers(0, 2))
        pp = float(np.exp(rng.uniform(np.log(40), np.log(1080))))
        vals = [float(x) for x in (rng.uniform(100, 30000), rng.uniform(1, 20000), rng.normal(0, 15), rng.normal(0, 15),
                                   rng.uniform(-80, 40), rng.uniform(950, 1050))]
        for j in range(6):
            r = rng.random()
            vals[j] = None if r < 0.12 else 0.0 if r < 0.15 else vals[j]
        msg(f, float(rng.uniform(-5, 359.8)), float(rng.uniform(-90, 90)), pp * float(rng.uniform(0.98, 1.02)),
            float(rng.uniform(-1, 4) if f == 0 else rng.uniform(-4, 0)), pp, z=vals[0], q=vals[1], u=vals[2], v=vals[3],
            t=vals[4], msl=vals[5])
    return files


def sparse(H, obs=None):
    import torch

    Hf = H.flatten()
    idx = torch.nonzero(Hf).flatten()
    assert bool((Hf[idx] == 1).all())
    if obs is None:
        return idx.numpy().astype(np.int64), None
    of = obs.flatten()
    on = Hf != 0
    assert float(of[~on].abs().max()) == 0.0, "yo must be 0 wherever H is"
    return idx.numpy().astype(np.int64), of[idx].numpy().astype(np.float32)


def main():
    from oracle import ref_harness

    ref_harness.import_reference()
    da = importlib.import_module("da_4dvar")
    from vaevar.problem import ObsInterpolater
    from vaevar.reports import pack_reports

    out = {}
    for name, da_win, n_out, mask in (("real_w1_n40", 1, 40, False), ("real_w6_n7", 6, 7, False),
                                      ("mask_w6", 6, 13, True)):
        levels = ObsInterpolater(13, n_out).height_level_new
        d0, d1 = make_files(levels, 1700 + n_out, mask=mask)
        files = {T0: d0, T0 + CYCLE: d1}
        stub = types.SimpleNamespace(obs_from_numpy=False, da_win=da_win, cycle_time=CYCLE, obs_type="prepbufr",
                                     read_json=lambda t, files=files: files[t],
                                     obs_interp=types.SimpleNamespace(dim_out=n_out, height_level_new=levels))
        if mask:
            idx, yo = sparse(da.data_reader.get_obs_mask(stub, T0))
        else:
            obs, H = da.data_reader.get_real_obs(stub, T0)
            idx, yo = sparse(H, obs)
            out[name + "_yo"] = yo
            del obs, H
        out[name + "_table"] = np.concatenate([pack_reports(d0, 0), pack_reports(d1, 1)])
        out[name + "_idx"] = idx
        out[name + "_meta"] = np.array([da_win, n_out], np.int64)
        print(name, "reports", len(out[name + "_table"]), "cells", len(idx))
    path = os.path.join(ROOT, "tests", "golden", "g17_obs_grid.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
