"""The host side of vv_obs_grid (include/vaevar.h): the station-report table and the level tables of
data_reader.get_real_obs / get_obs_mask (da_4dvar.py:301-440, :190-274). No GPU is needed here.

A parsed report file of the reference's layout is a dict message -> {"position": [lon, lat, plev, dt],
"value": [p, z, q, u, v, t, _, msl], ...} (an empty list when the hour has no file, :175). The table has one fp64 row
per message, in the dict's order; fp64 because the reference rounds its indices and forms its values in fp64."""
from __future__ import annotations

import numpy as np

COLUMNS = ("src", "lon", "lat", "plev", "dt", "p", "z", "q", "u", "v", "t", "msl")
GRID_REAL, GRID_MASK = 0, 1  # VV_GRID_*
# get_obs_mask's `height` (:195): the bounds between the 13 pressure levels of the state
MASK_BOUNDS = np.array([75, 125, 175, 225, 275, 350, 450, 550, 650, 775, 887.5, 962.5], np.float64)


def pack_reports(d, src: int = 0) -> np.ndarray:
    """One parsed report file as (N, 12) float64 rows in COLUMNS order, None as NaN, the dict's order kept. src 0: the
    file at tstamp, 1: the file at tstamp + cycle_time (:408-436). The table of a window is
    np.concatenate([pack_reports(d0, 0), pack_reports(d1, 1)])."""
    out = np.empty((len(d), 12), np.float64)
    for k, message in enumerate(d):
        elem = d[message]
        pos, val = elem["position"], elem["value"]
        row = [src, pos[0], pos[1], pos[2], pos[3], val[0], val[1], val[2], val[3], val[4], val[5], val[-1]]
        out[k] = [np.nan if x is None else x for x in row]
    return out


def level_tables(levels):
    """(bounds, log_lev, zcoef, tcoef) of get_real_obs for an ObsInterpolater (its height_level_new) or a sequence of
    levels: bounds[i] = sqrt(lev[i] * lev[i+1]) (:311-313), log_lev = log(lev), and get_geopotential_coeff /
    get_temperature_coeff (:315-327) per index. float64."""
    lev = np.asarray(getattr(levels, "height_level_new", levels), np.float64)
    bounds = np.zeros(len(lev) - 1)
    for i in range(len(bounds)):
        bounds[i] = np.sqrt(lev[i] * lev[i + 1])
    zcoef = np.array([61245 if i == 0 else 62000 if i <= 16 else 927.87 * i + 47138.48 for i in range(len(lev))],
                     np.float64)
    tcoef = np.array([0 if i <= 21 else -25 for i in range(len(lev))], np.float64)
    return bounds, np.log(lev), zcoef, tcoef
