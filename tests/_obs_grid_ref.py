"""Per-row numpy restatement of vv_obs_grid (include/vaevar.h): data_reader.get_real_obs (da_4dvar.py:301-440) and
get_obs_mask for obs_type prepbufr* (:190-274) on the (N, 12) report table, for any Hs, Ws and level set. Independent
of vaevar.reports and of the kernels; pinned bitwise to the reference by tests/golden/g17_obs_grid.npz
(tools/make_obs_grid_fixture.py, tests/test_obs_grid_host.py).

The grids are returned sparsely: the sorted flat indices of the cells with H = 1 in a (da_win, 4 + 5*n_lev, Hs, Ws)
grid and yo there (both grids are 0 elsewhere), and stats = [rows used, skipped, dropped, cells]. Rows on which the
reference would raise (an index out of range, a NaN p in the real mode) are dropped and counted."""
import numpy as np

REAL, MASK = 0, 1
HEIGHT_MASK = [75, 125, 175, 225, 275, 350, 450, 550, 650, 775, 887.5, 962.5]  # get_obs_mask's level bounds


def levels_of(n_out):
    return np.round(np.exp(np.linspace(3.91202301, 6.90775528, n_out)))


def _index(x, size, at_size):
    """int(np.round(x)) as an index of an axis; None where Python would raise."""
    try:
        i = int(np.round(x))
    except (OverflowError, ValueError):
        return None
    if i == size:
        i = at_size
    if i < -size or i >= size:
        return None
    return i + size if i < 0 else i


def _time_level(da_win, src, dt):
    if da_win == 1 or src == 0:
        if -0.5 <= dt < 0.5:
            return 0
        if da_win == 1:
            return None
        if 0.5 <= dt < 1.5:
            return 1
        if 1.5 <= dt < 2.5:
            return 2
        return 3 if dt >= 2.5 else None
    if dt < -2.5:
        return 3
    if -2.5 <= dt < -1.5:
        return 4
    if -1.5 <= dt < -0.5:
        return 5
    return None


def _zcoef(i):
    return 61245 if i == 0 else 62000 if i <= 16 else 927.87 * i + 47138.48


def _tcoef(i):
    return 0 if i <= 21 else -25


def _present(v):
    return not np.isnan(v) and v != 0.0  # None (NaN in the table) or a falsy number


def obs_grid_ref(table, mode, da_win, levels, Hs, Ws):
    """levels: the pressure levels of the observation space (real mode; ignored in mask mode, which has the 13 state
    levels). Returns (idx int64 sorted, yo float32 at idx or None in mask mode, stats int64[4])."""
    if da_win not in (1, 6):
        raise NotImplementedError("da win must equal six or one")
    if mode == REAL:
        lev = np.asarray(levels, np.float64)
        bounds = np.array([np.sqrt(lev[i] * lev[i + 1]) for i in range(len(lev) - 1)])
    else:
        lev, bounds = None, np.array(HEIGHT_MASK, np.float64)
    n_lev = len(bounds) + 1
    Ca, HW = 4 + 5 * n_lev, Hs * Ws
    sums, cnts = {}, {}
    used = skipped = dropped = 0

    def assign(t, layer, pix, value):
        c = (t * Ca + layer) * HW + pix
        cnts[c] = cnts.get(c, 0) + 1
        if value is not None:  # obs[...] += value on an fp32 tensor: the value rounded to fp32, then an fp32 add
            sums[c] = np.float32(sums.get(c, np.float32(0.0)) + np.float32(value))

    with np.errstate(all="ignore"):
        for row in np.asarray(table, np.float64).reshape(-1, 12):
            src, lon, lat, plev, dt, p = (float(x) for x in row[:6])
            z, q, u, v, tt, msl = (float(x) for x in row[6:])
            if da_win == 1 and src != 0:  # the second file is not read
                skipped += 1
                continue
            if np.isnan(lon) or np.isnan(lat) or np.isnan(plev) or np.isnan(dt):
                skipped += 1
                continue
            lon_i = _index(lon / 360 * Ws, Ws, 0)
            lat_i = _index((90 - lat) / 180 * Hs, Hs, Hs - 1)
            pl = p if mode == REAL else plev
            if lon_i is None or lat_i is None or np.isnan(pl):
                dropped += 1
                continue
            h = int(np.sum((bounds - pl) <= 0))
            t = _time_level(da_win, src, dt)
            if t is None:
                skipped += 1
                continue
            used += 1
            pix = lat_i * Ws + lon_i
            if mode == MASK:
                for i, x in enumerate((z, q, u, v, tt)):
                    if _present(x):
                        assign(t, 4 + h + i * n_lev, pix, None)
                if _present(msl):
                    assign(t, 3, pix, None)
                continue
            for i, x in enumerate((z, q, u, v, tt)):
                if not _present(x):
                    continue
                value = x
                if i == 0:
                    value *= 9.8
                elif i == 1:
                    value *= 1e-6
                elif i == 4:
                    value += 273.15
                if i == 0:
                    value += _zcoef(h) * (np.log(p) - np.log(lev[h]))
                elif i == 4:
                    value += _tcoef(h) * (np.log(p) - np.log(lev[h]))
                assign(t, 4 + h + i * n_lev, pix, value)
            if _present(msl):
                assign(t, 3, pix, msl * 100)
            if h == n_lev - 1:
                for i, x in enumerate((u, v, tt)):
                    if _present(x):
                        assign(t, i, pix, x + 273.15 if i == 2 else x)
    if mode == MASK:
        cells = set(cnts)
        for c in cnts:
            t, rem = divmod(c, Ca * HW)
            layer, pix = divmod(rem, HW)
            for k in range(3):
                if layer == 4 + (k + 2) * n_lev + n_lev - 1:
                    cells.add((t * Ca + k) * HW + pix)
        idx = np.array(sorted(cells), np.int64)
        return idx, None, np.array([used, skipped, dropped, len(idx)], np.int64)
    idx = np.array(sorted(cnts), np.int64)
    yo = np.array([sums[c] / np.float32(cnts[c]) for c in idx], np.float32)  # cnt = 1e-10f + 1 + ... = the count
    return idx, yo, np.array([used, skipped, dropped, len(idx)], np.int64)


def dense(idx, vals, shape):
    """The dense fp32 grid of a sparse result (vals None: ones, the mask H)."""
    out = np.zeros(int(np.prod(shape)), np.float32)
    out[idx] = 1.0 if vals is None else vals
    return out.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------
# seeded tables for the GPU tests
def random_table(n, n_out, da_win, seed, cells=None, Hs=None, Ws=None, p_none=0.0):
    """n plausible reports: positions over the globe (or confined to `cells` distinct pixel centres of an Hs x Ws grid),
    pressures over and beyond the levels, dt over and beyond the window, both files for da_win 6; about a tenth of the
    values missing (NaN) and a few zero; a few rows without a position, a few out of range (dropped)."""
    rng = np.random.default_rng(seed)
    t = np.empty((n, 12))
    t[:, 0] = rng.integers(0, 2, n) if da_win == 6 else 0
    if cells is None:
        t[:, 1] = rng.uniform(-20, 360, n)
        t[:, 2] = rng.uniform(-90, 90, n)
    else:
        ci = rng.integers(0, Ws, cells)
        cj = rng.integers(0, Hs, cells)
        k = rng.integers(0, cells, n)
        t[:, 1] = ci[k] * 360.0 / Ws
        t[:, 2] = 90.0 - cj[k] * 180.0 / Hs
    lev = levels_of(n_out)
    if cells is None:
        t[:, 3] = t[:, 5] = np.exp(rng.uniform(np.log(30), np.log(1100), n))
    else:  # few levels, so that the cells hold lists
        t[:, 3] = t[:, 5] = rng.choice(lev[-3:], n) * rng.uniform(0.99, 1.01, n)
    t[:, 4] = np.where(t[:, 0] == 0, rng.uniform(-1, 4, n), rng.uniform(-4, 0, n)) if cells is None else \
        np.where(t[:, 0] == 0, 0.1, -1.0)
    t[:, 6] = rng.uniform(100, 30000, n)       # z
    t[:, 7] = rng.uniform(1, 20000, n)         # q
    t[:, 8:10] = rng.normal(0, 15, (n, 2))     # u v
    t[:, 10] = rng.uniform(-80, 40, n)         # t
    t[:, 11] = rng.uniform(950, 1050, n)       # msl
    vals = t[:, 6:]
    vals[rng.random(vals.shape) < 0.1] = np.nan
    vals[rng.random(vals.shape) < 0.02] = 0.0
    if n >= 50:
        bad = rng.choice(n, max(1, n // 50), replace=False)
        t[bad[0::4], 1] = np.nan
        t[bad[1::4], 4] = np.nan
        t[bad[2::4], 1] = 800.0    # an index the reference raises on
        t[bad[3::4], 2] = -300.0
    if p_none:
        t[rng.random(n) < p_none, 5] = np.nan
    return t


def one_cell_table(n, n_out, da_win, seed, order=False):
    """n reports in one pixel, one level (the surface level: nine lists of n) and one time level; order: values
    1e8, 1, -1e8, 1, ... whose fp32 sum depends on the order of the additions."""
    rng = np.random.default_rng(seed)
    t = np.empty((n, 12))
    t[:, 0] = 0
    t[:, 1], t[:, 2] = 123.4, -33.3
    t[:, 3] = t[:, 5] = 1050.0
    t[:, 4] = 0.25
    if order:
        pat = np.array([1e8, 1.0, -1e8, 1.0])
        for c in range(6, 12):
            t[:, c] = np.roll(pat, c)[np.arange(n) % 4] * (1 + (np.arange(n) // 4 % 3))
    else:
        t[:, 6:] = rng.normal(0, 1, (n, 6)) * 10.0 ** rng.integers(-3, 6, (n, 6))
    return t
