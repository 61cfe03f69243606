"""CPU: vv_obs_grid (get_real_obs / get_obs_mask, da_4dvar.py:301-440 / :190-274) validates its arguments before any
device work; the report table (vaevar.reports.pack_reports) and the level tables (level_tables) are the reference's
expressions; and the per-row restatement the GPU tests compare against (tests/_obs_grid_ref.py) reproduces BITWISE
what the reference itself made of the golden reports (tests/golden/g17_obs_grid.npz, tools/make_obs_grid_fixture.py):
that is the pin of the whole feature to the reference."""
import ctypes
import os

import numpy as np
import pytest

from _obs_grid_ref import HEIGHT_MASK, MASK, REAL, levels_of, obs_grid_ref, one_cell_table, random_table
from conftest import GOLD


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_obs_grid_exported_and_versioned():
    from vaevar import _lib

    assert "vv_obs_grid" in _lib.EXPORTED and hasattr(_lib.lib, "vv_obs_grid")
    assert _lib.lib.vv_version() >= 105


BAD = {"null_ctx": dict(ctx=None), "null_H": dict(H=None), "null_yo_real": dict(yo=None),
       "null_reports": dict(rep=None), "n_negative": dict(n=-1), "mode_2": dict(mode=2), "mode_negative": dict(mode=-1),
       "da_win_0": dict(da_win=0), "da_win_2": dict(da_win=2), "da_win_3": dict(da_win=3), "da_win_7": dict(da_win=7),
       "n_lev_0": dict(n_lev=0), "n_lev_65": dict(n_lev=65), "Hs_0": dict(Hs=0), "Ws_0": dict(Ws=0),
       "null_bounds": dict(bounds=None), "null_log_lev": dict(log_lev=None), "null_zcoef": dict(zcoef=None),
       "null_tcoef": dict(tcoef=None), "yo_is_H": dict(alias=True),
       "cells_2^31": dict(da_win=6, n_lev=40, Hs=1024, Ws=2048),  # 6 * 204 * 2^21 > 2^31
       "cells_2^31_mask": dict(mode=1, yo=None, da_win=1, n_lev=13, Hs=4096, Ws=8192),
       "9n+1_2^31": dict(n=(2 ** 31 - 2) // 9 + 1)}


@pytest.mark.parametrize("case", list(BAD))
def test_obs_grid_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep = [ctypes.create_string_buffer(1 << 12) for _ in range(2)]  # never dereferenced
    b, b2 = (ctypes.cast(k, ctypes.c_void_p) for k in keep)
    a = dict(ctx=b, rep=b, n=10, mode=0, da_win=6, n_lev=40, Hs=8, Ws=8, bounds=b, log_lev=b, zcoef=b, tcoef=b, yo=b,
             H=b2)
    over = dict(BAD[case])
    if over.pop("alias", False):
        over["H"] = a["yo"]
    a.update(over)
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001  # another message first, so the one below is this call's
    before = _msg(lib)
    rc = lib.vv_obs_grid(a["ctx"], a["rep"], a["n"], a["mode"], a["da_win"], a["n_lev"], a["Hs"], a["Ws"], a["bounds"],
                         a["log_lev"], a["zcoef"], a["tcoef"], a["yo"], a["H"], None, None)
    assert rc == 1001
    after = _msg(lib)
    assert after and after != before


def test_pack_reports_order_nans_and_src():
    from vaevar.reports import COLUMNS, pack_reports

    d = {"zz": {"position": [10.0, -5.0, 500.0, 0.25], "value": [501.0, 5500.0, 3000.0, 4.0, -2.0, -12.5, 99.0, 1013.0],
                "type": "x"},
         "aa": {"position": [None, 1.0, None, 0.0], "value": [None, None, 0.0, None, 1.0, None, 5.0, None]},
         "mm": {"position": [359.9, 90, 1000, -3], "value": [1000, 1, 2, 3, 4, 5, 6, 7]}}
    t = pack_reports(d)
    assert COLUMNS == ("src", "lon", "lat", "plev", "dt", "p", "z", "q", "u", "v", "t", "msl")
    assert t.dtype == np.float64 and t.shape == (3, 12)
    assert t[0].tolist() == [0, 10.0, -5.0, 500.0, 0.25, 501.0, 5500.0, 3000.0, 4.0, -2.0, -12.5, 1013.0]  # dict order
    assert np.array_equal(np.isnan(t[1]), [False, True, False, True, False, True, True, False, True, False, True, True])
    assert t[1, 7] == 0.0 and t[1, 9] == 1.0
    assert t[2].tolist() == [0, 359.9, 90, 1000, -3, 1000, 1, 2, 3, 4, 5, 7]  # msl is value[-1], value[6] is not kept
    t1 = pack_reports(d, src=1)
    assert (t1[:, 0] == 1).all() and np.array_equal(t1[:, 1:], t[:, 1:], equal_nan=True)
    assert pack_reports([]).shape == (0, 12) and pack_reports({}, 1).shape == (0, 12)  # read_json's "no obs" value
    both = np.concatenate([pack_reports(d, 0), pack_reports(d, 1)])
    assert both.shape == (6, 12) and both[:3, 0].tolist() == [0, 0, 0] and both[3:, 0].tolist() == [1, 1, 1]


@pytest.mark.parametrize("n_out", [40, 7])
def test_level_tables_are_the_reference_expressions(n_out):
    from vaevar.problem import ObsInterpolater
    from vaevar.reports import MASK_BOUNDS, level_tables

    oi = ObsInterpolater(13, n_out)
    lev = np.round(np.exp(np.linspace(3.91202301, 6.90775528, n_out)))  # :68
    assert np.array_equal(oi.height_level_new, lev)
    height = np.zeros(n_out - 1)  # :311-313
    for i in range(len(height)):
        height[i] = np.sqrt(lev[i] * lev[i + 1])
    zc = [61245 if i == 0 else 62000 if i <= 16 else 927.87 * i + 47138.48 for i in range(n_out)]  # :315-321
    tc = [0 if i <= 21 else -25 for i in range(n_out)]  # :323-327
    for src in (oi, lev, list(lev)):
        bounds, log_lev, zcoef, tcoef = level_tables(src)
        assert all(a.dtype == np.float64 for a in (bounds, log_lev, zcoef, tcoef))
        assert np.array_equal(bounds, height) and np.array_equal(zcoef, zc) and np.array_equal(tcoef, tc)
        assert log_lev.tolist() == [float(np.log(x)) for x in lev]  # :353, the scalar np.log
    assert MASK_BOUNDS.tolist() == HEIGHT_MASK and MASK_BOUNDS.dtype == np.float64


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g17_obs_grid.npz"))


@pytest.mark.parametrize("name", ["real_w1_n40", "real_w6_n7", "mask_w6"])
def test_restatement_reproduces_the_reference_bitwise(gold, name):
    """H (the set of observed cells) and yo (fp32 bit patterns) at 721 x 1440 equal what the reference's get_real_obs
    / get_obs_mask returned for the same reports; no row of the fixture is one the reference raises on."""
    da_win, n_out = (int(x) for x in gold[name + "_meta"])
    mask = name.startswith("mask")
    idx, yo, stats = obs_grid_ref(gold[name + "_table"], MASK if mask else REAL, da_win, levels_of(n_out), 721, 1440)
    assert np.array_equal(idx, gold[name + "_idx"])
    assert stats[2] == 0 and stats[3] == len(idx) and stats[:3].sum() == len(gold[name + "_table"])
    assert stats[0] > 100 and stats[1] > 5
    if not mask:
        ref = gold[name + "_yo"]
        assert yo.dtype == np.float32 and ref.dtype == np.float32
        assert np.array_equal(yo.view(np.uint32), ref.view(np.uint32))


def test_fixture_covers_what_it_must(gold):
    t = gold["real_w6_n7_table"]
    assert 200 <= len(t) <= 600
    for col in (1, 2, 3, 4):
        assert np.isnan(t[:, col]).any()
    assert (t[:, 10] == 0.0).any() and np.isnan(t[:, 6:]).any()
    assert {0.125, 0.375, 359.875}.issubset(set(t[:, 1])) and (t[:, 1] < 0).any()
    assert {90.0, -90.0}.issubset(set(t[:, 2]))
    for src, edges in ((0, (-0.5, 0.5, 1.5, 2.5)), (1, (-2.5, -1.5, -0.5))):
        assert set(edges).issubset(set(t[t[:, 0] == src, 4]))
    lev = levels_of(7)
    assert float(np.sqrt(lev[2] * lev[3])) in set(t[:, 5]) and t[:, 5].min() < lev[0] and t[:, 5].max() > lev[-1]
    # the hit counts of the cells: 2, 3 and about 40, and a t = 3 cell fed from both files
    from collections import Counter

    rows = Counter()
    both = {}
    for r in t:
        if np.isnan(r[1:6]).any() or not (r[8] == r[8] and r[8] != 0):
            continue
        key = (round(r[1] / 360 * 1440), round((90 - r[2]) / 180 * 721), r[5] > 950)
        rows[key] += 1
        both.setdefault(key, set()).add(r[0])
    assert {2, 3}.issubset(set(rows.values())) and max(rows.values()) >= 40
    assert any(len(s) == 2 for s in both.values())


def test_restatement_rules_on_hand_made_rows():
    lev = levels_of(7)
    row = lambda **k: [k.get(c, d) for c, d in (("src", 0), ("lon", 10.0), ("lat", 0.0), ("plev", 500.0), ("dt", 0.0),
                                                ("p", 500.0), ("z", 1.0), ("q", 1.0), ("u", 1.0), ("v", 1.0), ("t", 1.0),
                                                ("msl", np.nan))]
    nan = np.nan
    t = np.array([row(), row(lon=nan), row(lon=800.0), row(lat=-300.0), row(p=nan), row(dt=0.5), row(src=1),
                  row(lon=-10.0), row(lon=359.9), row(lat=-90.0), row(t=0.0, z=nan)], np.float64)
    idx, yo, st = obs_grid_ref(t, REAL, 1, lev, 721, 1440)
    assert st.tolist() == [5, 3, 3, len(idx)]  # lon NaN, dt 0.5 and src 1 skipped; lon 800, lat -300, p NaN dropped
    Ca, HW = 39, 721 * 1440
    pix = {int(i % HW) for i in idx}
    assert pix == {360 * 1440 + 40, 360 * 1440 + 1400, 360 * 1440 + 0, 720 * 1440 + 40}
    idx6, _, st6 = obs_grid_ref(t, REAL, 6, lev, 721, 1440)
    assert st6.tolist() == [6, 2, 3, len(idx6)] and (idx6 // (Ca * HW)).max() == 1  # dt 0.5 is time level 1 now
    with pytest.raises(NotImplementedError):
        obs_grid_ref(t, REAL, 3, lev, 721, 1440)
    # the order of the fp32 additions is the row order
    o = one_cell_table(8, 7, 1, 1, order=True)
    _, yo_o, _ = obs_grid_ref(o, REAL, 1, lev, 33, 47)
    _, yo_r, _ = obs_grid_ref(o[::-1], REAL, 1, lev, 33, 47)
    assert not np.array_equal(yo_o, yo_r)
    r = random_table(300, 7, 6, 3, p_none=0.05)
    _, _, sm = obs_grid_ref(r, MASK, 6, None, 33, 47)
    _, _, sr = obs_grid_ref(r, REAL, 6, lev, 33, 47)
    assert sm[2] < sr[2] and sm[0] > sr[0]  # a NaN p drops the row in the real mode only
