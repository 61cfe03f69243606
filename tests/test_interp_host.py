"""CPU: da_mode 'interpolation' (da_4dvar.py:968-1061). The numpy restatement the GPU tests compare against
(tests/_interp_ref.py: integer edge functions, lowest simplex first, one fp64 expression) reproduces scipy's
griddata(method='linear') on the golden cases (tests/golden/g18_interpolation.npz, tools/make_interp_fixture.py) and,
where scipy imports, on live seeded masks: the NaN / hull set exactly, every value within ONE fp32 ulp of the
channel's largest |vertex value|. That bound is derived, not fitted: both sides form a convex combination of the
vertex values in fp64 and round it once to fp32, so both results lie within half an ulp (of a magnitude no larger
than the largest vertex) of the exact one, apart from fp64 rounding that is eight orders smaller. Also here:
vaevar.interp.pack_triangles' table, and the argument validation of vv_tri_interp and vv_obs_project."""
import ctypes
import os

import numpy as np
import pytest

from _interp_ref import (BAND, CASES, COLS, GRIDS, SEG, background, kernel_cases, nan_safe_vertex, table_from,
                         tri_interp_ref, ulp32)
from conftest import GOLD, check


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g18_interpolation.npz"))


def compare_with_griddata(name, out, bg, H, yo, lin_by_channel, owner, rule):
    """out: the restatement's field; lin_by_channel[c]: griddata at np.argwhere(H[c] == 0) (None: channel without
    rows, which must be untouched). Returns the largest error in ulps of the channel's largest |vertex|."""
    writers, rule_owner = rule
    free = H != 1  # the local rule may claim a vertex twice; a vertex is observed and never written
    assert int(writers[free].max(initial=0)) <= 1, f"{name}: a cell with two writers"
    assert np.array_equal(rule_owner[free], owner[free]), f"{name}: neighbour rule != lowest simplex index"
    worst = 0.0
    for c, lin in enumerate(lin_by_channel):
        same = out[c].view(np.uint32) == bg[c].view(np.uint32)
        assert same[H[c] != 0].all(), f"{name} channel {c}: a cell with H != 0 was written"
        if lin is None:
            assert same.all(), f"{name} channel {c}: no rows, yet written"
            continue
        at = np.argwhere(H[c] == 0)
        got, kept = out[c][at[:, 0], at[:, 1]], same[at[:, 0], at[:, 1]]
        assert np.array_equal(kept, np.isnan(lin)), f"{name} channel {c}: the NaN / hull set differs from griddata"
        vmax = np.nanmax(np.abs(yo[c][H[c] == 1]))
        err = np.abs(got[~kept].astype(np.float64) - lin[~kept].astype(np.float64)).max(initial=0.0) / ulp32(vmax)
        worst = max(worst, float(err))
    return worst


@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_restatement_reproduces_griddata_on_the_golden_cases(gold, gi):
    yo, H, cases, lin = kernel_cases(gold, gi)
    Hs, Ws = GRIDS[gi]
    table = table_from(cases, Hs, Ws)
    bg = background(H.shape, gi)
    out, stats, owner, rule = tri_interp_ref(table, yo, H, bg)
    assert stats[0] == len(table) and stats[1] == 0 and stats[2] > 0
    assert cases[CASES.index("few")] is None and cases[CASES.index("corners")] is not None
    worst = compare_with_griddata(f"g18 grid {Hs}x{Ws}", out, bg, H, yo, lin, owner, rule)
    check(f"g18 grid {Hs}x{Ws}: restatement vs griddata, ulps of the largest vertex", worst, 1.0, "<=")
    # what the cases are there for
    nan_c, nb_c, cor = CASES.index("nan_vertex"), CASES.index("nonbinary"), CASES.index("corners")
    assert np.isnan(yo[nan_c]).sum() == 1 and ((H[nb_c] != 0) & (H[nb_c] != 1)).sum() == 1
    rows = table[table[:, 0] == cor]
    assert ((rows[:, 1:7:2].max(1) - rows[:, 1:7:2].min(1) == Hs - 1)
            & (rows[:, 2:7:2].max(1) - rows[:, 2:7:2].min(1) == Ws - 1)).any()  # a box covering the whole grid
    assert (table[:, 11] - table[:, 10]).max() > 1 or Ws <= SEG  # boxes cut into several tiles


def station_like(rng, Hs, Ws):
    m = np.zeros((Hs, Ws), bool)
    for _ in range(5):
        r0, c0 = rng.uniform(0, Hs), rng.uniform(0, Ws)
        rr = np.clip(np.round(rng.normal(r0, 2.0, 10)), 0, Hs - 1).astype(int)
        cc = np.clip(np.round(rng.normal(c0, 3.0, 10)), 0, Ws - 1).astype(int)
        m[rr, cc] = True
    m[Hs // 2, 1:Ws - 1:2] = True
    m[2:Hs - 2:2, Ws // 4] = True
    k = np.arange(min(Hs, Ws) - 3)
    m[k + 2, k + 1] = True
    return m


def test_restatement_reproduces_a_live_griddata():
    pytest.importorskip("scipy")
    from scipy.interpolate import griddata
    from scipy.spatial import Delaunay

    from vaevar.interp import pack_triangles

    Hs, Ws = 29, 71
    rng = np.random.default_rng(2718)
    masks = [rng.random((Hs, Ws)) < d for d in (0.05, 0.2, 0.5, 0.9)] + [station_like(rng, Hs, Ws)]
    masks.append(rng.random((Hs, Ws)) < 0.1)   # with a NaN observation
    masks.append(rng.random((Hs, Ws)) < 0.15)  # with the four grid corners on the hull
    masks[-1][[0, 0, -1, -1], [0, -1, 0, -1]] = True
    masks.append(rng.random((Hs, Ws)) < 0.3)   # with a mask value that is neither 0 nor 1
    H = np.stack(masks).astype(np.float32)
    C = len(H)
    r, c = np.argwhere(H[-1] == 0)[100]
    H[-1, r, c] = 0.25
    yo = ((260.0 + 40.0 * rng.standard_normal(H.shape)) * (H == 1)).astype(np.float32)
    cells = [np.argwhere(H[k] == 1) for k in range(C)]
    table = pack_triangles(cells)
    r, c = cells[5][nan_safe_vertex(cells[5], Delaunay(cells[5]).simplices, H[5])]
    yo[5, r, c] = np.nan
    assert np.array_equal(table[:, 0], np.sort(table[:, 0])) and set(table[:, 0]) == set(range(C))
    lin = [griddata(cells[k], yo[k][H[k] == 1], np.argwhere(H[k] == 0), method="linear").astype(np.float32)
           for k in range(C)]
    bg = background(H.shape, 9)
    out, stats, owner, rule = tri_interp_ref(table, yo, H, bg)
    assert stats[1] == 0
    worst = compare_with_griddata("live", out, bg, H, yo, lin, owner, rule)
    check("live griddata: restatement, ulps of the largest vertex", worst, 1.0, "<=")


def _fake_triangulate(calls):
    def tri(points):
        calls.append(np.array(points))
        m = len(points) - 2  # a fan around point 0; the neighbours are made up but recognisable
        simp = np.stack([np.zeros(m, int), np.arange(1, m + 1), np.arange(2, m + 2)], 1)
        nbr = np.stack([np.full(m, -1), np.arange(1, m + 1), np.arange(-1, m - 1)], 1)
        nbr[nbr >= m] = -1
        return simp, nbr
    return tri


def test_pack_triangles_layout_offsets_and_sharing():
    from vaevar.interp import MIN_CELLS, TRI_BAND, TRI_COLS, TRI_SEG, pack_triangles

    assert (TRI_COLS, TRI_BAND, TRI_SEG, MIN_CELLS) == (COLS, BAND, SEG, 10)
    rng = np.random.default_rng(5)

    def cells(k, Hs=40, Ws=300):
        idx = np.sort(rng.choice(Hs * Ws, k, replace=False))
        return np.stack([idx // Ws, idx % Ws], 1)

    a, b = cells(11), cells(30)
    chans = [a, cells(10), None, b, a.copy(), np.zeros((0, 2), int), cells(3)]
    calls = []
    t = pack_triangles(chans, _fake_triangulate(calls))
    assert t.dtype == np.int32 and t.shape == (9 + 28 + 9, TRI_COLS)
    assert len(calls) == 2  # channels 0 and 4 share one triangulation; 10 cells or fewer: no rows, no call
    assert t[:, 0].tolist() == [0] * 9 + [3] * 28 + [4] * 9
    for ch, pts, first in ((0, a, 0), (3, b, 9), (4, a, 37)):
        blk = t[t[:, 0] == ch]
        m = len(pts) - 2
        for k, vert in enumerate((np.zeros(m, int), np.arange(1, m + 1), np.arange(2, m + 2))):
            assert np.array_equal(blk[:, 1 + 2 * k], pts[vert, 0]) and np.array_equal(blk[:, 2 + 2 * k], pts[vert, 1])
        assert (blk[:, 7] == -1).all()
        assert blk[:, 8].tolist() == [first + k if k < m else -1 for k in range(1, m + 1)]  # offset to table rows
        assert blk[:, 9].tolist() == [-1] + [first + k for k in range(m - 1)]
    rr, cc = t[:, 1:7:2], t[:, 2:7:2]
    tiles = ((rr.max(1) - rr.min(1)) // TRI_BAND + 1) * ((cc.max(1) - cc.min(1)) // TRI_SEG + 1)
    assert tiles.max() > 1
    assert np.array_equal(t[:, 11] - t[:, 10], tiles) and t[0, 10] == 0 and np.array_equal(t[1:, 10], t[:-1, 11])
    assert np.array_equal(t, table_from([(a, *_fake_triangulate([])(a)), None, None, (b, *_fake_triangulate([])(b)),
                                         (a, *_fake_triangulate([])(a))], 40, 300))
    empty = pack_triangles([cells(10), None], _fake_triangulate(calls))
    assert empty.shape == (0, TRI_COLS) and empty.dtype == np.int32 and len(calls) == 2
    with pytest.raises(ValueError):
        pack_triangles([np.zeros((12, 3), int)], _fake_triangulate(calls))


def test_pack_triangles_default_is_scipy_delaunay_and_collinear_cells_raise(gold):
    pytest.importorskip("scipy")
    from scipy.spatial import QhullError

    from vaevar.interp import pack_triangles

    _, _, cases, _ = kernel_cases(gold, 0)
    t = pack_triangles([None if k is None else k[0] for k in cases])
    assert np.array_equal(t, table_from(cases, *GRIDS[0]))  # the stored simplices are what Delaunay gives here
    row = np.stack([np.full(20, 7), np.arange(20) * 2], 1)  # a mask with one row of cells
    with pytest.raises(QhullError):
        pack_triangles([row])


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_interp_exported_and_versioned():
    from vaevar import _lib

    for name in ("vv_tri_interp", "vv_obs_project"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert _lib.lib.vv_version() >= 107


TRI_BAD = {"null_ctx": dict(ctx=None), "null_yo": dict(yo=None), "null_H": dict(H=None), "null_xa": dict(xa=None),
           "n_negative": dict(n=-1), "null_tris": dict(tris=None), "n_2^31": dict(n=2 ** 31), "C_0": dict(C=0),
           "Hs_0": dict(Hs=0), "Ws_0": dict(Ws=0), "Hs_16385": dict(Hs=16385), "Ws_16385": dict(Ws=16385),
           "xa_is_yo": dict(alias="yo"), "xa_is_H": dict(alias="H"), "xa_overlaps_yo": dict(alias="yo+")}


@pytest.mark.parametrize("case", list(TRI_BAD))
def test_tri_interp_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep = [ctypes.create_string_buffer(1 << 12) for _ in range(4)]  # never dereferenced
    b, yo, H, xa = (ctypes.cast(k, ctypes.c_void_p) for k in keep)
    a = dict(ctx=b, tris=b, n=10, yo=yo, H=H, xa=xa, C=2, Hs=8, Ws=8)
    over = dict(TRI_BAD[case])
    alias = over.pop("alias", None)
    a.update(over)
    if alias:
        a["xa"] = ctypes.c_void_p(a[alias[:2].strip("+")].value + (64 if alias.endswith("+") else 0))
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001  # another message first, so the one below is this call's
    before = _msg(lib)
    rc = lib.vv_tri_interp(a["ctx"], a["tris"], a["n"], a["yo"], a["H"], a["xa"], a["C"], a["Hs"], a["Ws"], None, None)
    assert rc == 1001
    assert _msg(lib) and _msg(lib) != before


PROJ_BAD = {"null_ctx": dict(ctx=None), "null_interp_inv": dict(P=None), "null_x_aug": dict(x_aug=None),
            "null_x": dict(x=None), "n_in_0": dict(n_in=0), "n_in_65": dict(n_in=65), "n_out_0": dict(n_out=0),
            "n_out_17": dict(n_out=17), "T_0": dict(T=0), "Hs_0": dict(Hs=0), "Ws_0": dict(Ws=0),
            "HW_2^31": dict(Hs=32768, Ws=65536), "x_is_x_aug": dict(alias=True)}


@pytest.mark.parametrize("case", list(PROJ_BAD))
def test_obs_project_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep = [ctypes.create_string_buffer(1 << 12) for _ in range(3)]
    b, x_aug, x = (ctypes.cast(k, ctypes.c_void_p) for k in keep)
    a = dict(ctx=b, P=b, n_out=13, n_in=40, x_aug=x_aug, x=x, T=1, Hs=8, Ws=8)
    over = dict(PROJ_BAD[case])
    if over.pop("alias", False):
        over["x"] = a["x_aug"]
    a.update(over)
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    rc = lib.vv_obs_project(a["ctx"], a["P"], a["n_out"], a["n_in"], a["x_aug"], a["x"], a["T"], a["Hs"], a["Ws"], None)
    assert rc == 1001
    assert _msg(lib) and _msg(lib) != before


def test_cyclic_da_still_refuses_the_mode_and_names_the_class():
    from vaevar.cycle import DA_MODES, CyclicDA, CyclicInterpolation

    assert DA_MODES == ("vae4dvar", "sc4dvar", "free_run") and issubclass(CyclicInterpolation, CyclicDA)
    with pytest.raises(NotImplementedError, match="CyclicInterpolation"):
        CyclicDA(None, None, None, None, Nit=1, name="x", da_mode="interpolation")
    with pytest.raises(NotImplementedError):
        CyclicDA(None, None, None, None, Nit=1, name="x", da_mode="nudging")


def test_a_nan_anywhere_differs_from_griddata_only_where_griddata_is_undefined():
    """A NaN at an arbitrary vertex: the restatement's NaN set may differ from griddata's only at cells that lie exactly
    on the edge opposite the NaN vertex, i.e. in a simplex that holds the NaN with weight 0 and in a finite one; there
    griddata returns whichever simplex its walk reached, the restatement the lower row. Everywhere else the sets agree,
    and the case is not empty (the seed gives such cells)."""
    pytest.importorskip("scipy")
    from scipy.interpolate import griddata
    from scipy.spatial import Delaunay

    Hs, Ws = 33, 47
    rng = np.random.default_rng(1805)
    on_edges = 0
    for trial in range(6):
        m = rng.random((Hs, Ws)) < 0.05
        cells = np.argwhere(m)
        vals = rng.standard_normal(len(cells)).astype(np.float32)
        v = int(rng.integers(len(cells)))
        vals[v] = np.nan
        tri = Delaunay(cells)
        H = m.astype(np.float32)[None]
        yo = np.zeros_like(H)
        yo[0, cells[:, 0], cells[:, 1]] = vals
        bg = background(H.shape, trial)
        table = table_from([(cells, tri.simplices, tri.neighbors)], Hs, Ws)
        out, _, owner, _ = tri_interp_ref(table, yo, H, bg)
        free = np.argwhere(H[0] == 0)
        lin = griddata(cells, vals, free, method="linear")
        kept = (out[0].view(np.uint32) == bg[0].view(np.uint32))[free[:, 0], free[:, 1]]
        for r, c in free[kept != np.isnan(lin)]:
            inside = []
            for s in tri.simplices:
                (r0, c0), (r1, c1), (r2, c2) = cells[s]
                A = (r1 - r0) * (c2 - c0) - (c1 - c0) * (r2 - r0)
                e = np.array([(r1 - r) * (c2 - c) - (c1 - c) * (r2 - r), (r2 - r) * (c0 - c) - (c2 - c) * (r0 - r), 0])
                e[2] = A - e[0] - e[1]
                e *= 1 if A > 0 else -1
                if (e >= 0).all():
                    inside.append((v in s, bool(e[list(s).index(v)] == 0) if v in s else None))
            assert len(inside) == 2 and sorted(x[0] for x in inside) == [False, True], (trial, r, c, inside)
            assert [x[1] for x in inside if x[0]] == [True]  # the NaN vertex has weight 0 there
            on_edges += 1
    assert on_edges > 0
