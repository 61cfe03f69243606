"""Numpy restatement of vv_tri_interp and vv_obs_project (include/vaevar.h), independent of vaevar.interp and of the
kernels; pinned to scipy's griddata(method='linear') by tests/golden/g18_interpolation.npz
(tools/make_interp_fixture.py, tests/test_interp_host.py).

tri_interp_ref walks the table rows in order, lowest index first: a cell goes to the first valid row whose simplex
contains it (integer edge functions, edges inclusive). The neighbour rule of the kernel (a cell on an edge belongs to
the row if the hull or a later row lies across it) is evaluated beside it, so that the tests can assert that both
give the same owner and that no cell has two writers. The value is ((e0 v0 + e1 v1) + e2 v2) / A in fp64, numpy
rounding every operation on its own, cast once to fp32."""
import numpy as np

COLS, BAND, SEG = 12, 16, 64


def ulp32(x):
    """One fp32 unit in the last place of |x| (x > 0 finite), as a float64."""
    x = np.float32(abs(x))
    return float(np.nextafter(x, np.float32(np.inf)) - x)


def row_ok(row, n, C, Hs, Ws):
    ch, r0, c0, r1, c1, r2, c2, n0, n1, n2 = (int(v) for v in row[:10])
    if not (0 <= ch < C and all(0 <= r < Hs for r in (r0, r1, r2)) and all(0 <= c < Ws for c in (c0, c1, c2))):
        return False
    if not all(-1 <= k < n for k in (n0, n1, n2)):
        return False
    return (r1 - r0) * (c2 - c0) - (c1 - c0) * (r2 - r0) != 0


def tri_interp_ref(table, yo, H, xa):
    """Returns (xa_out, stats[3], owner, rule_writers): owner (C, Hs, Ws) the lowest valid row containing each cell
    (-1 outside every hull), rule_writers the number of rows that claim the cell under the neighbour rule."""
    table = np.asarray(table, np.int64)
    yo, H = np.asarray(yo, np.float32), np.asarray(H, np.float32)
    out = np.array(xa, np.float32, copy=True)
    C, Hs, Ws = out.shape
    n = len(table)
    owner = np.full((C, Hs, Ws), -1, np.int64)
    writers = np.zeros((C, Hs, Ws), np.int32)
    rule_owner = np.full((C, Hs, Ws), -1, np.int64)
    stats = np.zeros(3, np.int64)
    for t, row in enumerate(table):
        if not row_ok(row, n, C, Hs, Ws):
            stats[1] += 1
            continue
        stats[0] += 1
        ch, r0, c0, r1, c1, r2, c2, n0, n1, n2 = (int(v) for v in row[:10])
        A = (r1 - r0) * (c2 - c0) - (c1 - c0) * (r2 - r0)
        sg = 1 if A > 0 else -1
        ra, rb = min(r0, r1, r2), max(r0, r1, r2)
        ca, cb = min(c0, c1, c2), max(c0, c1, c2)
        r, c = np.meshgrid(np.arange(ra, rb + 1), np.arange(ca, cb + 1), indexing="ij")
        e0 = ((r1 - r) * (c2 - c) - (c1 - c) * (r2 - r)) * sg
        e1 = ((r2 - r) * (c0 - c) - (c2 - c) * (r0 - r)) * sg
        e2 = A * sg - e0 - e1
        inside = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
        rule = inside.copy()
        for e, nb in ((e0, n0), (e1, n1), (e2, n2)):
            if not (nb == -1 or t < nb):
                rule &= e != 0
        sub_w = writers[ch, ra:rb + 1, ca:cb + 1]
        sub_w += rule
        sub_r = rule_owner[ch, ra:rb + 1, ca:cb + 1]
        sub_r[rule] = t
        sub_o = owner[ch, ra:rb + 1, ca:cb + 1]
        mine = inside & (sub_o < 0)
        sub_o[mine] = t
        v0, v1, v2 = (np.float64(yo[ch, rr, cc]) for rr, cc in ((r0, c0), (r1, c1), (r2, c2)))
        with np.errstate(invalid="ignore", over="ignore"):
            val = ((e0[mine].astype(np.float64) * v0 + e1[mine].astype(np.float64) * v1)
                   + e2[mine].astype(np.float64) * v2) / np.float64(A * sg)
            val32 = val.astype(np.float32)
        write = (H[ch, ra:rb + 1, ca:cb + 1][mine] == 0) & ~np.isnan(val)
        sub_x = out[ch, ra:rb + 1, ca:cb + 1]
        idx = np.argwhere(mine)[write]
        sub_x[idx[:, 0], idx[:, 1]] = val32[write]
        stats[2] += int(write.sum())
    return out, stats, owner, (writers, rule_owner)


def table_from(cases, Hs, Ws):
    """The vv_tri_interp table of a list of per-channel (cells, simplices, neighbors) triples (None: no rows), built
    here without vaevar.interp."""
    rows, n = [], 0
    for ch, case in enumerate(cases):
        if case is None:
            continue
        pts, simp, nbr = (np.asarray(a, np.int64) for a in case)
        blk = np.zeros((len(simp), COLS), np.int64)
        blk[:, 0] = ch
        for k in range(3):
            blk[:, 1 + 2 * k], blk[:, 2 + 2 * k] = pts[simp[:, k], 0], pts[simp[:, k], 1]
        blk[:, 7:10] = np.where(nbr >= 0, nbr + n, -1)
        rows.append(blk)
        n += len(simp)
    tab = np.concatenate(rows) if rows else np.zeros((0, COLS), np.int64)
    return with_prefix(tab)


def with_prefix(tab):
    """Fill work_begin / work_end from the rows' bounding boxes (clipped differences: a bad row still gets a tile)."""
    tab = np.array(tab, np.int64, copy=True)
    if len(tab):
        rr, cc = tab[:, 1:7:2], tab[:, 2:7:2]
        tiles = ((rr.max(1) - rr.min(1)) // BAND + 1) * ((cc.max(1) - cc.min(1)) // SEG + 1)
        end = np.cumsum(tiles)
        tab[:, 10], tab[:, 11] = end - tiles, end
    return tab.astype(np.int32)


def obs_project_ref(interp_inv, x_aug):
    """(x fp64, bound): x[t, 4 + n_out i + o] = sum_j W[o][j] x_aug[t, 4 + n_in i + j] in fp64 and the per-element
    bound n_in 2^-24 sum_j |W[o][j] x_aug[j]| of an n_in-term fp32 sum; channels 0..3 copied (bound 0)."""
    W = np.asarray(interp_inv, np.float64)
    x_aug = np.asarray(x_aug, np.float64)
    n_out, n_in = W.shape
    parts, bounds = [x_aug[:, :4]], [np.zeros_like(x_aug[:, :4])]
    for i in range(5):
        blk = x_aug[:, 4 + n_in * i:4 + n_in * (i + 1)]
        parts.append(np.einsum("oj,tjhw->tohw", W, blk))
        bounds.append(n_in * 2.0 ** -24 * np.einsum("oj,tjhw->tohw", np.abs(W), np.abs(blk)))
    return np.concatenate(parts, 1), np.concatenate(bounds, 1)


# --- tests/golden/g18_interpolation.npz (tools/make_interp_fixture.py) ---------------------------------------------
GRIDS = ((33, 47), (67, 131), (19, 200))
CASES = ("dense50", "clusters", "tracks", "corners", "few", "nan_vertex", "nonbinary", "clusters_again")


def background(shape, seed=0):
    """A recognisable background: no two cells of a field share their bits, and none is a plausible analysis."""
    n = int(np.prod(shape))
    return (-7.0e6 - 3.0 * seed - 0.5 * np.arange(n, dtype=np.float64)).astype(np.float32).reshape(shape)


def kernel_cases(g, gi):
    """Grid gi of g18(a) as one multi-channel problem: yo, H (C, Hs, Ws), the per-channel (cells, simplices, neighbors)
    triples (None for the channel without rows) and griddata's fp32 results at np.argwhere(H[c] == 0)."""
    Hs, Ws = GRIDS[gi]
    C = len(CASES)
    yo, H = np.zeros((C, Hs, Ws), np.float32), np.zeros((C, Hs, Ws), np.float32)
    cases, lin = [], []
    for ci in range(C):
        key = f"a{gi}_c{ci}_"
        cells = g[key + "cells"].astype(np.int64)
        H[ci, cells[:, 0], cells[:, 1]] = 1
        yo[ci, cells[:, 0], cells[:, 1]] = g[key + "vals"]
        if key + "other" in g.files:
            for r, c, v in g[key + "other"]:
                H[ci, int(r), int(c)] = v
        has = key + "simp" in g.files
        cases.append((cells, g[key + "simp"], g[key + "nbr"]) if has else None)
        lin.append(g[key + "lin"] if has else None)
    return yo, H, cases, lin


def stored_triangulations(g, prefixes):
    """triangulate(points) for vaevar.interp.pack_triangles that answers from the fixture: the stored simplices and
    neighbors of exactly that cell list (KeyError for any other), so that no GPU test runs scipy."""
    known = {}
    for p in prefixes:
        known[g[p + "cells"].astype(np.int64).tobytes()] = (g[p + "simp"], g[p + "nbr"])

    def triangulate(points):
        return known[np.ascontiguousarray(points, np.int64).tobytes()]

    return triangulate


def nan_safe_vertex(cells, simplices, H):
    """Index of an observed cell that can carry a NaN observation with a well-defined griddata answer. A cell on the
    edge opposite a NaN vertex lies in two simplices, one NaN (0 * NaN) and one finite; which of them scipy's
    find_simplex walk returns depends on where the walk came from, not on the data, so griddata has no canonical value
    there (vv_tri_interp takes the lower table row). The vertex returned has no unobserved lattice cell on any edge
    opposite it: every such edge has coprime steps, or only observed cells (H == 1) between its ends. Searched from
    the middle of the cell list."""
    cells, simplices = np.asarray(cells, np.int64), np.asarray(simplices, np.int64)
    n = len(cells)
    for v in list(range(n // 2, n)) + list(range(n // 2)):
        ok = True
        for s in simplices[(simplices == v).any(1)]:
            a, b = (cells[k] for k in s if k != v)
            g = int(np.gcd(abs(a[0] - b[0]), abs(a[1] - b[1])))
            for k in range(1, g):
                r, c = a + (b - a) // g * k
                ok &= H[r, c] == 1
        if ok:
            return v
    raise ValueError("no vertex whose opposite edges are free of unobserved cells")
