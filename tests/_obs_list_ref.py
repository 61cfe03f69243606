"""fp64 numpy restatement of the observation list (include/vaevar.h vv_set_obs_list): the compaction of the dense
observation-space fields into units and records in the documented order, and the evaluation of the observation term
from them. Inputs are the fp32 fields; everything here is float64 / int64.

A unit is one observed column (slot s, group v, pixel p): v = 0 the direct channels 0..3, v = 1..5 the five level
variables; it exists iff some H != 0 among its group's observation channels at p. Units go by slot, then group, then
ascending pixel; a unit's records (o, yo, h, r) -- one per H != 0 -- go by ascending o."""
import numpy as np


def _group(v, n_out):
    return (0, 4) if v == 0 else (4 + n_out * (v - 1), n_out)


def compact_ref(yo, H, R, n_out):
    """yo, H, R (S, 4 + 5*n_out, Hs, Ws) -> dict(uoff int64[6 S + 1], uslot, ugroup, upix int64[units],
    urec int64[units + 1], o int64[records], yo, h, r float64[records], counts int64 (S, 2))."""
    yo, H, R = (np.asarray(a) for a in (yo, H, R))
    S, Ca = H.shape[:2]
    assert Ca == 4 + 5 * n_out
    HW = int(np.prod(H.shape[2:]))
    yo, H, R = (a.reshape(S, Ca, HW) for a in (yo, H, R))
    uoff, uslot, ugroup, upix, nrec, ro, ry, rh, rr = [0], [], [], [], [], [], [], [], []
    for s in range(S):
        for v in range(6):
            c0, nc = _group(v, n_out)
            m = H[s, c0:c0 + nc] != 0                      # (nc, HW)
            pix = np.flatnonzero(m.any(0))                 # ascending
            ui, oi = np.nonzero(m[:, pix].T)               # unit-major, then ascending o
            upix.append(pix)
            uslot.append(np.full(pix.size, s))
            ugroup.append(np.full(pix.size, v))
            nrec.append(m[:, pix].sum(0))
            ro.append(oi)
            for dst, src in ((ry, yo), (rh, H), (rr, R)):
                dst.append(src[s, c0 + oi, pix[ui]].astype(np.float64))
            uoff.append(uoff[-1] + pix.size)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    L = dict(S=S, HW=HW, n_out=n_out, uoff=np.asarray(uoff, np.int64), uslot=cat(uslot, np.int64),
             ugroup=cat(ugroup, np.int64), upix=cat(upix, np.int64), o=cat(ro, np.int64), yo=cat(ry, np.float64),
             h=cat(rh, np.float64), r=cat(rr, np.float64))
    L["urec"] = np.concatenate([[0], np.cumsum(cat(nrec, np.int64))]).astype(np.int64)
    first = L["urec"][L["uoff"][::6]]
    L["counts"] = np.stack([np.diff(L["uoff"][::6]), np.diff(first)], 1).astype(np.int64)
    return L


def eval_ref(L, interp, x, coeff=1.0):
    """The observation term from the list L on the state x (S, 4 + 5*n_in, Hs, Ws), float64: returns dict(J (S,) =
    the slot's sum of h d^2 / r, g (S, C, HW) = coeff * Op^T(h d / r) (zero off the units), gabs (S, C, HW) =
    sum_o |P[o][j]| |g_o| (the scale of the gradient's rounding error), cells bool (S, C, HW): the state cells that
    belong to a unit, dmin = the smallest |d|)."""
    P = np.asarray(interp, np.float64)
    n_out, n_in = P.shape
    x = np.asarray(x, np.float64)
    S, C = x.shape[:2]
    assert C == 4 + 5 * n_in and S == L["S"] and n_out == L["n_out"]
    HW = L["HW"]
    x = x.reshape(S, C, HW)
    nrec = np.diff(L["urec"])
    unit = np.repeat(np.arange(nrec.size), nrec)           # the unit of every record
    s, v, p, o = L["uslot"][unit], L["ugroup"][unit], L["upix"][unit], L["o"]
    J, g, gabs = np.zeros(S), np.zeros((S, C, HW)), np.zeros((S, C, HW))
    cells = np.zeros((S, C, HW), bool)
    d_all = np.zeros(o.size)
    direct = v == 0
    # direct channels: y = x[o]
    sd, pd, od = s[direct], p[direct], o[direct]
    d = x[sd, od, pd] - L["yo"][direct]
    gd = coeff * (L["h"][direct] * d) / L["r"][direct]
    np.add.at(J, sd, L["h"][direct] * d * d / L["r"][direct])
    g[sd, od, pd] = gd
    gabs[sd, od, pd] = np.abs(gd)
    d_all[direct] = d
    # level variables: y = sum_j P[o][j] x[4 + n_in (v - 1) + j]
    lv = ~direct
    sl, vl, pl, ol = s[lv], v[lv], p[lv], o[lv]
    ch = 4 + n_in * (vl - 1)[:, None] + np.arange(n_in)[None]      # (records, n_in)
    xs = x[sl[:, None], ch, pl[:, None]]
    d = (P[ol] * xs).sum(1) - L["yo"][lv]
    gl = coeff * (L["h"][lv] * d) / L["r"][lv]
    np.add.at(J, sl, L["h"][lv] * d * d / L["r"][lv])
    np.add.at(g, (sl[:, None], ch, pl[:, None]), P[ol] * gl[:, None])
    np.add.at(gabs, (sl[:, None], ch, pl[:, None]), np.abs(P[ol]) * np.abs(gl)[:, None])
    d_all[lv] = d
    us, uv, up = L["uslot"], L["ugroup"], L["upix"]
    dm = uv == 0
    cells[us[dm][:, None], np.arange(4)[None], up[dm][:, None]] = True
    chu = 4 + n_in * (uv[~dm] - 1)[:, None] + np.arange(n_in)[None]
    cells[us[~dm][:, None], chu, up[~dm][:, None]] = True
    return dict(J=J, g=g, gabs=gabs, cells=cells, dmin=float(np.abs(d_all).min()) if d_all.size else np.inf)


def x_aug64(interp, x):
    """x_aug (S, 4 + 5*n_out, ...) of x (S, 4 + 5*n_in, ...) in float64."""
    P = np.asarray(interp, np.float64)
    n_out, n_in = P.shape
    x = np.asarray(x, np.float64)
    parts = [x[:, :4]]
    for i in range(5):
        parts.append(np.einsum("oj,sj...->so...", P, x[:, 4 + n_in * i:4 + n_in * (i + 1)]))
    return np.concatenate(parts, 1)
