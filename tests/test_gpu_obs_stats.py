"""vv_obs_stats / fields.obs_stats (the O-B / O-A departure moments of a window per time level and observation channel;
include/vaevar.h) on the GPU against the numpy restatement of tests/_obs_stats_ref.py.

Two references. (1) The restatement on the GPU's own operator output (obs_augment, downloaded): the fp32 departures
and J terms are then the kernel's bit for bit, so rows COUNT and H are exact and every other row is within the bound of
the fixed fp64 tree, 2 n 2^-53 sum|term| with n = Hs Ws. (2) The pure-CPU restatement (the operator as F.linear,
da_4dvar.py:770-776): the same bound for the identity, whose d is bit-exact; with an operator the bound propagated
from the operator's 1e-6 max|x_aug_c| through each term (_obs_stats_ref.operator_bound).

Grids: 33 x 47 = 1551 cells (the element path, one ragged chunk), 1 x 300 (the 16-byte path, one row), 67 x 131 = 8777
(three 4096-cell chunks, the last ragged). Operators 13 -> 40, 13 -> 7 and the identity with C = 69; T = 1, and T = 3
with the middle slice of H all zero; densities 2 % and 100 %; with and without xa_win."""
import numpy as np
import pytest
import torch

import _obs_stats_ref as Rf
from _obs_qc_ref import gt_aug_ref
from conftest import check, check_bitwise

pytestmark = pytest.mark.gpu

GRIDS = {"33x47": (33, 47), "1x300": (1, 300), "67x131": (67, 131)}
OPS = {"r40": 40, "r7": 7, "id": 0}
CASES = [(g, o, T, d) for g in GRIDS for o in OPS for T in (1, 3) for d in (0.02, 1.0)]
BASE = [i for i in range(Rf.NSTAT) if i not in Rf.ANALYSIS_ROWS]


def _id(c):
    return f"{c[0]}-{c[1]}-T{c[2]}-d{c[3]}"


@pytest.fixture(scope="module")
def ctx():
    from vaevar.engine import Context

    return Context.get(0)


_CASES: dict = {}


def _case(key):
    """The seeded inputs of a case, on the host and on the device, made once and never modified."""
    if key not in _CASES:
        g, o, T, d = key
        c = Rf.make_case(*GRIDS[g], T=T, n_out=OPS[o], seed=7100 + 7 * CASES.index(key), density=d,
                         zero_slice=1 if T == 3 else None)
        c["dev"] = {k: c[k].cuda() for k in ("xb", "xa", "yo", "H", "R")}
        c["dev"]["interp"] = None if c["interp"] is None else torch.from_numpy(c["interp"]).cuda()
        _CASES[key] = c
    return _CASES[key]


def _run(ctx, d, **over):
    from vaevar.engine import obs_stats

    a = dict(d, **over)
    return obs_stats(ctx, a["xb"], a["xa"], a["yo"], a["H"], a["R"], a["interp"])


def _within(tag, tab, ref, bound, rows):
    """max over the rows' entries of |tab - ref| / bound <= 1, exact where the bound is 0; recorded per row."""
    for i in rows:
        err, b = np.abs(tab[:, :, i] - ref[:, :, i]), bound[:, :, i]
        assert np.isfinite(err).all() and np.isfinite(b).all(), (tag, Rf.NAMES[i])
        pos = b > 0
        check(f"{tag} row {Rf.NAMES[i]}: max |sum - exact| / bound", (err[pos] / b[pos]).max() if pos.any() else 0.0,
              1.0, "<=")
        check(f"{tag} row {Rf.NAMES[i]}: entries with a zero bound", err[~pos].sum() if (~pos).any() else 0.0, 0.0,
              "==")


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_obs_stats_vs_restatement(ctx, key):
    from vaevar.engine import obs_augment

    c = _case(key)
    d = c["dev"]
    n = c["xb"].shape[-2] * c["xb"].shape[-1]
    tag = _id(key)
    out = _run(ctx, d)
    assert out.shape == (c["yo"].shape[0], c["yo"].shape[1], 10) and out.dtype == torch.float64 and out.is_cuda
    tab = out.cpu().numpy()
    stat_rows = [i for i in range(Rf.NSTAT) if i not in (Rf.COUNT, Rf.H)]
    # (1) the restatement on the GPU's own operator output
    if d["interp"] is None:
        ab, aa = c["xb"], c["xa"]
    else:
        ab, aa = (obs_augment(ctx, d["interp"], d[k]).cpu() for k in ("xb", "xa"))
    terms = Rf.terms_ref(ab, aa, c["yo"], c["H"], c["R"])
    ref, mag = Rf.table_ref(ab, aa, c["yo"], c["H"], c["R"], terms)
    check_bitwise(f"{tag} row count", tab[:, :, Rf.COUNT], ref[:, :, Rf.COUNT])
    check_bitwise(f"{tag} row h", tab[:, :, Rf.H], ref[:, :, Rf.H])
    check_bitwise(f"{tag} row count vs the mask", tab[:, :, Rf.COUNT], (c["H"] != 0).sum((2, 3)).double())
    _within(f"{tag} vs restatement on the device operator", tab, ref, Rf.tree_bound(n, mag), stat_rows)
    # (2) the pure-CPU restatement
    if d["interp"] is not None:
        cb, ca = gt_aug_ref(c["xb"], c["interp"]), gt_aug_ref(c["xa"], c["interp"])
        terms = Rf.terms_ref(cb, ca, c["yo"], c["H"], c["R"])
        ref2, mag2 = Rf.table_ref(cb, ca, c["yo"], c["H"], c["R"], terms)
        bound2 = Rf.operator_bound(cb, ca, c["yo"], c["H"], c["R"], n, terms, mag2)
        _within(f"{tag} vs pure-CPU restatement (operator bound)", tab, ref2, bound2, stat_rows)
    # the second call
    check_bitwise(f"{tag} second call", _run(ctx, d), out)
    # without the analysis: its rows are NaN, the others keep their bits; no xa_win buffer is passed at all
    tab_n = _run(ctx, d, xa=None).cpu().numpy()
    assert np.isnan(tab_n[:, :, list(Rf.ANALYSIS_ROWS)]).all()
    check_bitwise(f"{tag} without xa_win, the other rows", tab_n[:, :, BASE], tab[:, :, BASE])
    assert not np.isnan(tab).any()
    # xa_win = xb_win
    same = _run(ctx, d, xa=d["xb"]).cpu().numpy()
    for a, b in ((Rf.OA, Rf.OB), (Rf.OA2, Rf.OB2), (Rf.OAOB, Rf.OB2), (Rf.JA, Rf.JB)):
        check_bitwise(f"{tag} xa_win = xb_win: {Rf.NAMES[a]} == {Rf.NAMES[b]}", same[:, :, a], same[:, :, b])
    check_bitwise(f"{tag} xa_win = xb_win, the other rows", same[:, :, BASE], tab[:, :, BASE])
    if key[2] == 3:
        assert not tab[1].any() and tab[0, :, Rf.COUNT].any()  # the all-zero middle slice: every sum is +0


@pytest.mark.parametrize("key", [k for k in CASES if k[2] == 3], ids=_id)
def test_obs_stats_rows_do_not_depend_on_T(ctx, key):
    d = _case(key)["dev"]
    full = _run(ctx, d)
    for t in range(3):
        one = _run(ctx, {k: (v if k == "interp" else v[t:t + 1].contiguous()) for k, v in d.items()})
        check_bitwise(f"{_id(key)} slice {t} of the T = 3 call vs the T = 1 call", full[t:t + 1], one)


def _shifted(t):
    """A copy of t whose first element lies one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, device=t.device, dtype=t.dtype)
    off = 1 + (-(buf.data_ptr() // 4)) % 4
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("key", [("1x300", "r40", 3, 0.02), ("1x300", "id", 1, 1.0), ("1x300", "r7", 1, 1.0),
                                 ("67x131", "r40", 1, 0.02)], ids=_id)
def test_obs_stats_unaligned_views(ctx, key):
    d = _case(key)["dev"]
    for k in ("xb", "xa", "yo", "H", "R"):
        assert d[k].data_ptr() % 16 == 0
    out = _run(ctx, d)
    for which in (("xb",), ("xa",), ("yo",), ("H",), ("R",), ("xb", "xa", "yo", "H", "R")):
        moved = {k: _shifted(d[k]) for k in which}
        check_bitwise(f"{_id(key)} {'+'.join(which)} one element off alignment", _run(ctx, d, **moved), out)


@pytest.mark.parametrize("key", [("33x47", "r40", 3, 0.02), ("67x131", "r7", 1, 0.02), ("1x300", "id", 3, 0.02),
                                 ("1x300", "r40", 1, 0.02), ("67x131", "id", 1, 0.02)], ids=_id)
def test_obs_stats_ignores_unobserved_entries(ctx, key):
    """NaN in yo and R wherever H == 0, and in both windows wherever no observed channel reads the state (a surface or
    identity channel reads its own channel, the channels of a pressure-level variable its 13 levels), change no bit."""
    c = _case(key)
    d = c["dev"]
    n_out = c["n_out"]
    off = d["H"] == 0
    nan = float("nan")
    junk = {"yo": torch.where(off, torch.full_like(d["yo"], nan), d["yo"]),
            "R": torch.where(off, torch.full_like(d["R"], nan), d["R"])}
    for k in ("xb", "xa"):
        x = d[k].clone()
        if n_out:
            x[:, :4][off[:, :4]] = nan
            for i in range(5):
                unseen = off[:, 4 + n_out * i:4 + n_out * (i + 1)].all(1, keepdim=True)
                blk = x[:, 4 + 13 * i:17 + 13 * i]
                blk[unseen.expand_as(blk)] = -7e37 if i % 2 else nan
        else:
            x[off] = nan
        assert int((x != d[k]).sum()) > x.numel() // 4
        junk[k] = x
    assert int(torch.isnan(junk["yo"]).sum()) > off.numel() // 2
    out = _run(ctx, d)
    out_j = _run(ctx, d, **junk)
    assert torch.isfinite(out_j).all()
    check_bitwise(f"{_id(key)} junk at every unobserved entry", out_j, out)


@pytest.mark.parametrize("key", [("33x47", "r40", 1, 1.0), ("1x300", "id", 3, 1.0)], ids=_id)
def test_obs_stats_non_finite_values_stay_in_their_row(ctx, key):
    c = _case(key)
    d = c["dev"]
    out = _run(ctx, d)
    yo, R, xb = d["yo"].clone(), d["R"].clone(), d["xb"].clone()
    hit = torch.zeros(out.shape[:2], dtype=torch.bool, device=out.device)
    yo[0, 2, 0, 5] = float("nan")
    R[0, 7, 0, 3] = 0.0
    yo[-1, 9, 0, 1] = float("inf")
    for t, ch in ((0, 2), (0, 7), (-1, 9)):
        hit[t, ch] = True
    if c["n_out"] == 0:  # a state channel is read by its own row alone
        xb[0, 11, 0, 2] = float("inf")
        hit[0, 11] = True
    bad = _run(ctx, d, yo=yo, R=R, xb=xb)
    check_bitwise(f"{_id(key)} rows without a non-finite entry", bad[~hit], out[~hit])
    assert torch.isnan(bad[0, 2, Rf.OB]) and torch.isinf(bad[0, 7, Rf.JB]) and not torch.isfinite(bad[-1, 9, Rf.OB2])
    assert not torch.isfinite(bad[hit]).all(1).any()
    check_bitwise(f"{_id(key)} count and h of the hit rows", bad[hit][:, :2], out[hit][:, :2])


@pytest.mark.parametrize("with_xa", [True, False])
def test_obs_stats_profiled_as_misfit(ctx, with_xa):
    d = _case(("33x47", "r40", 3, 0.02))["dev"]
    ctx.profile_start()
    _run(ctx, d, **({} if with_xa else {"xa": None}))
    prof = ctx.profile_stop()
    assert prof["misfit"]["launches"] == 1 and prof["misfit"]["ms"] > 0
    assert sum(v["launches"] for v in prof.values()) == 1
    assert prof["misfit"]["bytes"] == 4.0 * 33 * 47 * 3 * (3 * 204 + (2 if with_xa else 1) * 69)


def test_obs_stats_python_checks(ctx):
    from vaevar.engine import obs_stats

    d = _case(("33x47", "r40", 1, 0.02))["dev"]
    xb, xa, yo, H, R, P = (d[k] for k in ("xb", "xa", "yo", "H", "R", "interp"))
    with pytest.raises(ValueError, match="operator expects"):
        obs_stats(ctx, xb[:, :68].contiguous(), None, yo, H, R, P)
    with pytest.raises(ValueError, match="yo must be"):
        obs_stats(ctx, xb, xa, yo, H, R, None)
    with pytest.raises(ValueError, match="H must be"):
        obs_stats(ctx, xb, xa, yo, H[:, :-1].contiguous(), R, P)
    with pytest.raises(ValueError, match="R must be"):
        obs_stats(ctx, xb, xa, yo, H, R[..., :-1].contiguous(), P)
    with pytest.raises(ValueError, match="xa_win"):
        obs_stats(ctx, xb, xa[:, :, :-1].contiguous(), yo, H, R, P)
    with pytest.raises(ValueError, match="float32"):
        obs_stats(ctx, xb.double(), xa, yo, H, R, P)
    with pytest.raises(ValueError, match="float32"):
        obs_stats(ctx, xb[0], xa, yo, H, R, P)
    with pytest.raises(ValueError, match="contiguous"):
        obs_stats(ctx, xb, xa, yo.transpose(2, 3).contiguous().transpose(2, 3), H, R, P)
    with pytest.raises(ValueError, match="device"):
        obs_stats(ctx, xb, xa, yo.cpu(), H, R, P)
    with pytest.raises(ValueError, match="out must be"):
        obs_stats(ctx, xb, xa, yo, H, R, P, out=torch.empty(1, 204, 9, device="cuda", dtype=torch.float64))
    buf = torch.empty(1, 204, 10, device="cuda", dtype=torch.float64)
    assert obs_stats(ctx, xb, xa, yo, H, R, P, out=buf) is buf
    check_bitwise("obs_stats into a caller's buffer", buf, obs_stats(ctx, xb, xa, yo, H, R, P))
