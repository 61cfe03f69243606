"""CPU: the generator of vv_obs_synth as restated in tests/_obs_synth_ref.py (Philox4x32-10 known answers, the
statistics of the mask and noise streams), the host helpers problem.free_amount / problem.r_table / cycle.FreeObs, and
the argument checks of vv_obs_synth, vv_select_smallest and vv_normal_fill, which are decided before any device work."""
import ctypes
import datetime as dt
import math

import numpy as np
import pytest

from _obs_synth_ref import eps_ref, key32, mask_ref, philox4x32_10, select_ref

SEED = 20250620


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_exported_and_versioned():
    from vaevar import _lib

    for name in ("vv_obs_synth", "vv_select_smallest", "vv_normal_fill"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert _lib.lib.vv_version() >= 110


@pytest.mark.parametrize("ctr, key, out", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))])
def test_philox_known_answers(ctr, key, out):
    got = philox4x32_10(*ctr, *key)
    assert tuple(int(w[0]) for w in got) == out


def test_philox_vectorised_equals_scalar():
    c0 = np.array([0, 1, 0xFFFFFFFF, 12345], np.uint64)
    v = philox4x32_10(c0, 7, 1, 9, 0x01234567, 0x89ABCDEF)
    for i, x in enumerate(c0):
        s = philox4x32_10(int(x), 7, 1, 9, 0x01234567, 0x89ABCDEF)
        assert [int(w[i]) for w in v] == [int(w[0]) for w in s]


def test_select_ref_breaks_ties_by_position():
    keys = np.array([5, 3, 5, 3, 9, 3, 5], np.uint32)
    m, ties = select_ref(keys, 4)
    assert m.tolist() == [1, 1, 0, 1, 0, 1, 0] and ties == 3  # the three 3s, then the first 5
    assert select_ref(keys, 0)[0].sum() == 0 and select_ref(keys, 0)[1] == 0
    assert select_ref(keys, 7)[0].sum() == 7 and select_ref(keys, 7)[1] == 1
    m, ties = select_ref(np.full(10, 0xFFFFFFFF, np.uint32), 3)
    assert m.tolist() == [1, 1, 1] + [0] * 7 and ties == 10


def test_free_amount():
    from vaevar.problem import free_amount

    assert free_amount("free_0015") == 15000
    assert free_amount("free_00150") == 15000
    assert free_amount("free_1038") == 1038000
    for bad in ("real_simu", "prepbufr", "", "fre_0015"):
        with pytest.raises(ValueError, match="free"):
            free_amount(bad)


def test_free_obs_refuses_more_cells_than_the_grid():
    from vaevar.cycle import FreeObs
    from vaevar.problem import r_table

    truth = lambda t: np.zeros((2, 721, 1440), np.float32)  # noqa: E731
    obs = FreeObs(None, truth, "free_1039", r_table(np.ones(2)))
    assert obs.amount == 1039000 > 721 * 1440
    with pytest.raises(ValueError, match="free_1039"):
        obs.get_obs_info(dt.datetime(2020, 1, 1))
    assert FreeObs(None, truth, "free_1038", r_table(np.ones(2))).amount == 1038000  # fits: 1038240 cells
    with pytest.raises(ValueError, match="obs_var"):
        FreeObs(None, truth, "free_0015", r_table(np.ones(2)), noise=True)
    # the draw number: whole hours since 1970-01-01, modulo 2^32
    assert FreeObs.draw_number(dt.datetime(1970, 1, 1, 5, 59)) == 5
    assert FreeObs.draw_number(dt.datetime(2020, 1, 1)) == 438288
    assert FreeObs.draw_number(dt.datetime(1969, 12, 31, 23)) == 2 ** 32 - 1


@pytest.mark.parametrize("T", [1, 3])
def test_r_table_is_the_reference_expression(T):
    import torch
    from vaevar.problem import r_table

    rng = np.random.default_rng(3)
    C, nlat, nlon = 5, 3, 4
    obs_var = torch.from_numpy(rng.random((C, 1, 1)).astype(np.float32) * 1e4)  # data_reader.obs_var's shape
    q = [torch.from_numpy(rng.random((C, 1, 1)).astype(np.float32) * 1e-3) for _ in range(T - 1)]
    R = torch.zeros(T, C, nlat, nlon)  # da_4dvar.py:630-634
    R[0] = obs_var
    for i in range(T - 1):
        R[i + 1] = obs_var + q[i]
    tab = r_table(obs_var.numpy(), None if T == 1 else np.stack([x.numpy().reshape(-1) for x in q]), T)
    assert tab.dtype == np.float32 and tab.shape == (T, C)
    ref = R.numpy()
    assert np.array_equal(np.broadcast_to(tab[:, :, None, None], ref.shape).view(np.uint32), ref.view(np.uint32))
    zero = r_table(obs_var.numpy(), None, T)  # q_type -1
    assert all(np.array_equal(zero[t], obs_var.numpy().reshape(-1)) for t in range(T))


def test_mask_stream_statistics():
    """256 draws of 500 of the 33 x 47 cells: every draw has exactly 500 distinct cells; the per-cell counts are
    those of a uniform subset (chi-square z-score; a cell's count is Binomial-like with the finite-population variance
    E (1 - 500 / 1551)); two draws overlap as two independent subsets do (hypergeometric mean 500^2 / 1551 = 161)."""
    hs, ws, k, draws = 33, 47, 500, 256
    hw = hs * ws
    masks = np.stack([mask_ref(SEED, d, hs, ws, k)[0].reshape(-1) for d in range(draws)])
    assert (masks.sum(1) == k).all() and set(np.unique(masks)) == {0.0, 1.0}
    counts = masks.sum(0)
    e = draws * k / hw
    chi2 = ((counts - e) ** 2).sum() / (e * (1 - k / hw))
    z = (chi2 - (hw - 1)) / math.sqrt(2 * (hw - 1))
    print("chi-square z", z)
    assert abs(z) < 4
    overlap = int((masks[0] * masks[1]).sum())
    print("overlap", overlap)
    assert abs(overlap - 161) < 4 * math.sqrt(161)
    assert not np.array_equal(mask_ref(SEED, 0, hs, ws, k)[0], mask_ref(SEED + 1, 0, hs, ws, k)[0])
    kk = key32(SEED, 0, hw)
    assert kk.dtype == np.uint32 and len(np.unique(kk)) > hw - 3


def test_noise_stream_statistics():
    """eps over 2 x 69 x 33 x 47 elements is standard normal: Kolmogorov-Smirnov against N(0, 1), mean, lag-1
    correlation; the bounds are conditions a correct generator meets, not tolerances."""
    n = 2 * 69 * 33 * 47
    x = eps_ref(SEED, 0, 0, n)
    assert np.isfinite(x).all() and np.abs(x).max() <= 5.78
    xs = np.sort(x)
    cdf = 0.5 * (1.0 + np.vectorize(math.erf)(xs / math.sqrt(2.0)))
    i = np.arange(1, n + 1)
    d = max((i / n - cdf).max(), (cdf - (i - 1) / n).max())
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * d  # the asymptotic Kolmogorov distribution
    p = 2.0 * sum((-1) ** (j - 1) * math.exp(-2.0 * j * j * lam * lam) for j in range(1, 101))
    zm = abs(x.mean()) * math.sqrt(n)
    xc = x - x.mean()
    zl = abs((xc[1:] * xc[:-1]).sum() / (xc * xc).sum()) * math.sqrt(n)
    print("KS p", p, "mean z", zm, "lag-1 z", zl, "std", x.std())
    assert p > 0.01
    assert zm < 4 and zl < 4
    assert abs(x.std() - 1.0) < 4 / math.sqrt(2 * n)
    # eps(e) depends on (seed, draw, e) alone: a window taken elsewhere is the same numbers
    assert np.array_equal(eps_ref(SEED, 0, 1001, 77), x[1001:1078])
    assert not np.array_equal(eps_ref(SEED, 1, 0, 64), x[:64]) and not np.array_equal(eps_ref(SEED + 1, 0, 0, 64), x[:64])


# ---------------------------------------------------------------------------------------------------------------
# VV_E_ARG before any device work: the pointers below are host buffers that are never dereferenced
# ---------------------------------------------------------------------------------------------------------------
def _bufs(k):
    keep = [ctypes.create_string_buffer(1 << 12) for _ in range(k)]
    return keep, [ctypes.cast(b, ctypes.c_void_p) for b in keep]


def _off(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


BAD_SYNTH = {
    "null_ctx": dict(ctx=None), "null_gt": dict(gt=None), "null_yo": dict(yo=None), "null_H": dict(H=None),
    "T_0": dict(T=0), "C_0": dict(C=0), "Hs_0": dict(Hs=0), "Ws_0": dict(Ws=0), "T_negative": dict(T=-1),
    "elements_2^31": dict(T=6, C=69, Hs=2048, Ws=4096), "elements_exactly_2^31": dict(T=1, C=2, Hs=32768, Ws=32768),
    "n_obs_negative": dict(n_obs=-1), "n_obs_above_cells": dict(n_obs=17),
    "R_without_rtab": dict(rtab=None), "rtab_without_R": dict(R=None),
    "H_is_gt": dict(alias=("H", "gt", 0)), "H_is_yo": dict(alias=("H", "yo", 0)), "H_is_R": dict(alias=("H", "R", 0)),
    "R_is_gt": dict(alias=("R", "gt", 0)), "R_is_yo": dict(alias=("R", "yo", 0)),
    "H_overlaps_gt_tail": dict(alias=("H", "gt", 124)), "R_overlaps_H_tail": dict(alias=("R", "H", 64)),
    "yo_overlaps_gt_partly": dict(alias=("yo", "gt", 16)),
}


@pytest.mark.parametrize("case", list(BAD_SYNTH))
def test_obs_synth_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, gt, yo, H, R, sd, rtab) = _bufs(7)
    a = dict(ctx=ctx, gt=gt, T=1, C=2, Hs=4, Ws=4, n_obs=5, sd=sd, rtab=rtab, yo=yo, H=H, R=R)  # 32 floats a field
    over = dict(BAD_SYNTH[case])
    alias = over.pop("alias", None)
    a.update(over)
    if alias:
        a[alias[0]] = _off(a[alias[1]], alias[2])
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001  # another message first, so the one below is this call's
    before = _msg(lib)
    rc = lib.vv_obs_synth(a["ctx"], a["gt"], a["T"], a["C"], a["Hs"], a["Ws"], a["n_obs"], 1, 2, 3, a["sd"],
                          a["rtab"], a["yo"], a["H"], a["R"], None, None)
    assert rc == 1001
    after = _msg(lib)
    assert after and after != before


BAD_SELECT = {"null_ctx": dict(ctx=None), "null_keys": dict(keys=None), "null_mask": dict(mask=None),
              "n_0": dict(n=0), "n_negative": dict(n=-4), "n_2^31": dict(n=2 ** 31), "k_negative": dict(k=-1),
              "k_above_n": dict(k=101)}


@pytest.mark.parametrize("case", list(BAD_SELECT))
def test_select_smallest_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, keys, mask) = _bufs(3)
    a = dict(ctx=ctx, keys=keys, n=100, k=10, mask=mask)
    a.update(BAD_SELECT[case])
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    assert lib.vv_select_smallest(a["ctx"], a["keys"], a["n"], a["k"], a["mask"], None, None) == 1001
    assert _msg(lib) and _msg(lib) != before


BAD_NORMAL = {"null_ctx": dict(ctx=None), "null_out": dict(out=None), "n_negative": dict(n=-1),
              "first_negative": dict(first=-1), "first_plus_n_overflows": dict(first=2 ** 63 - 5, n=10)}


@pytest.mark.parametrize("case", list(BAD_NORMAL))
def test_normal_fill_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, out) = _bufs(2)
    a = dict(ctx=ctx, out=out, n=8, first=0)
    a.update(BAD_NORMAL[case])
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    assert lib.vv_normal_fill(a["ctx"], a["out"], a["n"], a["first"], 1, 2, None) == 1001
    assert _msg(lib) and _msg(lib) != before
