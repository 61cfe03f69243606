"""CPU: vv_obs_stats (O-B / O-A departure moments, include/vaevar.h) validates its arguments before any device work:
every rejected call returns VV_E_ARG (1001) and leaves a message, and none reaches the context (a dummy non-null handle
stands in for it). Also calib.DepartureStats on a hand-made table, and the Desroziers relations on the numpy
restatement the GPU tests compare against (tests/_obs_stats_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import _obs_stats_ref as Rf


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_obs_stats_exported_and_versioned():
    from vaevar import _lib, fields

    assert "vv_obs_stats" in _lib.EXPORTED and hasattr(_lib.lib, "vv_obs_stats")
    assert _lib.lib.vv_version() >= 113
    assert fields.OSTAT_N == Rf.NSTAT == 10
    for i, name in enumerate(Rf.NAMES):
        assert getattr(fields, "OSTAT_" + name.upper()) == i == getattr(Rf, name.upper())
    from vaevar import engine

    assert engine.obs_stats is fields.obs_stats


BAD = {"null_ctx": dict(ctx=None), "null_xb": dict(xb=None), "null_yo": dict(yo=None), "null_H": dict(H=None),
       "null_R": dict(R=None), "null_out": dict(out=None), "T_0": dict(T=0), "C_0": dict(C=0, interp=None),
       "Hs_0": dict(Hs=0), "Ws_0": dict(Ws=0), "C_68_n_in_13": dict(C=68), "n_in_0": dict(n_in=0, C=4),
       "n_in_17": dict(n_in=17, C=4 + 5 * 17), "n_out_0": dict(n_out=0), "n_out_65": dict(n_out=65),
       "HW_2^31-4096": dict(Hs=1, Ws=2 ** 31 - 4096), "HW_2^31": dict(Hs=32768, Ws=65536),
       "workgroups_2^31": dict(T=100, C=100, interp=None, Hs=30000, Ws=30000)}


@pytest.mark.parametrize("case", list(BAD))
def test_obs_stats_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep = ctypes.create_string_buffer(1 << 12)  # never dereferenced
    b = ctypes.cast(keep, ctypes.c_void_p)
    a = dict(ctx=b, xb=b, xa=b, yo=b, H=b, R=b, interp=b, n_out=40, n_in=13, T=1, C=69, Hs=8, Ws=8, out=b)
    a.update(BAD[case])
    if case == "workgroups_2^31":
        assert 100 * 100 * ((30000 * 30000 + 4095) // 4096) >= 2 ** 31 and 30000 * 30000 < 2 ** 31 - 4096
    # clear the thread's last error with a call that fails differently, so the message below is this call's
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    rc = lib.vv_obs_stats(a["ctx"], a["xb"], a["xa"], a["yo"], a["H"], a["R"], a["interp"], a["n_out"], a["n_in"],
                          a["T"], a["C"], a["Hs"], a["Ws"], a["out"], None)
    assert rc == 1001
    after = _msg(lib)
    assert after and after != before


def test_departure_summary_on_a_hand_made_table():
    from vaevar.calib import DepartureStats, departure_summary

    # one time level, three channels: d_b = (1, 3), d_a = (0.5, -0.5) at r = 2, h = 1; an unobserved channel; a
    # channel without analysis rows
    tab = np.zeros((1, 3, 10))
    tab[0, 0] = [2, 2, 4, 0, 10, 0.5, -1.0, 4, 5, 0.25]
    tab[0, 2] = [4, 2, 2, np.nan, 8, np.nan, np.nan, 4, 6, np.nan]
    s = departure_summary(tab)
    assert set(s) == {"n", "mean_ob", "mean_oa", "std_ob", "std_oa", "rms_ob", "rms_oa", "r_prescribed",
                      "r_desroziers", "hbht_desroziers", "chi2_b", "chi2_a"}
    for v in s.values():
        assert v.shape == (1, 3)
    assert s["n"].tolist() == [[2, 0, 4]]
    exp0 = {"mean_ob": 2.0, "mean_oa": 0.0, "std_ob": 1.0, "std_oa": 0.5, "rms_ob": np.sqrt(5.0), "rms_oa": 0.5,
            "r_prescribed": 2.0, "r_desroziers": -0.5, "hbht_desroziers": 5.5, "chi2_b": 2.5, "chi2_a": 0.125}
    for k, v in exp0.items():
        assert s[k][0, 0] == pytest.approx(v, rel=1e-15, abs=1e-15), k
        assert np.isnan(s[k][0, 1]), k  # n == 0
    assert s["mean_ob"][0, 2] == 0.5 and s["chi2_b"][0, 2] == 1.5 and s["r_prescribed"][0, 2] == 1.0
    for k in ("mean_oa", "std_oa", "rms_oa", "r_desroziers", "hbht_desroziers", "chi2_a"):
        assert np.isnan(s[k][0, 2]), k
    # centred: E[d_a d_b] - E[d_a] E[d_b]
    tab2 = tab.copy()
    tab2[0, 0, Rf.OA] = 1.0
    c = departure_summary(tab2, centred=True)
    assert c["r_desroziers"][0, 0] == pytest.approx(-0.5 - 0.5 * 2.0)
    assert departure_summary(tab2)["r_desroziers"][0, 0] == pytest.approx(-0.5)

    d = DepartureStats()
    with pytest.raises(ValueError):
        d.summary()
    d.add(tab)
    d.add(torch.from_numpy(tab))
    assert d.cycles == 2 and np.array_equal(d.table.numpy(), 2 * tab, equal_nan=True)
    s2 = d.summary()
    assert s2["n"].tolist() == [[4, 0, 8]] and s2["mean_ob"][0, 0] == 2.0  # the means of two equal cycles
    with pytest.raises(ValueError):
        d.add(np.zeros((1, 3, 9)))
    with pytest.raises(ValueError):
        d.add(np.zeros((2, 3, 10)))


def test_departure_stats_save_load_and_obs_std(tmp_path):
    from vaevar.calib import DepartureStats

    tab = np.zeros((2, 2, 10))
    tab[0, 0, [Rf.COUNT, Rf.OAOB]] = [4, 1.0]   # r_desroziers 0.25 -> sigma 0.5
    tab[0, 1, [Rf.COUNT, Rf.OAOB]] = [4, -1.0]  # negative estimate -> 0
    tab[1] = np.nan
    d = DepartureStats()
    d.add(tab)
    sug = d.suggested_obs_std(np.array([2.0, 1.0]))
    assert sug.tolist() == [0.25, 0.0]
    with pytest.raises(ValueError):
        d.suggested_obs_std(np.ones(3))
    p = str(tmp_path / "dep.npz")
    d.save(p)
    e = DepartureStats.load(p)
    assert e.cycles == 1 and np.array_equal(e.table.numpy(), tab, equal_nan=True)


def test_desroziers_relations_on_the_restatement():
    """Per-cell optimal scalar analysis x_a = x_b + K (yo - x_b), K = s_b^2 / (s_b^2 + s_o^2), s_b = 1, s_o = 0.5 on
    N = 67 * 131 cells: each estimator is a scaled chi-square mean with relative standard deviation sqrt(2 / N), so the
    three ratios lie within 6 sqrt(2 / N) = 0.0906 of 1 (numpy over 200 seeds: the worst was 0.043)."""
    from vaevar.calib import departure_summary

    Hs, Ws, sb, so = 67, 131, 1.0, 0.5
    N = Hs * Ws
    rng = np.random.default_rng(20251021)
    truth = rng.standard_normal((1, 1, Hs, Ws))
    xb = (truth + sb * rng.standard_normal(truth.shape)).astype(np.float32)
    yo = (truth + so * rng.standard_normal(truth.shape)).astype(np.float32)
    K = sb ** 2 / (sb ** 2 + so ** 2)
    xa = (xb + np.float32(K) * (yo - xb)).astype(np.float32)
    Hm = np.ones_like(xb)
    Rm = np.full_like(xb, so ** 2)
    tab, mag = Rf.table_ref(xb, xa, yo, Hm, Rm)
    assert tab[0, 0, Rf.COUNT] == N and tab[0, 0, Rf.H] == N
    # the long-double sums against math.fsum on the same terms
    import math

    terms = Rf.terms_ref(xb, xa, yo, Hm, Rm)
    for i in (Rf.OB, Rf.OB2, Rf.OAOB, Rf.JA):
        assert tab[0, 0, i] == math.fsum(terms[i].ravel().tolist()), Rf.NAMES[i]
    s = departure_summary(tab)
    bound = 6 * np.sqrt(2.0 / N)
    assert bound == pytest.approx(0.0906, abs=5e-5)
    for name, v in (("r", s["r_desroziers"][0, 0] / so ** 2), ("hbht", s["hbht_desroziers"][0, 0] / sb ** 2),
                    ("ob2", s["rms_ob"][0, 0] ** 2 / (sb ** 2 + so ** 2))):
        print(f"desroziers {name}: ratio {v:.4f}, |ratio - 1| {abs(v - 1):.4f} (bound {bound:.4f})")
        assert abs(v - 1) < bound, (name, v)
    assert s["chi2_a"][0, 0] < 1 < s["chi2_b"][0, 0]  # 2 J_o(xa) / N < 1


def test_restatement_ignores_junk_at_unobserved_entries():
    c = Rf.make_case(5, 7, T=2, n_out=0, seed=7001, density=0.3, zero_slice=1)
    assert set(np.unique(c["H"].numpy())) == {0.0, 0.5, 1.0} and not c["H"][1].any()
    a, _ = Rf.table_ref(c["xb"], c["xa"], c["yo"], c["H"], c["R"])
    junk = {k: torch.where(c["H"] == 0, torch.tensor(float("nan")), c[k]) for k in ("xb", "xa", "yo", "R")}
    b, _ = Rf.table_ref(junk["xb"], junk["xa"], junk["yo"], c["H"], junk["R"])
    assert np.array_equal(a, b) and not np.isnan(a).any()
    assert (a[1] == 0).all() and a[0, :, Rf.COUNT].sum() == (c["H"][0] != 0).sum()
    n, _ = Rf.table_ref(c["xb"], None, c["yo"], c["H"], c["R"])
    assert np.isnan(n[:, :, list(Rf.ANALYSIS_ROWS)]).all()
    keep = [i for i in range(10) if i not in Rf.ANALYSIS_ROWS]
    assert np.array_equal(n[:, :, keep], a[:, :, keep])
    # d_a and d_b are correlated and non-trivial; R varies per (t, c)
    d = c["yo"] - c["xb"]
    assert float(np.corrcoef(d.ravel(), (c["yo"] - c["xa"]).ravel())[0, 1]) > 0.3
    assert len(np.unique(c["R"][:, :, 0, 0].numpy())) >= 0.9 * c["R"].shape[0] * c["R"].shape[1]
    assert (c["R"] > 0).all()
