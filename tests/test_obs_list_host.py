"""CPU: the observation-list entry points (vv_set_obs_list, vv_get_obs_list, vv_obs_list_eval) are exported, and
validate their arguments before any device work: every rejected call returns VV_E_ARG (1001) and leaves a message, and
none reaches the context (a dummy non-null handle stands in for it). Also the fp64 restatement the GPU tests compare
against (tests/_obs_list_ref.py) on a hand-made case."""
import ctypes

import numpy as np
import pytest

from _obs_list_ref import compact_ref, eval_ref, x_aug64


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_obs_list_exported_and_versioned():
    from vaevar import _lib

    for name in ("vv_set_obs_list", "vv_get_obs_list", "vv_obs_list_eval"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert _lib.lib.vv_version() >= 109


BAD = {"null_ctx": dict(ctx=None), "null_interp": dict(interp=None), "null_x": dict(x=None), "null_yo": dict(yo=None),
       "null_H": dict(H=None), "null_R": dict(R=None), "null_g": dict(g=None), "null_J": dict(J=None),
       "null_counts": dict(counts=None), "T_0": dict(T=0), "T_negative": dict(T=-1), "n_in_0": dict(n_in=0),
       "n_in_17": dict(n_in=17), "n_out_0": dict(n_out=0), "n_out_65": dict(n_out=65), "Hs_0": dict(Hs=0),
       "HW_2^31": dict(Hs=32768, Ws=65536), "6_T_HW_2^31": dict(Hs=16384, Ws=32768)}


@pytest.mark.parametrize("case", list(BAD))
def test_obs_list_eval_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep = ctypes.create_string_buffer(1 << 12)  # never dereferenced
    b = ctypes.cast(keep, ctypes.c_void_p)
    J, counts = (ctypes.c_double * 2)(), (ctypes.c_longlong * 4)()
    a = dict(ctx=b, interp=b, n_out=40, n_in=13, x=b, yo=b, H=b, R=b, T=2, Hs=8, Ws=8, g=b, J=J, counts=counts)
    a.update(BAD[case])
    # clear the thread's last error with a call that fails differently, so the message below is this call's
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    rc = lib.vv_obs_list_eval(a["ctx"], a["interp"], a["n_out"], a["n_in"], a["x"], a["yo"], a["H"], a["R"], a["T"],
                              a["Hs"], a["Ws"], 1.0, a["g"], a["J"], a["counts"], None)
    assert rc == 1001
    after = _msg(lib)
    assert after and after != before


def test_set_and_get_obs_list_reject_bad_arguments():
    from vaevar import _lib

    lib = _lib.lib
    keep = ctypes.create_string_buffer(1 << 12)
    b = ctypes.cast(keep, ctypes.c_void_p)
    info = (ctypes.c_longlong * 4)()
    for call in (lambda: lib.vv_set_obs_list(None, 0, 1), lambda: lib.vv_set_obs_list(b, 2, 1),
                 lambda: lib.vv_set_obs_list(b, -1, 0), lambda: lib.vv_get_obs_list(None, 0, info),
                 lambda: lib.vv_get_obs_list(b, 0, None), lambda: lib.vv_get_obs_list(b, 2, info)):
        assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
        before = _msg(lib)
        assert call() == 1001
        assert _msg(lib) and _msg(lib) != before


def test_restatement_on_a_hand_made_case():
    """One slot, a 2 x 3 grid, n_in = 2 state levels, n_out = 3 observation levels (C = 14, C_obs = 19): the units and
    records in the documented order, and J and the gradient worked out by hand."""
    P = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]], np.float32)
    x = np.arange(14 * 6, dtype=np.float32).reshape(1, 14, 2, 3) / 8
    xa = x_aug64(P, x)
    assert xa.shape == (1, 19, 2, 3)
    assert np.array_equal(xa[0, 4 + 3 * 2 + 1], 0.5 * (x[0, 4 + 2 * 2] + x[0, 4 + 2 * 2 + 1]))
    H = np.zeros((1, 19, 2, 3), np.float32)
    yo = xa.astype(np.float32).copy()
    R = np.full((1, 19, 2, 3), 2.0, np.float32)
    # pixel 4 (row 1, col 1): direct channels 3 and 1; pixel 0: level 2 then 0 of variable 3 (group 3), H = 0.5 at
    # level 0; pixel 5: level 1 of variable 1 (group 1)
    H[0, 3, 1, 1] = H[0, 1, 1, 1] = 1.0
    H[0, 4 + 3 * 2 + 2, 0, 0] = 1.0
    H[0, 4 + 3 * 2 + 0, 0, 0] = 0.5
    H[0, 4 + 3 * 0 + 1, 1, 2] = 1.0
    yo[0, 3, 1, 1] -= 1.0           # d = +1
    yo[0, 1, 1, 1] += 2.0           # d = -2
    yo[0, 4 + 6 + 2, 0, 0] -= 3.0   # d = +3
    yo[0, 4 + 6 + 0, 0, 0] += 4.0   # d = -4, h = 0.5
    yo[0, 4 + 1, 1, 2] -= 1.0       # d = +1
    L = compact_ref(yo, H, R, 3)
    assert L["uoff"].tolist() == [0, 1, 2, 2, 3, 3, 3]
    assert L["ugroup"].tolist() == [0, 1, 3] and L["upix"].tolist() == [4, 5, 0]
    assert L["urec"].tolist() == [0, 2, 3, 5] and L["o"].tolist() == [1, 3, 1, 0, 2]
    assert L["h"].tolist() == [1.0, 1.0, 1.0, 0.5, 1.0] and L["counts"].tolist() == [[3, 5]]
    E = eval_ref(L, P, x, coeff=2.0)
    # J = sum h d^2 / r = (4 + 1 + 1 + 0.5 * 16 + 9) / 2
    assert E["J"].tolist() == [11.5] and E["dmin"] == 1.0
    g = E["g"].reshape(14, 6)
    want = np.zeros((14, 6))
    want[1, 4], want[3, 4] = 2.0 * -2 / 2, 2.0 * 1 / 2
    want[4 + 0, 5] = want[4 + 1, 5] = 0.5 * (2.0 * 1 / 2)           # level 1 spreads evenly over both state levels
    want[4 + 2 * 2 + 0, 0] = 2.0 * 0.5 * -4 / 2                      # observation level 0 -> state level 0
    want[4 + 2 * 2 + 1, 0] = 2.0 * 3 / 2                             # observation level 2 -> state level 1
    assert np.array_equal(g, want)
    cells = E["cells"].reshape(14, 6)
    assert cells.sum() == 4 + 2 + 2 and cells[0:4, 4].all() and cells[4:6, 5].all() and cells[8:10, 0].all()
    assert np.array_equal(E["gabs"].reshape(14, 6), np.abs(want))
    # an empty slot: no units, J = 0
    L0 = compact_ref(np.zeros_like(yo), np.zeros_like(H), R, 3)
    assert L0["counts"].tolist() == [[0, 0]] and eval_ref(L0, P, x)["J"].tolist() == [0.0]
