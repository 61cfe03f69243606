"""CPU: vv_obs_error (the held-out observation verification of --use_eval) validates its arguments before any device
work. Every rejected call returns VV_E_ARG (1001) and leaves a message in vv_last_error; none of them reaches the
context (a dummy non-null handle stands in for it), so no GPU is needed."""
import ctypes

import pytest


def _call(lib, ctx, x, yo, H, mask, interp, n_out, n_in, C, Hs, Ws, err):
    return lib.vv_obs_error(ctx, x, yo, H, mask, interp, n_out, n_in, C, Hs, Ws, err, None, None)


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_obs_error_exported_and_versioned():
    from vaevar import _lib

    assert "vv_obs_error" in _lib.EXPORTED and hasattr(_lib.lib, "vv_obs_error")
    assert _lib.lib.vv_version() >= 101


def test_obs_error_null_context():
    from vaevar import _lib

    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    assert _call(_lib.lib, None, buf, buf, buf, buf, buf, 40, 13, 69, 8, 8, buf) == 1001
    assert _msg(_lib.lib)


@pytest.mark.parametrize("case", ["null_x", "null_yo", "null_H", "null_mask", "null_err", "n_out_65", "n_out_0",
                                  "n_in_17", "n_in_0", "C_68_n_in_13", "Hs_0", "Ws_0", "identity_C_0"])
def test_obs_error_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep = ctypes.create_string_buffer(1 << 16)  # never dereferenced: every case fails before the context is used
    b = ctypes.cast(keep, ctypes.c_void_p)
    a = dict(ctx=b, x=b, yo=b, H=b, mask=b, interp=b, n_out=40, n_in=13, C=69, Hs=8, Ws=8, err=b)
    a.update({"null_x": dict(x=None), "null_yo": dict(yo=None), "null_H": dict(H=None), "null_mask": dict(mask=None),
              "null_err": dict(err=None), "n_out_65": dict(n_out=65), "n_out_0": dict(n_out=0),
              "n_in_17": dict(n_in=17, C=4 + 5 * 17), "n_in_0": dict(n_in=0, C=4), "C_68_n_in_13": dict(C=68),
              "Hs_0": dict(Hs=0), "Ws_0": dict(Ws=0), "identity_C_0": dict(interp=None, C=0)}[case])
    # clear the thread's last error with a call that fails differently, so the message below is this call's
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    assert _call(lib, **a) == 1001
    after = _msg(lib)
    assert after and after != before
