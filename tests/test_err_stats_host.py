"""CPU: the ABI of vv_err_accum / vv_err_finalize / vv_r_fill (exports, version, the argument checks that are decided
before any device work) and the host halves of the model-error feature, problem.init_q_matrix and
problem.static_r_table, against the torch-on-CPU restatements of tests/_err_stats_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

from _err_stats_ref import init_q_matrix_ref, static_r_ref, sum_bound


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_exported_and_versioned():
    from vaevar import _lib

    for name in ("vv_err_accum", "vv_err_finalize", "vv_r_fill"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert _lib.lib.vv_version() >= 111


# ---------------------------------------------------------------------------------------------------------------
# VV_E_ARG before any device work: the pointers below are host buffers that are never dereferenced
# ---------------------------------------------------------------------------------------------------------------
def _bufs(k):
    keep = [ctypes.create_string_buffer(1 << 12) for _ in range(k)]
    return keep, [ctypes.cast(b, ctypes.c_void_p) for b in keep]


def _rejected(lib, call):
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001  # another message first, so the one below is this call's
    before = _msg(lib)
    assert call() == 1001
    after = _msg(lib)
    assert after and after != before


BAD_ACCUM = {"null_ctx": dict(ctx=None), "null_pred": dict(pred=None), "null_tgt": dict(tgt=None),
             "no_output": dict(cell=None, chan=None), "B_0": dict(B=0), "C_0": dict(C=0), "H_0": dict(H=0),
             "W_negative": dict(W=-3), "pred_stride_short": dict(ps=2 * 3 * 4 - 1),
             "tgt_stride_short": dict(ts=0), "sample_2^31": dict(C=2, H=32768, W=32768, ps=2 ** 40, ts=2 ** 40)}


@pytest.mark.parametrize("case", list(BAD_ACCUM))
def test_err_accum_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, pred, tgt, cell, chan) = _bufs(5)
    a = dict(ctx=ctx, pred=pred, ps=24, tgt=tgt, ts=24, B=2, C=2, H=3, W=4, cell=cell, chan=chan)
    a.update(BAD_ACCUM[case])
    _rejected(lib, lambda: lib.vv_err_accum(a["ctx"], a["pred"], a["ps"], a["tgt"], a["ts"], a["B"], a["C"], a["H"],
                                            a["W"], a["cell"], a["chan"], None))


BAD_FINAL = {"null_ctx": dict(ctx=None), "null_cell": dict(cell=None), "no_output": dict(qf=None, qt=None),
             "n_0": dict(n=0), "n_negative": dict(n=-5), "C_0": dict(C=0), "H_0": dict(H=0), "W_0": dict(W=0),
             "field_2^31": dict(C=2, H=32768, W=32768)}


@pytest.mark.parametrize("case", list(BAD_FINAL))
def test_err_finalize_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, cell, qf, qt) = _bufs(4)
    a = dict(ctx=ctx, cell=cell, n=3, C=2, H=3, W=4, qf=qf, qt=qt)
    a.update(BAD_FINAL[case])
    _rejected(lib, lambda: lib.vv_err_finalize(a["ctx"], a["cell"], a["n"], a["C"], a["H"], a["W"], a["qf"], a["qt"],
                                               None))


BAD_FILL = {"null_ctx": dict(ctx=None), "null_rtab": dict(rtab=None), "null_R": dict(R=None), "T_0": dict(T=0),
            "C_0": dict(C=0), "Hs_0": dict(Hs=0), "Ws_0": dict(Ws=0), "n_in_0": dict(op=True, n_in=0, C=4),
            "n_in_17": dict(op=True, n_in=17, C=4 + 5 * 17), "n_out_0": dict(op=True, n_out=0),
            "n_out_65": dict(op=True, n_out=65), "C_not_4_plus_5_n_in": dict(op=True, C=68)}


@pytest.mark.parametrize("case", list(BAD_FILL))
def test_r_fill_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep, (ctx, rtab, interp, R) = _bufs(4)
    a = dict(ctx=ctx, rtab=rtab, op=False, n_out=40, n_in=13, T=1, C=69, Hs=2, Ws=2, R=R)
    a.update(BAD_FILL[case])
    _rejected(lib, lambda: lib.vv_r_fill(a["ctx"], a["rtab"], interp if a["op"] else None, a["n_out"], a["n_in"],
                                         a["T"], a["C"], a["Hs"], a["Ws"], a["R"], None))


# ---------------------------------------------------------------------------------------------------------------
# init_q_matrix
# ---------------------------------------------------------------------------------------------------------------
NCH, NLAT, NLON = 5, 9, 14


@pytest.fixture(scope="module")
def coeff_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("coeff")
    rng = np.random.default_rng(41)
    for i in range(1, 4):  # calculate_q's output: float64, non-negative
        np.save(d / ("q%d.npy" % i), rng.random((NCH, NLAT, NLON)) ** 2 * 10.0 ** rng.integers(-6, 3, (NCH, 1, 1)))
    np.save(d / "new_q.npy", rng.random((6, NCH)))
    return str(d)


@pytest.mark.parametrize("q_type", [0, -1, 1])
@pytest.mark.parametrize("da_win", [2, 4])
def test_init_q_matrix_is_the_reference_table(coeff_dir, q_type, da_win):
    """Every (slot, channel) entry against the reference's broadcast tensor, read at two cells. q_type 0 sums H W
    non-negative fp64 terms: any two summation orders agree within 2 H W 2^-53 relative; the other types move values
    without arithmetic and must agree exactly."""
    from vaevar.problem import init_q_matrix

    tab = init_q_matrix(coeff_dir, q_type, da_win, NCH)
    ref = init_q_matrix_ref(coeff_dir, q_type, da_win, NCH, NLAT, NLON)
    assert tab.dtype == np.float64 and tab.shape == (da_win - 1, NCH)
    assert tuple(ref.shape) == (da_win - 1, NCH, NLAT, NLON)
    for cell in ((0, 0), (NLAT - 1, NLON - 2)):
        r = ref[:, :, cell[0], cell[1]].double().numpy()
        if q_type == 0:
            rel = np.abs(tab - r) / r
            print("q_type 0 relative difference", rel.max(), "bound", sum_bound(NLAT * NLON))
            assert (r > 0).all() and rel.max() <= sum_bound(NLAT * NLON)
        else:
            assert np.array_equal(tab, r)


def test_init_q_matrix_edges(coeff_dir):
    from vaevar.problem import init_q_matrix

    with pytest.raises(NotImplementedError, match="not implemented q type"):
        init_q_matrix(coeff_dir, 2, 3, NCH)
    with pytest.raises(NotImplementedError, match="not implemented q type"):
        init_q_matrix_ref(coeff_dir, 2, 3, NCH, NLAT, NLON)
    for q_type in (0, -1, 1, 2):  # da_win 1 returns before q_type is looked at (:529-530)
        e = init_q_matrix(coeff_dir, q_type, 1, NCH)
        assert e.shape == (0, NCH) and e.dtype == np.float64
        assert init_q_matrix_ref(coeff_dir, q_type, 1, NCH, NLAT, NLON) == []
    with pytest.raises(FileNotFoundError):
        init_q_matrix(coeff_dir, 0, 5, NCH)  # q4.npy does not exist
    with pytest.raises(ValueError, match="q1.npy"):
        init_q_matrix(coeff_dir, 0, 2, NCH + 1)


# ---------------------------------------------------------------------------------------------------------------
# static_r_table
# ---------------------------------------------------------------------------------------------------------------
def _r_inputs(T, C, seed=7):
    rng = np.random.default_rng(seed)
    obs_var = (rng.random(C) * 10.0 ** rng.integers(-8, 5, C)).astype(np.float32)
    q = rng.random((T - 1, C)) * obs_var.astype(np.float64) * 3.0  # float64, the size of obs_var
    return obs_var, q


@pytest.mark.parametrize("qdtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", [1, 4])
def test_static_r_table_is_the_reference_assignment(T, qdtype):
    from vaevar.problem import static_r_table

    C = 20
    obs_var, q = _r_inputs(T, C)
    q = q.astype(qdtype)
    qm = [torch.broadcast_to(torch.from_numpy(q[i]).reshape(C, 1, 1), (C, 2, 3)) for i in range(T - 1)]
    ref = static_r_ref(torch.from_numpy(obs_var).reshape(C, 1, 1), qm, T, 2, 3).numpy()
    tab = static_r_table(obs_var, q if T > 1 else None, T)
    assert tab.dtype == np.float32 and tab.shape == (T, C) and ref.dtype == np.float32
    assert np.array_equal(np.broadcast_to(tab[:, :, None, None], ref.shape).view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(static_r_table(obs_var, None, T), np.broadcast_to(obs_var, (T, C)))  # q_type -1


def test_static_r_table_rounds_once_where_r_table_rounds_twice():
    """With a float64 q the reference adds in fp64 and rounds once; r_table rounds q to fp32 first. On this seed's 60
    values the two differ in at least one fp32 word (a double rounding): the reason static_r_table exists. With a
    float32 q the two are the same function."""
    from vaevar.problem import r_table, static_r_table

    obs_var, q = _r_inputs(4, 20)
    a, b = static_r_table(obs_var, q, 4), r_table(obs_var, q, 4)
    n = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    print("words that differ", n, "of", a.size - 20)
    assert n >= 1 and np.array_equal(a[0], b[0])
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)  # of fp32: one ulp, no more
    assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulp).all()
    q32 = q.astype(np.float32)
    assert np.array_equal(static_r_table(obs_var, q32, 4).view(np.uint32), r_table(obs_var, q32, 4).view(np.uint32))
    with pytest.raises(ValueError, match="rows"):
        static_r_table(obs_var, q[:2], 4)
