"""CPU: vv_obs_qc (the departure filter of the obs_type real* family, da_4dvar.py:764-800) validates its arguments
before any device work: every rejected call returns VV_E_ARG (1001) and leaves a message, and none reaches the context
(a dummy non-null handle stands in for it). Also the host helpers qc_flags / qc_threshold, and the torch restatement
the GPU tests compare against (tests/_obs_qc_ref.py) on a hand-made case."""
import ctypes

import numpy as np
import pytest
import torch

from _obs_qc_ref import EXEMPT_Z, FILTER, FLAG_SETS, YO_SIMU, YO_SIMU_Z, gt_aug_ref, make_case, obs_qc_ref


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_obs_qc_exported_and_versioned():
    from vaevar import _lib

    assert "vv_obs_qc" in _lib.EXPORTED and hasattr(_lib.lib, "vv_obs_qc")
    assert _lib.lib.vv_version() >= 104


BAD = {"null_ctx": dict(ctx=None), "null_gt": dict(gt=None), "null_yo": dict(yo=None), "null_H": dict(H=None),
       "null_thr": dict(thr=None), "T_0": dict(T=0), "C_68_n_in_13": dict(C=68),
       "n_in_17": dict(n_in=17, C=4 + 5 * 17), "n_out_65": dict(n_out=65), "flags_16": dict(flags=16),
       "flags_negative": dict(flags=-1), "exempt_z_without_filter": dict(flags=EXEMPT_Z | YO_SIMU),
       "both_yo_simu": dict(flags=FILTER | YO_SIMU | YO_SIMU_Z),
       "exempt_z_identity": dict(interp=None, flags=FILTER | EXEMPT_Z),
       "yo_simu_z_identity": dict(interp=None, flags=FILTER | YO_SIMU_Z), "yo_is_H": dict(alias=True),
       "HW_2^31-4096": dict(Hs=1, Ws=2 ** 31 - 4096), "HW_2^31": dict(Hs=32768, Ws=65536)}


@pytest.mark.parametrize("case", list(BAD))
def test_obs_qc_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep = [ctypes.create_string_buffer(1 << 12) for _ in range(2)]  # never dereferenced
    b, b2 = (ctypes.cast(k, ctypes.c_void_p) for k in keep)
    a = dict(ctx=b, gt=b, yo=b, H=b2, interp=b, n_out=40, n_in=13, thr=b, flags=FILTER, T=1, C=69, Hs=8, Ws=8)
    over = dict(BAD[case])
    if over.pop("alias", False):
        over["H"] = a["yo"]
    a.update(over)
    # clear the thread's last error with a call that fails differently, so the message below is this call's
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    rc = lib.vv_obs_qc(a["ctx"], a["gt"], a["yo"], a["H"], a["interp"], a["n_out"], a["n_in"], a["thr"], a["flags"],
                       a["T"], a["C"], a["Hs"], a["Ws"], None, None)
    assert rc == 1001
    after = _msg(lib)
    assert after and after != before


def test_qc_flags():
    from vaevar.problem import qc_flags

    for name, flags in FLAG_SETS.items():
        if name != "none":
            assert qc_flags(name) == flags, name
    assert qc_flags("real_simuz_x") == FILTER | EXEMPT_Z | YO_SIMU_Z
    assert qc_flags("real_simu_nofilteringz2") == FILTER | EXEMPT_Z | YO_SIMU
    assert qc_flags("realistic") == FILTER  # the reference's prefix test, :760
    for bad in ("free_0.01", "rea", ""):
        with pytest.raises(ValueError):
            qc_flags(bad)


@pytest.mark.parametrize("n_out", [40, 7])
def test_qc_threshold_is_the_reference_expression(n_out):
    from vaevar import config as C
    from vaevar.problem import ObsInterpolater, qc_threshold

    interp = ObsInterpolater(13, n_out).interp
    std_layer = np.array(C.MODEL_STD)
    assert interp.dtype == np.float32 and std_layer.dtype == np.float64
    std_layer_aug = [std_layer[:4]]  # :135-138
    for i in range(5):
        std_layer_aug.append(np.matmul(torch.from_numpy(interp).cpu().numpy(), std_layer[4 + 13 * i:17 + 13 * i]))
    std_layer_aug = np.concatenate(std_layer_aug, 0)
    ref = 0.1 * torch.Tensor(std_layer_aug)  # :779
    thr = qc_threshold(0.1, interp, C.MODEL_STD)
    assert thr.dtype == torch.float32 and thr.shape == (4 + 5 * n_out,)
    assert torch.equal(thr, ref) and torch.equal(qc_threshold(0.1, interp), ref)
    ident = qc_threshold(0.25, None, C.MODEL_STD)
    assert ident.dtype == torch.float32 and torch.equal(ident, 0.25 * torch.Tensor(std_layer))


def test_restatement_on_a_hand_made_case():
    """1 x 204 x 2 x 3: a departure exactly at the threshold (surface channel 0, where gt_aug = gt, with gt = 0 so
    that yo - gt is thr exactly) is rejected, a NaN departure is rejected, a z-block outlier is kept under EXEMPT_Z
    and rejected without it."""
    from vaevar import config as Cf
    from vaevar.problem import ObsInterpolater, qc_threshold

    interp = ObsInterpolater(13, 40).interp
    thr = qc_threshold(0.1, interp, Cf.MODEL_STD)
    g = torch.Generator().manual_seed(3)
    gt = torch.tensor(Cf.MODEL_MEAN, dtype=torch.float32).reshape(1, -1, 1, 1) + torch.randn(1, 69, 2, 3, generator=g)
    gt[0, 0, 0, 0] = 0.0
    ga = gt_aug_ref(gt, interp)
    assert ga.shape == (1, 204, 2, 3) and torch.equal(ga[:, :4], gt[:, :4])
    yo = ga + 0.5 * thr.reshape(1, -1, 1, 1)  # inside everywhere ...
    H = torch.ones(1, 204, 2, 3)
    H[0, 5, 1, 2] = 0.0
    yo[0, 0, 0, 0] = thr[0]           # ... except: d == thr exactly,
    yo[0, 50, 1, 1] = float("nan")    # a NaN departure,
    yo[0, 10, 0, 2] = ga[0, 10, 0, 2] + 5 * thr[10]  # a z-block outlier
    yo[0, 2, 1, 0] = ga[0, 2, 1, 0] - 1.5 * thr[2]   # and a plain outlier
    assert (yo[0, 0, 0, 0] - ga[0, 0, 0, 0]) == thr[0]
    y1, H1, c1 = obs_qc_ref(gt, yo, H, interp, thr, FILTER)
    assert H1[0, 0, 0, 0] == 0 and H1[0, 50, 1, 1] == 0 and H1[0, 10, 0, 2] == 0 and H1[0, 2, 1, 0] == 0
    assert c1.dtype == torch.float64 and c1.tolist() == [[204 * 6 - 1, 204 * 6 - 1 - 4]]
    assert y1 is yo  # 'real' keeps the observations
    y2, H2, c2 = obs_qc_ref(gt, yo, H, interp, thr, FILTER | EXEMPT_Z | YO_SIMU_Z)
    assert H2[0, 10, 0, 2] == 1 and H2[0, 0, 0, 0] == 0 and H2[0, 50, 1, 1] == 0
    assert c2[0, 1] == c1[0, 1] + 1
    assert torch.equal(y2[:, 4:44], ga[:, 4:44] * H2[:, 4:44])
    keep = torch.ones(204, dtype=torch.bool)
    keep[4:44] = False
    assert torch.equal(y2[:, keep].isnan(), yo[:, keep].isnan())
    assert torch.equal(y2[:, keep].nan_to_num(7.0), yo[:, keep].nan_to_num(7.0))
    y3, H3, c3 = obs_qc_ref(gt, yo, H, interp, thr, YO_SIMU)
    assert torch.equal(H3, H) and c3[0, 0] == c3[0, 1] and torch.equal(y3, ga * H)
    assert y3[0, 5, 1, 2] == 0


@pytest.mark.parametrize("n_out", [40, 0])
def test_make_case_keeps_a_guard_band(n_out):
    c = make_case(11, 13, T=2, n_out=n_out, seed=5001, density=1.0)
    d = (c["yo"] - gt_aug_ref(c["gt"], c["interp"])).double().abs() / c["thr"].double().reshape(1, -1, 1, 1)
    assert not ((d > 0.95) & (d < 1.05)).any()
    inside = (d < 1).float().mean((0, 2, 3))
    assert (inside > 0.35).all() and (inside < 0.65).all()  # both decisions in every channel
    # the decisions do not depend on the precision gt_aug is formed in
    d64 = (c["yo"].double() - gt_aug_ref(c["gt"].double(), c["interp"])).abs() / c["thr"].double().reshape(1, -1, 1, 1)
    assert torch.equal(d64 < 1, d < 1)
    assert set(np.unique(c["H"].numpy())) == {0.5, 1.0}
    c2 = make_case(11, 13, T=3, n_out=n_out, seed=5002, density=0.02, zero_slice=1)
    assert set(np.unique(c2["H"].numpy())) == {0.0, 0.5, 1.0} and not c2["H"][1].any() and c2["H"][0].any()
