"""CPU: the forecast-verification statistics (vv_verify, Metrics.verify). The project's restatement
(tests/_verify_ref.py) against what the reference's utils.metrics.Metrics gave for the same inputs
(tests/golden/g19_verify.npz, tools/make_verify_fixture.py), and the entry point's argument checks, which are made
before any device work: a dummy non-null handle stands in for the context, so no GPU is needed."""
import ctypes
import os

import numpy as np
import pytest

from _verify_ref import CASES, NAMES, STORED_INPUTS, make_case, region_bounds, rel_err, verify_ref
from conftest import GOLD

# the project's G9 Bias bound for this kind of quantity; about 5x the reference's own fp32-vs-fp64 spread (< 3e-7,
# recorded per statistic in the fixture)
BOUND = 1e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g19_verify.npz"))


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_matches_reference(gold, case):
    d = make_case(case)
    if case in STORED_INPUTS:  # the generator still makes the inputs the reference was run on
        for k, v in d.items():
            assert np.array_equal(gold[f"{case}_{k}"], v), k
    got = verify_ref(d["pred"], d["gt"], d["clim"], d["mean"], d["std"], d["scale"])
    assert set(got) == set(NAMES)
    for name in NAMES:
        assert float(gold[f"{case}_spread_{name}"]) < 3e-7
        e = rel_err(got[name], gold[f"{case}_{name}"])
        print(f"{case} {name}: {e:.2e}")
        assert e < BOUND, (name, e)


def test_region_bounds():
    assert region_bounds(5) == (2, 3) and region_bounds(37) == (14, 23) and region_bounds(721) == (280, 441)


def test_verify_exported_and_versioned():
    import re

    from conftest import ROOT
    from vaevar import _lib
    from vaevar.metrics import VERIFY_NAMES

    assert "vv_verify" in _lib.EXPORTED and hasattr(_lib.lib, "vv_verify")
    hdr = open(os.path.join(ROOT, "include", "vaevar.h")).read()
    assert sorted(set(re.findall(r"^int\s+(vv_\w+)\s*\(", hdr, flags=re.M))) == _lib.EXPORTED
    assert _lib.lib.vv_version() >= 108
    # the documented enum is the order Metrics.verify names the rows in
    enum = re.search(r"enum \{(.*?)VV_VERIFY_NSTAT", hdr, flags=re.S).group(1)
    assert [n.strip()[len("VV_VERIFY_"):].split(" ")[0] for n in enum.split(",") if n.strip()] == \
        [n.upper() for n in VERIFY_NAMES]
    assert VERIFY_NAMES == NAMES


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def _call(lib, ctx, pred, gt, clim, mean, std, scale, B, C, H, W, out):
    return lib.vv_verify(ctx, pred, gt, clim, mean, std, scale, B, C, H, W, out, None)


@pytest.mark.parametrize("case", ["null_ctx", "null_pred", "null_gt", "null_mean", "null_std", "null_scale",
                                  "null_out", "B_0", "C_0", "W_0", "H_0", "H_1", "H_2", "H_4"])
def test_verify_rejects_bad_arguments(case):
    from vaevar import _lib

    lib = _lib.lib
    keep = ctypes.create_string_buffer(1 << 12)  # never dereferenced: every case fails before the context is used
    b = ctypes.cast(keep, ctypes.c_void_p)
    a = dict(ctx=b, pred=b, gt=b, clim=None, mean=b, std=b, scale=b, B=1, C=2, H=37, W=8, out=b)
    a.update({"null_ctx": dict(ctx=None), "null_pred": dict(pred=None), "null_gt": dict(gt=None),
              "null_mean": dict(mean=None), "null_std": dict(std=None), "null_scale": dict(scale=None),
              "null_out": dict(out=None), "B_0": dict(B=0), "C_0": dict(C=0), "W_0": dict(W=0), "H_0": dict(H=0),
              "H_1": dict(H=1), "H_2": dict(H=2), "H_4": dict(H=4)}[case])
    # clear the thread's last error with a call that fails differently, so the message below is this call's
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    assert _call(lib, **a) == 1001
    after = _msg(lib)
    assert after and after != before


def test_empty_region_heights():
    """The heights the entry point refuses are exactly those whose index formulas leave a region empty."""
    bad = [H for H in range(1, 200) if not 0 < region_bounds(H)[0] < region_bounds(H)[1] < H]
    assert bad == [1, 2, 4]
