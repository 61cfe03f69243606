"""GPU: Metrics.verify (vv_verify), the forecast-verification statistics in one pass, against what the reference's
utils.metrics.Metrics gave for the same inputs (tests/golden/g19_verify.npz; inputs from tests/_verify_ref.py). The
bound is the CPU restatement's: relative error against the statistic's largest magnitude over channels < 1e-6, the
project's G9 Bias bound for this kind of quantity, about 5x the reference's own fp32-vs-fp64 spread (< 3e-7, recorded
per statistic in the fixture)."""
import os

import numpy as np
import pytest
import torch

from _verify_ref import CASES, CLIM_NAMES, ERROR_NAMES, NAMES, make_case, rel_err
from conftest import GOLD, check, check_bitwise

pytestmark = pytest.mark.gpu

BOUND = 1e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g19_verify.npz"))


@pytest.fixture(scope="module")
def ctx():
    from vaevar.engine import Context

    return Context.get(0)


_CASE = {}


def _case(ctx, name):
    """(Metrics, device inputs) of a golden case, made once and left unchanged."""
    from vaevar.metrics import Metrics

    if name not in _CASE:
        d = make_case(name)
        m = Metrics(ctx, d["mean"], d["std"])
        m.scale = torch.from_numpy(d["scale"]).cuda()
        _CASE[name] = (m, {k: torch.from_numpy(d[k]).cuda() for k in ("pred", "gt", "clim")})
    return _CASE[name]


@pytest.mark.parametrize("case", list(CASES))
def test_verify_vs_reference(gold, ctx, case):
    """Every statistic with and without the climatology; the error family is the same bits in both runs, the
    climatology keys are absent without clim and their rows of the raw output are NaN."""
    from vaevar._lib import check as rc_check, lib
    from vaevar.engine import _ptr, _stream
    from vaevar.metrics import _ptr64

    m, x = _case(ctx, case)
    full = m.verify(x["pred"], x["gt"], x["clim"])
    bare = m.verify(x["pred"], x["gt"])
    assert tuple(full) == NAMES and tuple(bare) == ERROR_NAMES
    C = x["pred"].shape[1]
    for name in NAMES:
        v = full[name]
        assert v.dtype == torch.float64 and v.shape == (C,) and v.is_cuda
        e = rel_err(v.cpu().numpy(), gold[f"{case}_{name}"])
        print(f"{case} {name}: {e:.2e}")
        check(f"verify {case} {name}", e, BOUND)
    for name in ERROR_NAMES:
        check_bitwise(f"verify {case} {name} with vs without clim", full[name], bare[name])
    B, _, H, W = x["pred"].shape
    raw = torch.zeros(len(NAMES), C, device="cuda", dtype=torch.float64)
    rc_check(lib.vv_verify(ctx.h, _ptr(x["pred"]), _ptr(x["gt"]), None, _ptr(m.mean), _ptr(m.std), _ptr64(m.scale),
                           B, C, H, W, _ptr64(raw), _stream()), "verify")
    assert bool(torch.isnan(raw[len(ERROR_NAMES):]).all()) and bool(torch.isfinite(raw[:len(ERROR_NAMES)]).all())


def test_verify_accepts_3d_and_rejects_mismatch(gold, ctx):
    m, x = _case(ctx, "h37_w20")
    r4 = m.verify(x["pred"], x["gt"], x["clim"])
    r3 = m.verify(x["pred"][0], x["gt"][0], x["clim"])
    for name in NAMES:
        check_bitwise(f"verify (C,H,W) {name}", r3[name], r4[name])
    with pytest.raises(ValueError):
        m.verify(x["pred"], x["gt"][:, :, :-1])
    with pytest.raises(ValueError):
        m.verify(x["pred"][:, :1], x["gt"][:, :1])
    with pytest.raises(ValueError):
        m.verify(x["pred"], x["gt"], x["clim"][:, :-1])


@pytest.mark.parametrize("case", ["h37_w18", "workload"])
def test_verify_agrees_with_vv_metrics(ctx, case):
    """WRMSE and Bias are what vv_metrics returns for the same fields: the same fp32 terms and weights, fp64 sums in
    another order (a difference near 1e-16), then the same fp32 roundings, so the two agree unless a sum sits on a
    rounding boundary: within 2 ulp of fp32 of the statistic's largest magnitude."""
    m, x = _case(ctx, case)
    r = m.verify(x["pred"], x["gt"])
    w, b = m.wrmse_bias(x["pred"], x["gt"])
    for name, old in (("WRMSE", w), ("Bias", b)):
        e = rel_err(r[name].cpu().numpy(), old.cpu().numpy())
        check(f"verify {case} {name} vs vv_metrics", e, 2.0 ** -22, "<=")


@pytest.mark.parametrize("case", ["h37_w18", "workload"])
def test_verify_repeats_bitwise(ctx, case):
    m, x = _case(ctx, case)
    a = m.verify(x["pred"], x["gt"], x["clim"])
    b = m.verify(x["pred"], x["gt"], x["clim"])
    for name in NAMES:
        check_bitwise(f"verify {case} {name} second call", a[name], b[name])


@pytest.mark.parametrize("case", ["h37_w18", "h37_w20"])
def test_wacc_of_a_perfect_forecast_is_one(ctx, case):
    """pred == gt: sum(w p' t'), sum(w p'^2) and sum(w t'^2) are the same number s, so WACC = s / sqrt(s * s) = 1 up to
    the fp32 roundings of the product, the root and the quotient: within 4 ulp of fp32. (A climatology EQUAL to the
    truth makes t' = 0 and WACC = 0 / 0: NaN, in the reference too -- checked as well.)"""
    m, x = _case(ctx, case)
    r = m.verify(x["gt"], x["gt"], x["clim"])
    ulp = float(np.spacing(np.float32(1.0)))
    for name in ("WACC", "NWACC", "SWACC", "TWACC"):
        check(f"verify {case} {name} of pred == gt", float((r[name] - 1.0).abs().max()), 4 * ulp, "<=")
    for name in ERROR_NAMES:
        check(f"verify {case} {name} of pred == gt", float(r[name].abs().max()), 0.0, "==")
    r = m.verify(x["pred"], x["gt"], x["gt"][0])
    for name in ("WACC", "NWACC", "SWACC", "TWACC"):
        assert bool(torch.isnan(r[name]).all()), name


@pytest.mark.parametrize("case", ["h37_w18", "h37_w20"])
def test_junk_climatology_leaves_error_family(ctx, case):
    m, x = _case(ctx, case)
    good = m.verify(x["pred"], x["gt"], x["clim"])
    junk = x["clim"].clone()
    junk.view(-1)[::3] = float("nan")
    junk.view(-1)[1::3] = float("inf")
    junk.view(-1)[2::3] = -3.0e38
    bad = m.verify(x["pred"], x["gt"], junk)
    for name in ERROR_NAMES:
        check_bitwise(f"verify {case} {name} with junk clim", bad[name], good[name])
    assert not any(bool(torch.isfinite(bad[n]).any()) for n in CLIM_NAMES if n.endswith(("Activity", "WACC")))


@pytest.mark.parametrize("with_clim", [False, True])
def test_verify_profiled_as_misfit(ctx, with_clim):
    m, x = _case(ctx, "h37_w18")
    m.verify(x["pred"], x["gt"], x["clim"])  # the weight table of this height is uploaded
    ctx.profile_start()
    m.verify(x["pred"], x["gt"], x["clim"] if with_clim else None)
    prof = ctx.profile_stop()
    assert prof["misfit"]["launches"] == 1 and prof["misfit"]["ms"] > 0
    assert sum(v["launches"] for k, v in prof.items() if k != "misfit") == 0
    assert prof["misfit"]["bytes"] == 4.0 * x["pred"].numel() * (3 if with_clim else 2)
