"""Observation lists on the GPU (include/vaevar.h vv_set_obs_list / vv_obs_list_eval): the kernels on
their own against the fp64 restatement (tests/_obs_list_ref.py), the list path of the vae4dvar and sc4dvar closures
against the dense path of the same problem, and two cycles of CyclicDA with obs_list on and off.

Bounds. Kernel level: every term is a handful of fp32 operations on exact fp32 inputs -- the 13-term dot product, d,
h d, / r, * coeff, and up to 40 accumulations into a gradient cell -- so with u = 2^-24: |dJ| <= 40 u J (J sums
non-negative terms in fp64), level channels |dg_j| <= 64 u sum_o |P[o][j]| |g_o| (13 + 4 + 40, and slack), direct
channels |dg| <= 8 u |g|. The fixture keeps every departure away from cancellation (|d| >= max|x|), so these hold term
by term. Closures: the bounds tests/test_gpu_obs.py::test_real_obs_closure (5e-7 J_o, 5e-5 gradient) and
tests/test_gpu_sc4dvar.py::test_sc4dvar_closure (2e-6, 5e-5) set for either path against the oracle; the achieved
values are recorded (expected: 0 for the gradient, ~1e-15 for J_o -- the same fp32 terms summed in another fp64 order)."""
import datetime as dt
import os

import numpy as np
import pytest
import torch

from _obs_list_ref import compact_ref, eval_ref, x_aug64
from conftest import GOLD, check, check_bitwise, note

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
BQ = os.path.join(GOLD, "bq_info_lr.npz")
T0 = dt.datetime(2020, 1, 1, 0)
H6 = dt.timedelta(hours=6)


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def ctx():
    from vaevar.engine import Context

    return Context.get(0)


@pytest.fixture(scope="module")
def full_dec():
    from vaevar import config as C
    from vaevar.engine import LGUnet

    return LGUnet(C.DECODER, 1, 1).load_synthetic()


def _fields(interp, x, H, seed):
    """yo = x_aug(x) +- s (1 + u), s = max|x|, u in [2^-20, 1) (clear of the fp32 rounding of yo, at most 3 s 2^-24):
    |d| >= s, no departure cancels; R in [0.5, 1.5)."""
    from vaevar.synth import splitmix_uniform

    xa = x_aug64(interp, x)
    s = float(np.abs(x).max())
    u = splitmix_uniform(seed, 3 * xa.size).reshape((3,) + xa.shape)
    yo = (xa + np.where(u[0] < 0.5, -1.0, 1.0) * s * (1.0 + 2.0 ** -20 + (1.0 - 2.0 ** -20) * u[1])).astype(np.float32)
    R = (0.5 + u[2]).astype(np.float32)
    return yo, R, s


def _check_eval(ctx, tag, interp, x, yo, H, R, coeff, s):
    """vv_obs_list_eval against the restatement, with the module docstring's bounds; returns the restatement."""
    from vaevar.engine import obs_list_eval

    n_out, n_in = interp.shape
    T = x.shape[0]
    L = compact_ref(yo, H, R, n_out)
    E = eval_ref(L, interp, x, coeff)
    assert E["dmin"] >= s, (E["dmin"], s)  # the fixture rule: no departure cancels
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (interp, x, yo, H, R)]
    out = torch.full(x.shape, float("nan"), device="cuda")
    g, J, counts = obs_list_eval(ctx, *d, coeff=coeff, out=out)
    g = g.cpu().numpy().astype(np.float64).reshape(E["g"].shape)
    check_bitwise(f"{tag} counts vs restatement", counts, L["counts"])
    for t in range(T):
        if L["counts"][t, 1] == 0:
            check(f"{tag} J[{t}] of an empty slot", J[t], 0.0, "==")
        else:
            check(f"{tag} J[{t}] / (u J)", abs(J[t] - E["J"][t]) / (U * E["J"][t]), 40.0, "<=")
    cells = E["cells"]
    assert not np.isnan(g).any()
    check(f"{tag} g_obs off the units", np.abs(g[~cells]).max() if (~cells).any() else 0.0, 0.0, "==")
    err = np.abs(g - E["g"])
    lev, dirc = np.zeros_like(cells), np.zeros_like(cells)
    lev[:, 4:], dirc[:, :4] = cells[:, 4:], cells[:, :4]
    zero = lev & (E["gabs"] == 0)  # a level no record of the unit has a weight on
    check(f"{tag} level cells without a weight", err[zero].max() if zero.any() else 0.0, 0.0, "==")
    m = lev & (E["gabs"] > 0)
    check(f"{tag} level dg / (u sum |P||g|)", (err[m] / (U * E["gabs"][m])).max(), 64.0, "<=")
    zero = dirc & (E["g"] == 0)  # the unrecorded channels of a direct unit
    check(f"{tag} unrecorded direct cells", np.abs(g[zero]).max() if zero.any() else 0.0, 0.0, "==")
    m = dirc & (E["g"] != 0)
    check(f"{tag} direct dg / (u |g|)", (err[m] / (U * np.abs(E["g"][m]))).max(), 8.0, "<=")
    g2, J2, counts2 = obs_list_eval(ctx, *d, coeff=coeff)
    check_bitwise(f"{tag} second call: g_obs", g2.cpu().numpy().reshape(g.shape), g)
    check_bitwise(f"{tag} second call: J", J2, J)
    check_bitwise(f"{tag} second call: counts", counts2, counts)
    return L, E


@pytest.mark.parametrize("n_out", [40, 7])
def test_obs_list_kernels(ctx, n_out):
    """T = 2 on a 33 x 47 grid (HW = 1551, a multiple of neither 64 nor 256), 13 state levels. Slot 0: a sparse random
    station set, and on cleared columns a pixel with only direct channel 3, one with one level of one variable, one
    with every level of all five variables (one entry H = 0.5), units whose only record is the first / the last level,
    a direct unit with only channel 0, pixel 0 and pixel HW - 1 observed. Slot 1 entirely unobserved."""
    from vaevar.problem import ObsInterpolater
    from vaevar.synth import smooth_field, splitmix_uniform

    T, Hs, Ws, n_in = 2, 33, 47, 13
    HW, Ca, last = Hs * Ws, 4 + 5 * n_out, n_out - 1
    interp = np.ascontiguousarray(ObsInterpolater(n_in, n_out).interp, np.float32)
    x = (3.0 * smooth_field(9100 + n_out, (T, 4 + 5 * n_in, Hs, Ws), sigma=2.0)).astype(np.float32)
    st = splitmix_uniform(9200, HW) < 0.03
    H = np.zeros((T, Ca, HW), np.float32)
    H[0] = (st[None] & (splitmix_uniform(9201, Ca * HW).reshape(Ca, HW) < 0.5)).astype(np.float32)
    special = [0, HW - 1, 100, 200, 300, 400, 401, 402, 403, 404]
    H[0][:, special] = 0.0
    H[0, 0, 0] = H[0, 4 + min(5, last), 0] = 1.0                  # pixel 0
    H[0, 0:4, HW - 1] = H[0, 4 + 4 * n_out + last, HW - 1] = 1.0  # pixel HW - 1
    H[0, 3, 100] = 1.0                                            # only direct channel 3
    H[0, 4 + 2 * n_out + min(17, last), 200] = 1.0                # one level of one variable
    H[0, 4:, 300] = 1.0                                           # every level of all five variables
    H[0, 4 + 3, 300] = 0.5
    H[0, 4 + 1 * n_out, 400] = H[0, 4, 403] = 1.0                 # only o = 0
    H[0, 4 + 3 * n_out + last, 401] = H[0, 4 + 4 * n_out + last, 404] = 1.0  # only the last level
    H[0, 0, 402] = 1.0                                            # a direct unit with only channel 0
    H = H.reshape(T, Ca, Hs, Ws)
    assert not H[0].reshape(Ca, HW).any(0).all() and not H[1].any()  # unobserved pixels; an empty slot
    yo, R, s = _fields(interp, x, H, 9300 + n_out)
    L, _ = _check_eval(ctx, f"obs list 13->{n_out}", interp, x, yo, H, R, 0.75, s)
    assert L["counts"][1].tolist() == [0, 0] and L["counts"][0, 0] > 20


def test_obs_list_kernels_more_units_than_threads(ctx):
    """A 300 x 301 grid with a 2 -> 3 level operator, every pixel observed in direct channel 0 and in one level of each
    variable: 541 800 units, more than the 1024 x 256 lanes of one pass of the evaluation kernel (its grid-stride
    loop), and 2117 scan blocks, more than the 1024 threads of the block-sum scan (a chunk of 3 per thread)."""
    from vaevar.synth import smooth_field

    Hs, Ws = 300, 301
    HW = Hs * Ws
    interp = np.array([[1.0, 0.0], [0.25, 0.75], [0.0, 1.0]], np.float32)
    x = (2.0 * smooth_field(9400, (1, 14, Hs, Ws), sigma=2.0)).astype(np.float32)
    H = np.zeros((1, 19, HW), np.float32)
    H[0, 0] = 1.0
    p = np.arange(HW)
    for v in range(5):
        H[0, 4 + 3 * v + (p + v) % 3, p] = 1.0
    H = H.reshape(1, 19, Hs, Ws)
    yo, R, s = _fields(interp, x, H, 9401)
    L, _ = _check_eval(ctx, "obs list 541800 units", interp, x, yo, H, R, 1.0, s)
    assert L["counts"].tolist() == [[6 * HW, 6 * HW]]


def _poison(prob):
    for t in (prob.yo, prob.H, prob.R):
        t.fill_(float("nan"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("T,Hs,Ws", [(1, 128, 256), (2, 150, 300)])
def test_obs_list_in_the_closure(full_dec, T, Hs, Ws):
    """The vae4dvar closure of test_real_obs_closure's problem, dense and from the list."""
    from vaevar import config as C
    from vaevar.engine import DAProblem, LGUnet
    from vaevar.problem import make_real_problem
    from vaevar.synth import smooth_field

    tag = f"obs list closure T={T} {Hs}x{Ws}"
    p = make_real_problem(Hs=Hs, Ws=Ws, T=T, seed=20250623, obs_frac=0.05)
    flow = LGUnet(C.FLOW, 1, 1).load_synthetic() if T > 1 else None
    prob = DAProblem(full_dec, p, flow=flow)
    cx = prob.ctx
    z = torch.from_numpy(0.3 * smooth_field(406, (1, 32, 128, 256))).cuda()

    def ev():
        g = torch.empty(1, 32, 128, 256, device="cuda")
        jb, jo = prob.closure(z, g)
        return jb, jo, g.cpu()

    def same(name, a, b):
        check_bitwise(f"{tag} {name}: J_b", a[0], b[0])
        check_bitwise(f"{tag} {name}: J_o", a[1], b[1])
        check_bitwise(f"{tag} {name}: dJ/dz", a[2], b[2])

    dense = ev()
    assert prob.obs_list_info == {"enabled": False, "units": 0, "records": 0, "bytes": 0}
    prob.obs_list(True)
    info = prob.obs_list_info
    want = compact_ref(p["yo"], p["H"], p["R"], 40)["counts"].sum(0)
    assert info["enabled"] and info["bytes"] >= 16 * info["records"]
    check_bitwise(f"{tag} units, records vs restatement", [info["units"], info["records"]], want)
    graphs = cx.closure_graph_state(1)["enabled"]
    cx.set_closure_graph(True)
    prob.obs_list(True)  # a second build of the same fields
    lst = ev()           # eager: the first evaluation after the graphs were dropped
    check_bitwise(f"{tag} J_b list vs dense", lst[0], dense[0])
    e_j, e_g = abs(lst[1] - dense[1]) / abs(dense[1]), rel(lst[2], dense[2])
    note(f"{tag} J_o list vs dense (achieved)", e_j)
    note(f"{tag} dJ/dz list vs dense (achieved)", e_g)
    check(f"{tag} J_o list vs dense", e_j, 5e-7)
    check(f"{tag} dJ/dz list vs dense", e_g, 5e-5)
    same("captured graph vs eager", ev(), lst)
    same("graph replay vs eager", ev(), lst)
    state = cx.closure_graph_state(1)
    assert state["instantiated"] and not state["eager_only"] and state["launches"] >= 2, state
    cx.set_closure_graph(False)
    same("graphs off", ev(), lst)
    cx.set_closure_graph(graphs)
    prob.obs_list(False)
    assert not prob.obs_list_info["enabled"]
    same("dense path restored", ev(), dense)
    prob.obs_list(True)
    same("list rebuilt", ev(), lst)
    _poison(prob)
    same("yo, H, R overwritten with NaN", ev(), lst)
    same("yo, H, R overwritten with NaN, again", ev(), lst)
    # a rebind leaves the list off
    prob2 = DAProblem(full_dec, p, flow=flow)
    assert not prob2.obs_list_info["enabled"]
    same("rebound problem (dense)", (lambda g: prob2.closure(z, g) + (g.cpu(),))(torch.empty_like(z)), dense)


def test_obs_list_in_the_sc4dvar_closure():
    """The "real" case of test_sc4dvar_closure (128 x 256, T = 1), dense and from the list."""
    from vaevar.problem import make_real_problem
    from vaevar.sc4dvar import BMatrix, Sc4dvarProblem

    tag = "obs list sc4dvar closure"
    p = make_real_problem(nch=69, Hs=128, Ws=256, T=1, seed=21, dim_out=40)
    prob = Sc4dvarProblem(BMatrix.from_npz(BQ), p)
    w = (torch.randn(69, 128, 256, generator=torch.Generator().manual_seed(9)) * 0.3).cuda()

    def ev():
        g = torch.empty(69, 128, 256, device="cuda")
        jb, jo = prob.closure(w, g)
        return jb, jo, g.cpu()

    dense = ev()
    prob.obs_list(True)
    info = prob.obs_list_info
    want = compact_ref(p["yo"], p["H"], p["R"], 40)["counts"].sum(0)
    check_bitwise(f"{tag} units, records vs restatement", [info["units"], info["records"]], want)
    lst = ev()
    check_bitwise(f"{tag} J_b list vs dense", lst[0], dense[0])
    e_j, e_g = abs(lst[1] - dense[1]) / abs(dense[1]), rel(lst[2], dense[2])
    note(f"{tag} J_o list vs dense (achieved)", e_j)
    note(f"{tag} dJ/dw list vs dense (achieved)", e_g)
    check(f"{tag} J_o list vs dense", e_j, 2e-6)
    check(f"{tag} dJ/dw list vs dense", e_g, 5e-5)
    _poison(prob)
    again = ev()
    for k, name in enumerate(("J_b", "J_o", "dJ/dw")):
        check_bitwise(f"{tag} yo, H, R overwritten with NaN: {name}", again[k], lst[k])
    # the identity operator has no list
    from vaevar._lib import VVError
    from vaevar.problem import make_problem

    ident = Sc4dvarProblem(BMatrix.from_npz(BQ), make_problem(nch=69, Hs=128, Ws=256, T=1, seed=21))
    assert not ident.obs_list_info["enabled"]
    with pytest.raises(VVError, match="1002"):
        ident.obs_list(True)


FILES = ("xb", "bg_wrmse", "ana_wrmse", "bg_bias", "ana_bias", "error_obs")


def test_obs_list_cycle(tmp_path):
    """Two cycles of the real-observation sc4dvar cycle of tests/test_gpu_cycle_modes.py (128 x 256, 3 % of the
    observation entries, use_eval on). obs_list=False writes the bits of a run that never passed the keyword. With
    obs_list=True the closures agree with the dense ones to rounding (above), so the runs follow the same line
    searches: xb.npy and the metric files are held to 1e-6 of the dense run's (max-norm relative), the bound
    tests/test_gpu_obs_qc.py::test_real_obs_filtered_cycle sets for analyses from inputs equal to rounding."""
    from vaevar import config as C
    from vaevar.cycle import CyclicDA, SyntheticRealObs
    from vaevar.engine import LGUnet
    from vaevar.problem import ObsInterpolater, make_problem
    from vaevar.sc4dvar import BMatrix
    from vaevar.synth import smooth_field, splitmix_uniform

    mean = np.asarray(C.MODEL_MEAN, np.float32)[:, None, None]
    std = np.asarray(C.MODEL_STD, np.float32)[:, None, None]
    fields = {}

    def truth(t):
        k = int((t - T0).total_seconds() // 3600)
        if k not in fields:
            fields[k] = (mean + std * smooth_field(6100 + k, (69, 128, 256))).astype(np.float32)
        return fields[k]

    p = make_problem(nch=69, Hs=128, Ws=256, T=1, seed=8181, obs_frac=0.03)
    fc = LGUnet(C.FLOW, 1, 1).load_synthetic()
    interp = ObsInterpolater(13, 40).interp
    H = (splitmix_uniform(84, 204 * 128 * 256).reshape(1, 204, 128, 256) < 0.03).astype(np.float32)
    mask = (splitmix_uniform(83, 128 * 256).reshape(128, 256) < 0.3).astype(np.float32)
    obs = SyntheticRealObs(fc.ctx, truth, H, p["R"], interp)
    out = {}
    for name, kw in (("plain", {}), ("off", {"obs_list": False}), ("on", {"obs_list": True})):
        cyc = CyclicDA(fc, obs, T0, T0 + 2 * H6, Nit=1, name=name, da_mode="sc4dvar", bmatrix=BMatrix.from_npz(BQ),
                       out_dir=str(tmp_path), xb0=p["xb"], obs_interp=interp, use_eval=True, mask_eval=mask, **kw)
        cyc.run_assimilation()
        out[name] = {f: np.load(os.path.join(str(tmp_path), name, f + ".npy")) for f in FILES}
        assert out[name]["error_obs"].shape == (2, 204) and out[name]["ana_wrmse"].shape == (2, 69)
    for f in FILES:
        check_bitwise(f"cycle {f}.npy: obs_list=False vs no keyword", out["off"][f], out["plain"][f])
        fin = np.isfinite(out["off"][f])
        assert np.array_equal(fin, np.isfinite(out["on"][f]))
        check(f"cycle {f}.npy: obs_list=True vs False", rel(out["on"][f][fin], out["off"][f][fin]), 1e-6, "<=")
