"""vv_obs_qc / engine.obs_qc / cycle.RealObs (the departure filter of get_obs_info for the obs_type real* family,
da_4dvar.py:764-800) on the GPU against the torch CPU restatement of those lines (tests/_obs_qc_ref.py) and against
the same steps composed on the device from vv_obs_augment and torch element-wise ops.

What is exact: H' (the cases keep every departure at least 10 % away from its threshold, tests/_obs_qc_ref.make_case, so
no element is left out of the comparison), the counts (sums of 0 / 0.5 / 1 are exact in float64 in any order), the
untouched channels of yo, determinism, and everything against the device composition (the operator in registers is
k_obs_augment's). What has a tolerance: yo' on the simu channels against the CPU restatement, per channel
max|yo' - ref| <= 1e-6 max|ref|, the vv_obs_augment bound of DESIGN §2 (F.linear on the CPU and the kernel's FMA chain
round a 13-term dot product differently).

Grids: 33 x 47 = 1551 pixels (a ragged last 64-pixel segment), 1 x 300 (a single row), 67 x 131 = 8777 (three
4096-pixel chunks, the last ragged). Operators 13 -> 40, 13 -> 7 and the identity; T = 1, and T = 3 with the middle time
slice of H all zero; station densities 2 % and 100 % (and two at the kernel's switch between its two walks over the
observed entries); the five obs_type flag sets and flags = 0 (the identity operator
has no z block, so the two ...z sets do not apply to it)."""
import datetime as dt

import numpy as np
import pytest
import torch

from _obs_qc_ref import FILTER, FLAG_SETS, YO_SIMU, make_case, obs_qc_composed, obs_qc_ref, simu_channels
from conftest import check, check_bitwise

pytestmark = pytest.mark.gpu

GRIDS = {"33x47": (33, 47), "1x300": (1, 300), "67x131": (67, 131)}
OPS = {"r40": 40, "r7": 7, "id": 0}
CASES = [(g, o, T, d) for g in GRIDS for o in OPS for T in (1, 3) for d in (0.02, 1.0)]
# the kernel takes the observed entries of a (64 pixels, channel group) block as a list up to 512 of them and walks
# the channels beyond: densities at which the blocks of a 40-channel (2560 entries) and of a 64-channel group (4096)
# hold about 512, so that both walks and the switch between them occur in one call
CASES += [("67x131", "r40", 1, 0.2), ("67x131", "id", 3, 0.125)]
T0 = dt.datetime(2018, 1, 1, 0)
H6 = dt.timedelta(hours=6)


def _id(c):
    return f"{c[0]}-{c[1]}-T{c[2]}-d{c[3]}"


def _flag_sets(n_out):
    return {k: f for k, f in FLAG_SETS.items() if n_out or not k.endswith("z")}


@pytest.fixture(scope="module")
def ctx():
    from vaevar.engine import Context

    return Context.get(0)


_CASES: dict = {}


def _case(key):
    """The seeded inputs of a case and the restatement's outputs per flag set, computed once and never modified."""
    if key not in _CASES:
        g, o, T, d = key
        c = make_case(*GRIDS[g], T=T, n_out=OPS[o], seed=5100 + 7 * CASES.index(key), density=d,
                      zero_slice=1 if T == 3 else None)
        c["ref"] = {k: obs_qc_ref(c["gt"], c["yo"], c["H"], c["interp"], c["thr"], f)
                    for k, f in _flag_sets(c["n_out"]).items()}
        _CASES[key] = c
    return _CASES[key]


def _dev(c):
    d = {k: c[k].cuda() for k in ("gt", "yo", "H", "thr")}
    d["interp"] = None if c["interp"] is None else torch.from_numpy(c["interp"]).cuda()
    return d


def _run(ctx, d, flags, **over):
    """obs_qc on fresh copies of yo and H; returns (yo', H', counts) on the device."""
    from vaevar.engine import obs_qc

    a = dict(d, **over)
    yo, H = a["yo"].clone(), a["H"].clone()
    counts = obs_qc(ctx, a["gt"], yo, H, a["interp"], a["thr"], flags)
    return yo, H, counts


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_obs_qc_vs_restatement_and_device_composition(ctx, key):
    c = _case(key)
    d = _dev(c)
    c_obs = c["yo"].shape[1]
    for name, flags in _flag_sets(c["n_out"]).items():
        tag = f"{_id(key)} {name}"
        yo_r, H_r, cnt_r = c["ref"][name]
        yo, H, cnt = _run(ctx, d, flags)
        assert cnt.shape == (c["gt"].shape[0], 2) and cnt.dtype == torch.float64
        check_bitwise(f"{tag} H'", H, H_r)
        check_bitwise(f"{tag} counts vs float64 sums of H and the reference H'", cnt, cnt_r)
        simu = simu_channels(flags, c_obs, c["n_out"])
        if simu.any():
            ref = yo_r[:, simu]
            err = (yo.cpu()[:, simu] - ref).abs().amax((0, 2, 3))
            scale = ref.abs().amax((0, 2, 3))
            assert torch.isfinite(err).all()
            check(f"{tag} yo' simu channels, max over channels of max|yo' - ref| / max|ref|",
                  (err / scale.clamp_min(1e-30)).max(), 1e-6, "<=")
            check(f"{tag} yo' simu channels with an all-zero reference", err[scale == 0].sum() if (scale == 0).any()
                  else 0.0, 0.0, "==")
        if not simu.all():
            check_bitwise(f"{tag} yo on the other channels", yo[:, ~simu], c["yo"][:, ~simu])
        if flags & FILTER and key[3] == 1.0:
            assert float(cnt[0, 1]) < float(cnt[0, 0])  # the case does reject
        # bit for bit the composition of obs_augment and torch element-wise ops on the GPU: the operator in registers
        # is k_obs_augment's (-0 of the composition's gt_aug * 0 compares equal to the kernel's +0)
        yo_c, H_c, cnt_c = obs_qc_composed(ctx, d["gt"], d["yo"], d["H"], d["interp"], d["thr"], flags)
        check_bitwise(f"{tag} H' vs device composition", H, H_c)
        check_bitwise(f"{tag} yo' vs device composition", yo, yo_c)
        check_bitwise(f"{tag} counts vs device composition", cnt, cnt_c)
        # determinism: a second call on fresh copies
        yo2, H2, cnt2 = _run(ctx, d, flags)
        check_bitwise(f"{tag} second call H'", H2, H)
        check_bitwise(f"{tag} second call yo'", yo2, yo)
        check_bitwise(f"{tag} second call counts", cnt2, cnt)


@pytest.mark.parametrize("key", [("33x47", "r40", 3, 0.02), ("67x131", "r7", 1, 0.02), ("1x300", "id", 3, 0.02),
                                 ("67x131", "id", 1, 0.02)], ids=_id)
def test_obs_qc_ignores_unobserved_entries(ctx, key):
    """NaN in yo wherever H == 0, and NaN in a pixel's gt column wherever no channel that reads the column is observed
    (a surface channel reads its own gt channel, the channels of a pressure-level variable its 13 levels), change no
    bit of H', of the counts or of yo' on the simu channels; the other channels of yo keep the junk they were given."""
    c = _case(key)
    d = _dev(c)
    n_out, c_obs = c["n_out"], c["yo"].shape[1]
    off = d["H"] == 0
    yo_j = torch.where(off, torch.full_like(d["yo"], float("nan")), d["yo"])
    gt_j = d["gt"].clone()
    if n_out:
        gt_j[:, :4][off[:, :4]] = float("nan")
        for i in range(5):
            unseen = off[:, 4 + n_out * i:4 + n_out * (i + 1)].all(1, keepdim=True)
            blk = gt_j[:, 4 + 13 * i:17 + 13 * i]
            blk[unseen.expand_as(blk)] = -7e37 if i % 2 else float("nan")
    else:
        gt_j[off] = float("nan")
    assert int((gt_j != d["gt"]).sum()) > gt_j.numel() // 4 and int(torch.isnan(yo_j).sum()) > yo_j.numel() // 2
    for name, flags in _flag_sets(n_out).items():
        tag = f"{_id(key)} {name}"
        yo, H, cnt = _run(ctx, d, flags)
        yo2, H2, cnt2 = _run(ctx, d, flags, yo=yo_j, gt=gt_j)
        check_bitwise(f"{tag} H' with junk at H == 0", H2, H)
        check_bitwise(f"{tag} counts with junk at H == 0", cnt2, cnt)
        simu = torch.from_numpy(simu_channels(flags, c_obs, n_out)).cuda()
        if simu.any():
            assert torch.isfinite(yo2[:, simu]).all()
            check_bitwise(f"{tag} yo' simu channels with junk at H == 0", yo2[:, simu], yo[:, simu])
        if not simu.all():
            check_bitwise(f"{tag} yo other channels keep their input", yo2[:, ~simu], yo_j[:, ~simu])


def test_obs_qc_h_zero_gives_plus_zero(ctx):
    """yo' at an unobserved entry of a simu channel is +0 (the reference's gt_aug * 0 is -0 for a negative gt_aug)."""
    c = _case(("33x47", "r40", 1, 0.02))
    yo, H, _ = _run(ctx, _dev(c), YO_SIMU)
    z = yo[H == 0]
    assert z.numel() > 0 and not z.any() and not torch.signbit(z).any()


def test_obs_qc_profiled_as_misfit(ctx):
    from vaevar.engine import obs_qc

    c = _case(("33x47", "r40", 1, 0.02))
    d = _dev(c)
    yo, H = d["yo"].clone(), d["H"].clone()
    ctx.profile_start()
    obs_qc(ctx, d["gt"], yo, H, d["interp"], d["thr"], FILTER | YO_SIMU)
    prof = ctx.profile_stop()
    assert prof["misfit"]["launches"] == 1 and prof["misfit"]["ms"] > 0
    assert sum(v["launches"] for v in prof.values()) == 1
    # Hmask and the truth once, yo read (filter) and written (simu) on all 204 channels
    assert prof["misfit"]["bytes"] == 4.0 * 33 * 47 * (204 + 69 + 204 + 204)


def test_obs_qc_python_checks(ctx):
    from vaevar.engine import obs_qc

    d = _dev(_case(("33x47", "r40", 1, 0.02)))
    with pytest.raises(ValueError, match="operator expects"):
        obs_qc(ctx, d["gt"][:, :68], d["yo"].clone(), d["H"].clone(), d["interp"], d["thr"], FILTER)
    with pytest.raises(ValueError, match="yo / H"):
        obs_qc(ctx, d["gt"], d["yo"].clone(), d["H"].clone(), None, d["thr"], FILTER)
    with pytest.raises(ValueError, match="thr"):
        obs_qc(ctx, d["gt"], d["yo"].clone(), d["H"].clone(), d["interp"], d["thr"][:-1], FILTER)
    assert obs_qc(ctx, d["gt"], d["yo"].clone(), d["H"].clone(), d["interp"], d["thr"], FILTER, counts=False) is None


# ---------------------------------------------------------------------------------------------------------------
# the provider

def test_real_obs_unfiltered_equals_synthetic_real_obs(ctx):
    """RealObs(obs_type='real_simu_nofiltering') returns what SyntheticRealObs returns on the same truth / H / R."""
    from vaevar.cycle import RealObs, SyntheticRealObs
    from vaevar.problem import ObsInterpolater, make_problem

    c = _case(("33x47", "r40", 3, 0.02))
    interp = ObsInterpolater(13, 40).interp
    gts = c["gt"].numpy()
    truth = lambda t: gts[int((t - T0).total_seconds() // 3600)]  # noqa: E731
    H = c["H"].numpy()
    R = make_problem(nch=69, Hs=33, Ws=47, T=3, seed=31)["R"]
    syn = SyntheticRealObs(ctx, truth, H, R, interp, da_win=3)
    junk = np.full(H.shape, 1e30, np.float32)  # the simulated types never read the reader's yo
    real = RealObs(ctx, truth, lambda t: (junk, H), R, interp, "real_simu_nofiltering", filter_coeff=0.1, da_win=3)
    a, b = syn.get_obs_info(T0), real.get_obs_info(T0)
    for k, x, y in zip(("yo", "H", "R", "gt"), a, b):
        check_bitwise(f"RealObs real_simu_nofiltering {k} vs SyntheticRealObs", y, x)
    assert real.counts.shape == (3, 2) and (real.counts[:, 0] == real.counts[:, 1]).all()
    check_bitwise("RealObs counts vs sum H", real.counts[:, 0], c["H"].double().sum((1, 2, 3)))
    assert real.counts[1, 0] == 0 and (junk == 1e30).all() and np.array_equal(H, c["H"].numpy())


def _truth4(t):
    from vaevar import config as C
    from vaevar.synth import smooth_field

    k = int((t - T0).total_seconds() // 3600)
    mean = np.asarray(C.MODEL_MEAN[:4], np.float32)[:, None, None]
    std = np.asarray(C.MODEL_STD[:4], np.float32)[:, None, None]
    return (mean + std * smooth_field(5300 + k, (4, 32, 64), sigma=3.0)).astype(np.float32)


class _Handed:
    """A provider that hands over fields computed elsewhere, per cycle time."""

    def __init__(self, items):
        self.items = items

    def get_obs_info(self, t):
        return self.items[t]


def test_real_obs_filtered_cycle(tmp_path, ctx):
    """RealObs(obs_type='real_simu', filter_coeff=0.1) through two cycles of CyclicDA (tiny networks, the identity
    operator, use_eval on) against a provider that hands over the restatement's (yo, H): the reader plants outliers,
    which the filter removes. With the identity operator yo' = gt * H' is one fp32 product, the same on both sides, so
    the analyses are compared bit for bit; were yo' not bitwise equal the bound would be 1e-6 max|xa|."""
    from vaevar import config as C
    from vaevar.cycle import CyclicDA, RealObs
    from vaevar.engine import LGUnet
    from vaevar.problem import obs_variance, qc_threshold
    from vaevar.synth import smooth_field, splitmix_uniform

    std = np.asarray(C.MODEL_STD[:4], np.float32)
    thr = qc_threshold(0.1, None, C.MODEL_STD[:4])
    R = np.broadcast_to(obs_variance(4, 0.005, 2, std)[None, :, None, None], (1, 4, 32, 64)).astype(np.float32).copy()
    xb0 = (_truth4(T0) + 0.1 * std[:, None, None] * smooth_field(5378, (4, 32, 64), sigma=3.0)).astype(np.float32)
    mask_eval = (splitmix_uniform(5379, 32 * 64).reshape(32, 64) < 0.3).astype(np.float32)

    def reader(t):
        k = int((t - T0).total_seconds() // 3600)
        u = splitmix_uniform(5400 + k, 3 * 4 * 32 * 64).reshape(3, 1, 4, 32, 64)
        H = (u[0] < 0.1).astype(np.float32)
        dep = np.where(u[1] < 0.25, 1.5 + u[2], 0.8 * (2 * u[2] - 1))  # a quarter of the stations are outliers
        yo = _truth4(t)[None] + (dep * thr.numpy()[None, :, None, None]).astype(np.float32)
        return yo.astype(np.float32), H

    dec = LGUnet(C.TINY, 1, 1).load_synthetic()
    fc = LGUnet(C.TINY_FLOW, 1, 1).load_synthetic()
    end = T0 + 2 * H6
    kw = dict(Nit=1, decoder=dec, out_dir=str(tmp_path), xb0=xb0, use_eval=True, mask_eval=mask_eval)

    real = RealObs(dec.ctx, _truth4, reader, R, None, "real_simu", filter_coeff=0.1, std=C.MODEL_STD[:4])
    counts = []
    cyc = CyclicDA(fc, real, T0, end, name="real", **kw)
    xas = []

    def log(t, res):
        xas.append(res["xa"].clone())
        counts.append(real.counts.copy())

    cyc.run_assimilation(log=log)
    assert len(xas) == 2

    handed, same = {}, True
    for k in range(2):
        t = T0 + k * H6
        yo, H = (torch.from_numpy(a) for a in reader(t))
        gt = torch.from_numpy(_truth4(t)[None])
        yo_r, H_r, cnt_r = obs_qc_ref(gt, yo, H, None, thr, FILTER | YO_SIMU)
        handed[t] = (yo_r.numpy(), H_r.numpy(), R, gt.numpy())
        check_bitwise(f"cycle {k} RealObs counts vs restatement", counts[k], cnt_r)
        assert counts[k][0, 1] < counts[k][0, 0]
        y_d, H_d, _, _ = real.get_obs_info(t)
        check_bitwise(f"cycle {k} RealObs H' vs restatement", H_d, H_r)
        same = same and torch.equal(y_d.cpu(), yo_r)
    cyc_r = CyclicDA(fc, _Handed(handed), T0, end, name="handed", **kw)
    xas_r = []
    cyc_r.run_assimilation(log=lambda t, res: xas_r.append(res["xa"].clone()))
    for k in range(2):
        if same:
            check_bitwise(f"cycle {k} xa, RealObs vs the restatement's (yo, H)", xas[k], xas_r[k])
        else:
            check(f"cycle {k} xa, RealObs vs the restatement's (yo, H)",
                  (xas[k] - xas_r[k]).abs().max() / xas_r[k].abs().max(), 1e-6, "<=")
    for key in ("bg_wrmse", "ana_wrmse", "bg_bias", "ana_bias", "error_obs"):
        a, b = np.asarray(cyc.metrics_list[key]), np.asarray(cyc_r.metrics_list[key])
        assert a.shape[0] == 2
        if same:
            check_bitwise(f"metric {key}, RealObs vs the restatement's (yo, H)", a, b)
        else:
            check(f"metric {key}, RealObs vs the restatement's (yo, H)", np.abs(a - b).max() / np.abs(b).max(), 1e-6,
                  "<=")
