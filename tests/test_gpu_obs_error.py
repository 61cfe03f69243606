"""vv_obs_error / Metrics.obs_error (the held-out observation verification of --use_eval, da_4dvar.py:1271-1286) on the
GPU against the torch CPU restatement of those lines (tests/_obs_error_ref.py), in fp32 and in float64 on the same
inputs. Tolerance on the finite channels: e_hip <= max(4 e_ref, 5e-7), e_ref being the fp32 restatement's own
distance to float64 (the factor 4 allows another contraction of the 13-term dot product under the cancellation of
x_aug - yo; the floor is the G9 WRMSE bound for the same kind of reduction, about 4 ulp for the two casts, the
division and the square root). Everything else is bitwise: determinism, the in-register operator against
k_obs_augment, the pixel skip, the denominator sums.

Grids: 33 x 47 = 1551 pixels (no multiple of 256, 64 or 4: a ragged last 64-pixel segment), 1 x 300, 67 x 131 = 8777
(three 4096-pixel chunks, the last ragged, and more listed pixels than one pass of the four waves takes), and the
workload's 204 x 721 x 1440."""
import numpy as np
import pytest
import torch

from _obs_error_ref import check_error_obs, make_case
from conftest import check, check_bitwise

pytestmark = pytest.mark.gpu

#        tag       Hs  Ws   n_out C   zeroed observation channel
CASES = {"r40": (33, 47, 40, 69, 4 + 40 * 2 + 3),
         "r7": (33, 47, 7, 69, 4 + 7 * 4 + 6),
         "id69": (33, 47, 0, 69, 17),
         "row300": (1, 300, 40, 69, 2),
         "c3": (67, 131, 40, 69, 4 + 40 * 3 + 39)}


@pytest.fixture(scope="module")
def metric():
    from vaevar.engine import Context
    from vaevar.metrics import Metrics

    return Metrics(Context.get(0))


@pytest.fixture(scope="module")
def cases():
    out = {}
    for k, (Hs, Ws, n_out, C, z) in CASES.items():
        out[k] = make_case(Hs, Ws, 13, n_out, C, seed=4100 + 10 * len(out), zero_channel=z)
    return out


def _dev(c):
    d = {k: torch.from_numpy(c[k]).cuda() for k in ("x", "yo", "H", "mask")}
    d["interp"] = None if c["interp"] is None else torch.from_numpy(c["interp"]).cuda()
    return d


def _run(metric, d, **over):
    a = dict(d, **over)
    err, sums = metric.obs_error(a["x"], a["yo"], a["H"], a["mask"], a["interp"], return_sums=True)
    return err.cpu(), sums.cpu()


@pytest.mark.parametrize("tag", list(CASES))
def test_obs_error_vs_restatement(metric, cases, tag):
    c = cases[tag]
    d = _dev(c)
    err, sums = _run(metric, d)
    assert err.dtype == torch.float32 and err.shape == (c["yo"].shape[0],)
    # exactly one NaN channel in the reference, the zeroed one (0/0), and the same set from the kernel
    check_error_obs(tag, err, c["x"], c["yo"], c["H"], c["mask"], c["interp"], nan_channels=[c["zero"]])
    # the denominator is a sum of 0/1 products: exact
    den = (torch.from_numpy(c["mask"]).double() * torch.from_numpy(c["H"]).double()).sum((1, 2))
    check_bitwise(f"{tag} sums[2c+1] vs float64 sum(mask H)", sums[:, 1], den)
    # err is the fp32 quotient and root of the two sums: two casts (1/2 ulp each) and a division (<= 1 ulp), halved by
    # the root, plus the root (<= 1 ulp) and fp32's spacing against the float64 value: within 4 ulp = 4 * 2^-24
    fin = den > 0
    q = torch.sqrt(sums[fin, 0] / sums[fin, 1])
    check(f"{tag} err vs sqrt(num / den) of the returned sums", ((err[fin].double() - q).abs() / q).max(), 4 * 2.0 ** -24,
          "<=")
    assert torch.isnan(err[~fin]).all()
    # determinism: no atomics, fixed order
    err2, sums2 = _run(metric, d)
    check_bitwise(f"{tag} second call err", err2, err)
    check_bitwise(f"{tag} second call sums", sums2, sums)


@pytest.mark.parametrize("tag", ["r40", "r7", "row300", "c3"])
def test_obs_error_operator_equals_obs_augment(metric, cases, tag):
    """obs_error(x, interp) == obs_error(obs_augment(x), identity) bit for bit: the operator applied in registers is
    k_obs_augment's, and a channel's sums do not depend on how the channels are grouped over the grid."""
    from vaevar.engine import obs_augment

    d = _dev(cases[tag])
    err, sums = _run(metric, d)
    xa = obs_augment(metric.ctx, d["interp"], d["x"][None])[0]
    err_i, sums_i = _run(metric, d, x=xa, interp=None)
    check_bitwise(f"{tag} err operator vs augmented identity", err, err_i)
    check_bitwise(f"{tag} sums operator vs augmented identity", sums, sums_i)


@pytest.mark.parametrize("tag", ["r40", "id69", "c3"])
def test_obs_error_pixel_skip_is_exact(metric, cases, tag):
    """Large finite x, yo and H at the pixels with mask == 0 change neither err nor sums by a bit."""
    c = cases[tag]
    d = _dev(c)
    err, sums = _run(metric, d)
    off = d["mask"] == 0
    assert 0 < int(off.sum()) < off.numel()
    big = {k: torch.where(off, torch.full_like(d[k], v), d[k]) for k, v in (("x", 1e6), ("yo", -3e6), ("H", 7e5))}
    err_b, sums_b = _run(metric, d, **big)
    check_bitwise(f"{tag} err with junk at mask == 0", err_b, err)
    check_bitwise(f"{tag} sums with junk at mask == 0", sums_b, sums)


@pytest.mark.parametrize("tag", ["r40", "id69"])
def test_obs_error_non_binary_mask(metric, cases, tag):
    """A mask of values 0, 0.5 and 1 is read, not assumed binary."""
    from vaevar.synth import splitmix_uniform

    c = cases[tag]
    u = splitmix_uniform(991, c["mask"].size).reshape(c["mask"].shape)
    mask = np.where(u < 0.15, 0.5, np.where(u < 0.3, 1.0, 0.0)).astype(np.float32)
    assert set(np.unique(mask)) == {0.0, 0.5, 1.0}
    d = _dev(c)
    err, _ = _run(metric, d, mask=torch.from_numpy(mask).cuda())
    check_error_obs(f"{tag} mask 0/0.5/1", err, c["x"], c["yo"], c["H"], mask, c["interp"], nan_channels=[c["zero"]])


def test_obs_error_workload_shape(metric):
    """204 x 721 x 1440 (13 -> 40 levels), the shape the verification runs at in a real-observation cycle."""
    c = make_case(721, 1440, 13, 40, 69, seed=4700, zero_channel=4 + 40 * 1 + 11, planes=True)
    d = _dev(c)
    err, sums = _run(metric, d)
    check_error_obs("204x721x1440", err, c["x"], c["yo"], c["H"], c["mask"], c["interp"], nan_channels=[c["zero"]],
                    chunk=25)
    err2, sums2 = _run(metric, d)
    check_bitwise("204x721x1440 second call err", err2, err)
    check_bitwise("204x721x1440 second call sums", sums2, sums)


def test_obs_error_profiled_as_misfit(metric, cases):
    """The live profiler books the call under the misfit class with the no-skip algorithmic bytes: the mask, the
    state, yo and H once each."""
    c = cases["r40"]
    d = _dev(c)
    metric.ctx.profile_start()
    metric.obs_error(d["x"], d["yo"], d["H"], d["mask"], d["interp"])
    prof = metric.ctx.profile_stop()
    assert prof["misfit"]["launches"] == 1 and prof["misfit"]["ms"] > 0
    assert sum(v["launches"] for v in prof.values()) == 1
    assert prof["misfit"]["bytes"] == 4.0 * c["mask"].size * (1 + 69 + 2 * 204)


def test_obs_error_python_checks(metric, cases):
    d = _dev(cases["r40"])
    with pytest.raises(ValueError, match="mask_eval"):
        metric.obs_error(d["x"], d["yo"], d["H"], d["mask"][:-1], d["interp"])
    with pytest.raises(ValueError, match="operator expects"):
        metric.obs_error(d["x"][:68], d["yo"], d["H"], d["mask"], d["interp"])
    with pytest.raises(ValueError, match="yo / H"):
        metric.obs_error(d["x"], d["yo"], d["H"], d["mask"], None)
