"""Shared by the real-observation quality-control tests: the torch CPU restatement of get_obs_info's departure filter
(da_4dvar.py:770-798) with the five obs_type branches expressed as the VV_QC_* flag bits, the device composition of
the same steps from the existing pieces (vv_obs_augment + torch element-wise ops), and seeded cases with a guard band
around the threshold, so that the accept / reject decision of every element is compared exactly."""
import numpy as np
import torch
import torch.nn.functional as F

FILTER, EXEMPT_Z, YO_SIMU, YO_SIMU_Z = 1, 2, 4, 8
FLAG_SETS = {"real_simu_nofilteringz": FILTER | EXEMPT_Z | YO_SIMU, "real_simuz": FILTER | EXEMPT_Z | YO_SIMU_Z,
             "real_simu_nofiltering": YO_SIMU, "real_simu": FILTER | YO_SIMU, "real": FILTER, "none": 0}


def gt_aug_ref(gt: torch.Tensor, interp):
    """gt_aug of :770-776 for gt (T,C,H,W): F.linear over the level axis of each of the five variables (permute
    instead of the reference's transpose(1, 3): the same values, see _obs_error_ref.x_aug_ref)."""
    if interp is None:
        return gt
    interp = torch.as_tensor(np.asarray(interp)).to(gt.dtype)
    nlev = interp.shape[1]
    parts = [gt[:, :4]]
    for i in range(5):
        mat = gt[:, 4 + i * nlev:4 + (i + 1) * nlev]
        parts.append(F.linear(mat.permute(0, 2, 3, 1), interp).permute(0, 3, 1, 2))
    return torch.cat(parts, 1)


def simu_channels(flags: int, c_obs: int, n_out: int) -> np.ndarray:
    """Boolean (c_obs,): the channels whose yo the flags replace (:795-798)."""
    s = np.zeros(c_obs, bool)
    if flags & YO_SIMU_Z:
        s[4:4 + n_out] = True
    elif flags & YO_SIMU:
        s[:] = True
    return s


def obs_qc_ref(gt, yo, H, interp, thr, flags: int):
    """(yo', H', counts) of :766-798 on CPU fp32 tensors gt (T,C,H,W), yo / H (T,C_obs,H,W), thr (C_obs,) =
    filter_coeff * torch.Tensor(std_layer_aug). The z block 4:44 of the reference (:782, :796) is 4:4+n_out. counts
    (T,2) float64: the amounts printed before (:768) and after (:793) the filter."""
    n_out = 0 if interp is None else np.asarray(interp).shape[0]
    gt_aug = gt_aug_ref(gt, interp)
    before = H.double().sum((1, 2, 3))
    if flags & FILTER:  # :779-781 / :786-788
        t = thr.reshape(1, -1, 1, 1)
        mask1 = ((yo - gt_aug) < t) * 1
        mask2 = ((yo - gt_aug) > -t) * 1
        mask = mask1 * mask2
        if flags & EXEMPT_Z:
            mask[:, 4:4 + n_out] = 1  # :782
    else:
        mask = torch.zeros(yo.shape) + 1  # :784
    Hn = H * mask  # :790
    after = Hn.double().sum((1, 2, 3))
    if flags & YO_SIMU_Z:  # :795-796
        yo = yo.clone()
        yo[:, 4:4 + n_out] = gt_aug[:, 4:4 + n_out] * Hn[:, 4:4 + n_out]
    elif flags & YO_SIMU:  # :797-798
        yo = gt_aug * Hn
    return yo, Hn, torch.stack([before, after], 1)


def obs_qc_composed(ctx, gt, yo, H, interp, thr, flags: int):
    """The same steps on the device from the existing pieces: obs_augment (k_obs_augment) and torch element-wise ops;
    nothing in place. Returns (yo', H', counts)."""
    from vaevar.engine import obs_augment

    n_out = 0 if interp is None else interp.shape[0]
    gt_aug = gt if interp is None else obs_augment(ctx, interp, gt)
    before = H.double().sum((1, 2, 3))
    if flags & FILTER:
        t = thr.reshape(1, -1, 1, 1)
        d = yo - gt_aug
        mask = ((d < t) & (d > -t)).float()
        if flags & EXEMPT_Z:
            mask[:, 4:4 + n_out] = 1
    else:
        mask = torch.ones_like(yo)
    Hn = H * mask
    after = Hn.double().sum((1, 2, 3))
    if flags & YO_SIMU_Z:
        yo = yo.clone()
        yo[:, 4:4 + n_out] = gt_aug[:, 4:4 + n_out] * Hn[:, 4:4 + n_out]
    elif flags & YO_SIMU:
        yo = gt_aug * Hn
    return yo, Hn, torch.stack([before, after], 1)


def make_case(Hs, Ws, T=1, n_out=40, seed=5100, density=0.02, coeff=0.1, zero_slice=None):
    """gt = mean_c + std_c * N(0,1) (69 channels); station H at `density` per (t, channel, pixel), a fifth of the
    stations 0.5; yo = gt_aug_ref + u * thr with |u| drawn from [0, 0.9] U [1.1, 3] and a random sign: no departure
    within 10 % of its threshold, while the fp32 and fp64 gt_aug differ by ~1e-7 of |gt_aug| << 0.1 thr, so the decision
    of every element is the same in any correctly rounded evaluation. n_out = 0: the identity operator. zero_slice: a
    time index whose H is all zero."""
    from vaevar import config as Cf
    from vaevar.problem import ObsInterpolater, qc_threshold

    g = torch.Generator().manual_seed(seed)
    mean = torch.tensor(Cf.MODEL_MEAN, dtype=torch.float32).reshape(1, -1, 1, 1)
    std = torch.tensor(Cf.MODEL_STD, dtype=torch.float32).reshape(1, -1, 1, 1)
    gt = mean + std * torch.randn(T, 69, Hs, Ws, generator=g)
    interp = ObsInterpolater(13, n_out).interp if n_out else None
    thr = qc_threshold(coeff, interp, Cf.MODEL_STD)
    ga = gt_aug_ref(gt, interp)
    shape = ga.shape
    st = torch.rand(shape, generator=g) < density
    H = st.float() * torch.where(torch.rand(shape, generator=g) < 0.2, 0.5, 1.0)
    if zero_slice is not None:
        H[zero_slice] = 0
    r = torch.rand(shape, generator=g)
    u = torch.where(r < 0.5, 1.8 * r, 1.1 + 3.8 * (r - 0.5))  # [0, 0.9) or [1.1, 3.0)
    u = u * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    yo = ga + u * thr.reshape(1, -1, 1, 1)
    return {"gt": gt, "yo": yo, "H": H, "interp": interp, "thr": thr, "n_out": n_out}
