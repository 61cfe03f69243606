"""Shared by the held-out verification tests: the torch CPU restatement of the reference's error_obs
(da_4dvar.py:1271-1286 = :1140-1155) in fp32 and, on the same fp32 inputs, in float64; the free_run MSE (:948); the
tolerance rule of both; and seeded inputs."""
import numpy as np
import torch
import torch.nn.functional as F

from conftest import check, note


def x_aug_ref(x: torch.Tensor, interp):
    """xhat_aug of :1271-1281 for x (C,H,W): F.linear over the level axis of each of the five variables. The
    reference moves the level axis last with transpose(1, 3); permute(0, 2, 3, 1) does so without swapping H and W,
    which gives the same values bit for bit and copies three times faster at 721 x 1440."""
    if interp is None:
        return x
    nlev = interp.shape[1]
    x0 = x.unsqueeze(0)
    parts = [x0[:, :4]]
    for i in range(5):
        mat = x0[:, 4 + i * nlev:4 + (i + 1) * nlev]
        parts.append(F.linear(mat.permute(0, 2, 3, 1), interp).permute(0, 3, 1, 2))
    return torch.cat(parts, 1).squeeze(0)


def error_obs_ref(x, yo, H, mask, interp, dtype=torch.float32, chunk: int = 0):
    """(error_obs, num, den) of :1286 in `dtype`; x (C,H,W), yo / H (C_obs,H,W), mask (H,W) as CPU tensors or arrays.
    chunk > 0 evaluates that many observation channels at a time (the same values, bounded memory)."""
    x, yo, H, mask = (torch.as_tensor(np.asarray(t)) if not isinstance(t, torch.Tensor) else t.cpu()
                      for t in (x, yo, H, mask))
    it = None if interp is None else torch.as_tensor(np.asarray(interp)).to(dtype)
    xa = x_aug_ref(x.to(dtype), it)
    m = mask.to(dtype)
    nums, dens = [], []
    step = chunk or xa.shape[0]
    for c in range(0, xa.shape[0], step):
        h = H[c:c + step].to(dtype)
        nums.append(torch.sum((xa[c:c + step] - yo[c:c + step].to(dtype)) ** 2 * m * h, (1, 2)))
        dens.append(torch.sum(m * h, (1, 2)))
    num, den = torch.cat(nums), torch.cat(dens)
    return torch.sqrt(num / den).numpy(), num.numpy(), den.numpy()


def check_error_obs(tag: str, hip, x, yo, H, mask, interp, nan_channels=None, chunk: int = 0):
    """The tests' tolerance rule: on the finite channels e_hip = max |hip - ref64| / ref64 <= max(4 e_ref, 5e-7),
    e_ref the fp32 restatement's own distance to float64; the NaN sets of kernel and restatement are identical (and
    equal nan_channels when given)."""
    r32 = error_obs_ref(x, yo, H, mask, interp, torch.float32, chunk)[0]
    r64 = error_obs_ref(x, yo, H, mask, interp, torch.float64, chunk)[0]
    hip = np.asarray(hip.detach().cpu().numpy() if isinstance(hip, torch.Tensor) else hip)
    assert hip.dtype == np.float32 and hip.shape == r32.shape, (hip.dtype, hip.shape, r32.shape)
    nan_ref = np.flatnonzero(np.isnan(r32))
    if nan_channels is not None:
        assert list(nan_ref) == list(nan_channels) and list(np.flatnonzero(np.isnan(r64))) == list(nan_channels)
    check(f"{tag} NaN set differs from the restatement's", np.count_nonzero(np.isnan(hip) != np.isnan(r32)), 0, "==")
    fin = np.isfinite(r64)
    assert fin.sum() == r64.size - nan_ref.size and (r64[fin] > 0).all()
    e_ref = float(np.max(np.abs(r32[fin].astype(np.float64) - r64[fin]) / r64[fin]))
    e_hip = float(np.max(np.abs(hip[fin].astype(np.float64) - r64[fin]) / r64[fin]))
    print(f"{tag}: e_hip {e_hip:.2e}, e_ref {e_ref:.2e}, bound {max(4 * e_ref, 5e-7):.2e}")
    note(f"{tag} e_ref", e_ref)
    check(f"{tag} e_hip", e_hip, max(4 * e_ref, 5e-7), "<=")


def mse_ref(xb, gt, mean, std, dtype):
    """MSE_bg of the free_run branch (:944-948) in `dtype` on fp32 inputs."""
    xb, gt, mean, std = (torch.as_tensor(np.asarray(t, np.float32)).to(dtype) for t in (xb, gt, mean, std))
    gn = (gt - mean.reshape(-1, 1, 1)) / std.reshape(-1, 1, 1)
    xn = (xb - mean.reshape(-1, 1, 1)) / std.reshape(-1, 1, 1)
    return torch.mean((xn - gn) ** 2).item()


def uniform_planes(seed: int, C: int, Hs: int, Ws: int) -> torch.Tensor:
    """(C, Hs, Ws) values in [0,1): 8 splitmix_uniform planes, channel c taking plane c % 8 (mirrored about 0.5
    for odd c // 8). Cheap at 204 x 721 x 1440, where one draw per element would dominate the test."""
    from vaevar.synth import splitmix_uniform

    u = torch.from_numpy(splitmix_uniform(seed, 8 * Hs * Ws).reshape(8, Hs, Ws))
    c = torch.arange(C)
    out = u[c % 8]
    odd = (c // 8) % 2 == 1
    out[odd] = 1 - out[odd]
    return out


def make_case(Hs, Ws, n_in=13, n_out=40, C=69, seed=4100, frac=0.3, zero_channel=None, planes=False):
    """x = mean + std * field; yo = x_aug(x) + 1e-2 |x_aug| noise (bounds the cancellation in x_aug - yo); H and
    mask from splitmix_uniform at `frac` each; observation channel zero_channel of H zeroed. n_out = 0: identity."""
    from vaevar import config as Cf
    from vaevar.problem import ObsInterpolater
    from vaevar.synth import smooth_field, splitmix_uniform

    HW = Hs * Ws
    mean = torch.tensor(Cf.MODEL_MEAN[:C], dtype=torch.float32).reshape(-1, 1, 1)
    std = torch.tensor(Cf.MODEL_STD[:C], dtype=torch.float32).reshape(-1, 1, 1)
    if planes:
        s = (uniform_planes(seed, C, Hs, Ws) * 2 - 1) * 1.7
    else:
        s = torch.from_numpy(smooth_field(seed, (C, Hs, Ws), sigma=2.0))
    x = mean + std * s
    interp = ObsInterpolater(n_in, n_out).interp if n_out else None
    xa = x_aug_ref(x, None if interp is None else torch.from_numpy(interp))
    ca = xa.shape[0]
    if planes:
        noise = uniform_planes(seed + 1, ca, Hs, Ws) * 2 - 1
        H = (uniform_planes(seed + 2, ca, Hs, Ws) < frac).float()
    else:
        noise = torch.from_numpy(splitmix_uniform(seed + 1, ca * HW).reshape(ca, Hs, Ws)) * 2 - 1
        H = (torch.from_numpy(splitmix_uniform(seed + 2, ca * HW).reshape(ca, Hs, Ws)) < frac).float()
    yo = xa + 1e-2 * xa.abs() * noise
    mask = (splitmix_uniform(seed + 3, HW).reshape(Hs, Ws) < frac).astype(np.float32)
    if zero_channel is not None:
        H[zero_channel] = 0
    return {"x": x.numpy(), "yo": yo.numpy(), "H": H.numpy(), "mask": mask, "interp": interp, "zero": zero_channel}
