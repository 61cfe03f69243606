"""Shared by the forecast-verification tests: the project's torch CPU restatement of the statistics vv_verify
returns (include/vaevar.h), written from their definitions; the seeded inputs of the golden cases
(tests/golden/g19_verify.npz, tools/make_verify_fixture.py); and the tests' error measure."""
import numpy as np
import torch

NAMES = ("WRMSE", "NWRMSE", "SWRMSE", "TWRMSE", "Bias", "NBias", "SBias", "TBias", "Channel_MSE", "MSE", "MAE",
         "Activity", "NActivity", "SActivity", "TActivity", "Anomaly", "NAnomaly", "SAnomaly", "TAnomaly",
         "WACC", "NWACC", "SWACC", "TWACC")
ERROR_NAMES, CLIM_NAMES = NAMES[:11], NAMES[11:]

# (B, C, H, W), seed: the smallest valid height on the scalar path with W below a wave; si = 14 / ni = 23 with W % 4
# != 0 and B > 1; the float4 path with a region boundary inside what would else be one chunk; the workload plane
CASES = {"h5": ((1, 1, 5, 3), 1901), "h37_w18": ((2, 3, 37, 18), 1902), "h37_w20": ((1, 2, 37, 20), 1903),
         "workload": ((1, 5, 721, 1440), 1904)}
STORED_INPUTS = ("h5", "h37_w18", "h37_w20")  # the workload case's inputs are regenerated from its seed


def region_bounds(H: int):
    return int(70. / 180. * H + 0.5), int(110. / 180. * H + 0.5)


def row_sets(H: int):
    """{prefix: (lo, hi, fp32 weights of rows lo..hi)}: '' every row, S rows [0, si), T [si, ni), N [ni, H). The
    factor of N is si, not its own row count."""
    si, ni = region_bounds(H)
    j = torch.arange(H)
    lat = 90. - j * 180. / float(H - 1)  # fp32: an integer tensor times a Python float
    c = torch.cos(3.1416 / 180. * lat)
    out = {}
    for pre, lo, hi, k in (("", 0, H, H), ("N", ni, H, si), ("S", 0, si, si), ("T", si, ni, ni - si)):
        cs = c[lo:hi]
        out[pre] = (lo, hi, k * cs / torch.sum(cs))
    return out


def normalise(x, mean, std):
    """(x - mean) / std in fp32, the channel axis third from last."""
    x = torch.as_tensor(np.asarray(x, np.float32))
    m = torch.as_tensor(np.asarray(mean, np.float32)).reshape(-1, 1, 1)
    s = torch.as_tensor(np.asarray(std, np.float32)).reshape(-1, 1, 1)
    return (x - m) / s


def verify_ref(pred, gt, clim, mean, std, scale, dtype=torch.float32):
    """{name: (C,) float64 array}. pred, gt (B,C,H,W), clim (C,H,W) or None, physical; normalised in fp32, then every
    statistic in `dtype` with the fp32 weights (as a float64 run of the reference has them)."""
    p, t = normalise(pred, mean, std).to(dtype), normalise(gt, mean, std).to(dtype)
    c = None if clim is None else normalise(clim, mean, std).to(dtype)
    sc = torch.as_tensor(np.asarray(scale, np.float64))
    B, C, H, W = p.shape
    hw = (-1, -2)
    out = {}
    d = p - t
    out["Channel_MSE"] = torch.mean(d ** 2, (0, 2, 3)).double()
    out["MSE"] = torch.mean(d ** 2).double().expand(C)
    out["MAE"] = torch.mean(torch.abs(d)).double().expand(C)
    for pre, (lo, hi, w) in row_sets(H).items():
        w = w.reshape(1, 1, -1, 1)
        ds = d[:, :, lo:hi]
        out[pre + "WRMSE"] = torch.mean(torch.sqrt(torch.mean(w * ds ** 2, hw)), 0) * sc
        out[pre + "Bias"] = torch.mean(torch.mean(w * ds, hw), 0) * sc
        if c is None:
            continue
        a, b = (p - c)[:, :, lo:hi], (t - c)[:, :, lo:hi]
        ac = a - torch.mean(w * a, hw, keepdim=True)
        bc = b - torch.mean(w * b, hw, keepdim=True)
        sa, sb = torch.sqrt(torch.mean(w * ac ** 2, hw)), torch.sqrt(torch.mean(w * bc ** 2, hw))
        out[pre + "Activity"] = torch.mean(sa, 0) * sc
        # the numerator is ONE mean over batch, channels and the slice (the reference's mean without a dim)
        out[pre + "Anomaly"] = torch.mean(torch.mean(w * ac * bc) / (sa * sb), 0).double()
        out[pre + "WACC"] = torch.mean(torch.sum(w * a * b, hw) / torch.sqrt(torch.sum(w * a * a, hw) *
                                                                            torch.sum(w * b * b, hw)), 0).double()
    return {k: np.asarray(v.numpy(), np.float64).copy() for k, v in out.items()}


def make_case(name: str):
    """Seeded inputs of a golden case: normalised truth uniform in +-1.7, forecast = truth + 0.3 of such a field,
    climatology 0.5 of one plus 0.2, mapped to physical values by a per-channel mean and std."""
    from vaevar.synth import splitmix_uniform

    (B, C, H, W), seed = CASES[name]

    def field(k, *shape):
        return (splitmix_uniform(seed + k, int(np.prod(shape))).reshape(shape) * 2 - 1) * np.float32(1.7)

    mean = (np.float32(250.0) + np.float32(40.0) * np.arange(C, dtype=np.float32)).reshape(C, 1, 1)
    std = (np.float32(3.0) + np.float32(1.5) * np.arange(C, dtype=np.float32)).reshape(C, 1, 1)
    gtn = field(0, B, C, H, W)
    gt = mean + std * gtn
    pred = mean + std * (gtn + np.float32(0.3) * field(1, B, C, H, W))
    clim = mean + std * (np.float32(0.5) * field(2, C, H, W) + np.float32(0.2))
    return {"pred": pred.astype(np.float32), "gt": gt.astype(np.float32), "clim": clim.astype(np.float32),
            "mean": mean.reshape(C), "std": std.reshape(C), "scale": std.reshape(C).astype(np.float64) * 1.0009765625}


def rel_err(got, want):
    """max_c |got - want| / max_c |want|: the error against the statistic's largest magnitude over channels."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
