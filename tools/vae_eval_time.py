"""vv_vae_sample, vv_vae_sse and vv_err_sample timing (development tool): the median of VV_VAE_REPS
(default 25, at least 20) event-timed calls after warm-up, buffers allocated once, at the full configuration
(config.VAE: 69 x 128 x 256 state, 32 latent channels) for B = 1 and B = 4.

Per batch size: the sample kernel with z and stat, z alone, stat alone and the posterior mean; the sse kernel; the error
sample on the model grid (pred the flow network's (B, 138, H, W) output) and, at B = 1, from a 721 x 1440 state; then the
encoder and decoder forwards and one whole calib.VAEStats.add, so that the kernels stand next to the call they sit in.
Bytes are the fields each kernel reads and writes once. No threshold is asserted. Writes $VV_OUT/vae_eval.json (default
profiles/r12/)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-var_amd"))
import numpy as np
import torch

from vaevar import config as Cf
from vaevar._lib import lib
from vaevar.calib import VAEStats
from vaevar.engine import Context, err_sample, vae_sample, vae_sse
from vaevar.vae import VAE_lr

REPS = max(20, int(os.environ.get("VV_VAE_REPS", 25)))
ctx = Context.get(0)


def events(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def with_rate(r, nbytes):
    r["bytes"] = int(nbytes)
    r["GBps"] = nbytes / r["ms_median"] * 1e-6
    return r


out = {"device": torch.cuda.get_device_name(0), "lib_version": lib.vv_version(), "repeats": REPS, "batches": {}}
C, L, H, W = 69, 32, 128, 256
sd = torch.tensor(Cf.STD_TR, dtype=torch.float32).cuda()
g = torch.Generator().manual_seed(5)

for B in (1, 4):
    vae = VAE_lr(Cf.VAE, B, ctx=ctx).load_synthetic()
    x = torch.randn((B, C, H, W), generator=g).cuda()
    enc = vae.encode(x)
    z = torch.empty(B, L, H, W, device="cuda")
    stat = torch.empty(B, L, 4, device="cuda", dtype=torch.float64)
    recon = vae.dec.forward_raw(vae_sample(ctx, enc, 1, 2, z=z)[0])
    sse = torch.empty(B, C, device="cuda", dtype=torch.float64)
    pred = torch.randn((B, 138, H, W), generator=g).cuda()
    eout = torch.empty(B, C, H, W, device="cuda")
    nz, nx = B * L * H * W, B * C * H * W
    r = {"shape": {"B": B, "C": C, "L": L, "H": H, "W": W}}
    r["sample_z_stat"] = with_rate(events(lambda: vae_sample(ctx, enc, 1, 2, z=z, stat=stat)), 12 * nz)
    r["sample_z"] = with_rate(events(lambda: vae_sample(ctx, enc, 1, 2, z=z)), 12 * nz)
    r["sample_stat"] = with_rate(events(lambda: vae_sample(ctx, enc, stat=stat, want_z=False)), 8 * nz)
    r["sample_mean"] = with_rate(events(lambda: vae_sample(ctx, enc, mean=True, z=z)), 12 * nz)
    r["sse"] = with_rate(events(lambda: vae_sse(ctx, recon, x, out=sse)), 8 * nx)
    r["err_sample_identity"] = with_rate(events(lambda: err_sample(ctx, pred, x, sd, out=eout, C=C)), 12 * nx)
    r["encoder_forward"] = events(lambda: vae.encode(x, out=enc))
    r["decoder_forward"] = events(lambda: vae.dec.forward_raw(z, out=recon))
    st = VAEStats(vae, 2.0)
    r["vae_stats_add"] = events(lambda: st.add(x, 1, 2))
    kernels = r["sample_z_stat"]["ms_median"] + r["sample_mean"]["ms_median"] + 2 * r["sse"]["ms_median"]
    r["kernels_fraction_of_add"] = kernels / r["vae_stats_add"]["ms_median"]
    r["sample_fraction_of_add"] = r["sample_z_stat"]["ms_median"] / r["vae_stats_add"]["ms_median"]
    out["batches"][f"B{B}"] = r
    print(f"B={B}", r, flush=True)
    del vae, st, enc, recon, pred

# the reference's own resampling: a 0.25 degree state to the network grid
p721, t721 = (torch.randn((1, C, 721, 1440), generator=g).cuda() for _ in range(2))
e721 = torch.empty(1, C, H, W, device="cuda")
out["err_sample_721x1440_to_128x256"] = with_rate(
    events(lambda: err_sample(ctx, p721, t721, sd, (H, W), out=e721)), 12 * C * H * W)
print("err_sample 721x1440 -> 128x256", out["err_sample_721x1440_to_128x256"], flush=True)

out_dir = os.environ.get("VV_OUT", os.path.join(ROOT, "profiles", "r12"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "vae_eval.json"), "w") as f:
    json.dump(out, f, indent=1)
