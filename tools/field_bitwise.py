"""Dev tool: run the chunk-layout field operations (err_accum, err_finalize, r_fill, vae_sample, vae_sse, err_sample)
on seeded inputs with the library named by VAEVAR_LIB and save every output, to compare two builds bit for bit:

  VAEVAR_LIB=old.so python tools/field_bitwise.py old.npz
  VAEVAR_LIB=new.so python tools/field_bitwise.py new.npz old.npz     prints `bitwise` or the differing words per output

Shapes (the tests'): an odd 5 x 7 plane, a 16-byte-path 32 x 64 plane, the two-chunk planes 72 x 96 (16-byte path) and
67 x 71 (element path with a tail); layouts: contiguous, samples strided inside a 138-channel buffer (B > 1) and a
buffer that starts one element off a 16-byte boundary. Exit status 1 when an output differs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-var_amd"))
from vaevar.engine import (Context, err_accum, err_finalize, err_sample, r_fill, vae_sample,  # noqa: E402
                           vae_sse)

SHAPES = [(1, 3, 5, 7), (2, 4, 32, 64), (2, 2, 72, 96), (3, 2, 67, 71)]
LAYOUTS = ("plain", "strided138", "offset1")
ctx = Context.get(0)
out = {}


def field(seed, shape, scale=3.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def laid_out(t, layout):
    """t (B, C, H, W) on the device in another layout holding the same values"""
    B, C, H, W = t.shape
    if layout == "strided138":
        full = field(99, (B, 138, H, W))
        full[:, :C] = t
        return full[:, :C]
    if layout == "offset1":
        buf = torch.zeros(t.numel() + 1, device="cuda")
        buf[1:] = t.reshape(-1)
        return buf[1:].view(B, C, H, W)
    return t


def keep(name, t):
    a = t.detach().cpu().numpy()
    out[name] = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


for B, C, H, W in SHAPES:
    for layout in LAYOUTS:
        tag = f"{B}x{C}x{H}x{W}_{layout}"
        pred, tgt = laid_out(field(1, (B, C, H, W)), layout), field(2, (B, C, H, W))
        cell = torch.zeros(C, H, W, device="cuda", dtype=torch.float64)
        chan = torch.zeros(C, device="cuda", dtype=torch.float64)
        for _ in range(2):  # the second call accumulates onto the first
            err_accum(ctx, pred, tgt, cell, chan, C=C)
        keep(f"err_accum_cell_{tag}", cell)
        keep(f"err_accum_chan_{tag}", chan)
        chan_only = torch.zeros_like(chan)
        err_accum(ctx, pred, tgt, None, chan_only, C=C)
        keep(f"err_accum_chan_only_{tag}", chan_only)
        keep(f"vae_sse_{tag}", vae_sse(ctx, pred, tgt, C=C))
        std = field(3, (C,), 1.0).abs() + 0.5
        keep(f"err_sample_same_{tag}", err_sample(ctx, pred, tgt, std, C=C))
        keep(f"err_sample_resized_{tag}", err_sample(ctx, pred, tgt, std, size=(H // 2 + 1, 2 * W - 3), C=C))
    tag = f"{B}x{C}x{H}x{W}"
    q_field, q_tab = err_finalize(ctx, cell, 7)
    keep(f"err_finalize_field_{tag}", q_field)
    keep(f"err_finalize_tab_{tag}", q_tab)
    odd = torch.zeros(cell.numel() + 1, device="cuda", dtype=torch.float64)[1:].view(C, H, W)  # 8 bytes off
    keep(f"err_finalize_field_offset_{tag}", err_finalize(ctx, cell, 7, q_field=odd, table=False)[0])
    enc = torch.cat([field(4, (B, C, H, W), 2.0), field(5, (B, C, H, W), 6.0)], 1).contiguous()
    for mean in (False, True):
        stat = torch.zeros(B, C, 4, device="cuda", dtype=torch.float64)
        z, _ = vae_sample(ctx, enc, seed=0x5EEDC0DE12345, draw=3, mean=mean, stat=stat)
        keep(f"vae_sample_z_mean{int(mean)}_{tag}", z)
        keep(f"vae_sample_stat_mean{int(mean)}_{tag}", stat)
    zo = torch.zeros(z.numel() + 1, device="cuda")[1:].view(z.shape)
    keep(f"vae_sample_z_offset_{tag}", vae_sample(ctx, enc, seed=7, draw=1, z=zo)[0])
    rtab = field(6, (B, 69), 1.0).abs()
    interp = field(7, (40, 13), 1.0)
    keep(f"r_fill_identity_{tag}", r_fill(ctx, rtab, H, W))
    keep(f"r_fill_operator_{tag}", r_fill(ctx, rtab, H, W, interp=interp))
    ro = torch.zeros(B * 69 * H * W + 1, device="cuda")[1:].view(B, 69, H, W)
    keep(f"r_fill_offset_{tag}", r_fill(ctx, rtab, H, W, out=ro))

torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print(f"{len(out)} outputs with {os.environ.get('VAEVAR_LIB', 'the default library')} -> {sys.argv[1]}")
if len(sys.argv) > 2:
    ref = np.load(sys.argv[2])
    bad = 0
    for k in sorted(out):
        n = int((out[k] != ref[k]).sum())
        bad += n > 0
        print(k, "bitwise" if n == 0 else f"DIFF in {n} of {out[k].size} words")
    print(f"{len(out) - bad} of {len(out)} outputs bitwise equal")
    sys.exit(1 if bad else 0)
