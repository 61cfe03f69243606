"""Make tests/golden/g20_vae_eval.npz and g21_full_encoder.npz: what the REFERENCE's nf_model.vae.VAE_lr and
loss_function make of synthetic weights and inputs. CPU only; needs the reference tree that oracle.ref_harness imports
(it is not part of this repository).

    python tools/make_vae_eval_fixture.py            # both fixtures (the full encoder takes a minute or two)
    python tools/make_vae_eval_fixture.py --tiny     # g20 only

VAE_lr reads nf_model/<name>.yaml relative to the working directory, so the configuration (config.TINY_VAE, config.VAE)
is written as yaml into a scratch directory and the process changes into it after the reference is imported. Only data
is written.

g20 (B = 1, config.TINY_VAE, weights oracle.lgunet_ref.synth_params under `enc.` / `dec.`):
  x_seed, seed, draw, sigma   the input is smooth_field(x_seed, (1, 17, 32, 64), sigma=2), eps the fp32 rounding of
                              tests/_obs_synth_ref.eps_ref(seed, draw, 0, n)
  enc_out                     vae.enc(x)                                        (1, 16, 32, 64)
  z                           eps.mul(exp(0.5 * log_var)).add_(mu)              vae.py:79-81 with eps given
  recon                       vae.decoder(z)
  loss, rec, kld              loss_function(recon, x, mu, log_var, sigma)       fp32, as the reference returns them
g21 (config.ENCODER on smooth_field(451, (1, 69, 128, 256))), in g3_full_decoder's form: idx_out, out_sample (4096
sampled outputs), out_sum, out_sumsq, out_abssum in fp64.
"""
import argparse
import importlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vae-var_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

X_SEED, SEED, DRAW, SIGMA = 2001, 0x5EEDC0DE12345, 3, 2.0
FULL_X_SEED = 451


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def ref_vae(vmod, params, name, scratch):
    """The reference's VAE_lr built from `params` with synthetic weights; also returns the weights."""
    import torch
    import yaml

    from oracle.lgunet_ref import synth_params

    os.makedirs(os.path.join(scratch, "nf_model"), exist_ok=True)
    with open(os.path.join(scratch, "nf_model", name + ".yaml"), "w") as f:
        yaml.safe_dump({k: dict(v) for k, v in params.items()}, f)
    os.chdir(scratch)
    torch.manual_seed(0)
    m = vmod.VAE_lr(name)
    p = {**synth_params(params["encoder"], "enc."), **synth_params(params["decoder"], "dec.")}
    sd = m.state_dict()
    missing = [k for k in sd if k not in p]
    assert all(k.endswith("relative_position_index") or k.endswith("attn_mask") for k in missing), missing[:5]
    assert not [k for k in p if k not in sd]
    m.load_state_dict(p, strict=False)
    m.eval()
    return m, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="g20 only")
    args = ap.parse_args()

    import torch

    from oracle import ref_harness

    ref_harness.import_reference()
    vmod = importlib.import_module("nf_model.vae")
    from _obs_synth_ref import eps_ref
    from oracle.lgunet_ref import lgunet_forward
    from vaevar import config as C
    from vaevar.synth import smooth_field

    gold = os.path.join(ROOT, "tests", "golden")
    with tempfile.TemporaryDirectory() as scratch, torch.no_grad():
        m, p = ref_vae(vmod, C.TINY_VAE, "tiny_vae", scratch)
        x = torch.from_numpy(smooth_field(X_SEED, (1, 17, 32, 64), sigma=2.0))
        mu, lv = m.encoder(x)
        enc_out = torch.cat([mu, lv], 1)
        eps = torch.from_numpy(eps_ref(SEED, DRAW, 0, mu.numel()).astype(np.float32).reshape(mu.shape))
        z = eps.mul(torch.exp(0.5 * lv)).add_(mu)
        recon = m.decoder(z)
        loss, rec, kld = vmod.loss_function(recon, x, mu, lv, SIGMA)
        assert loss.dtype == torch.float32
        o_enc = lgunet_forward(p, C.TINY_VAE["encoder"], x, "enc.")
        o_rec = lgunet_forward(p, C.TINY_VAE["decoder"], z, "dec.")
        print(f"g20: oracle restatement vs reference rel enc {rel(o_enc, enc_out):.2e} recon {rel(o_rec, recon):.2e}; "
              f"loss {float(loss):.6e} rec {float(rec):.6e} kld {float(kld):.6e}; log_var in "
              f"[{float(lv.min()):.3f}, {float(lv.max()):.3f}]")
        path = os.path.join(gold, "g20_vae_eval.npz")
        np.savez_compressed(path, x_seed=X_SEED, seed=np.uint64(SEED), draw=DRAW, sigma=SIGMA, enc_out=enc_out.numpy(),
                            z=z.numpy(), recon=recon.numpy(), loss=np.float32(loss), rec=np.float32(rec),
                            kld=np.float32(kld))
        print("wrote", path, os.path.getsize(path), "bytes")
        if args.tiny:
            return
        m, p = ref_vae(vmod, C.VAE, "full_vae", scratch)
        x = torch.from_numpy(smooth_field(FULL_X_SEED, (1, 69, 128, 256)))
        out = m.enc(x)
        o = out.numpy().reshape(-1).astype(np.float64)
        idx = np.sort(np.random.default_rng(909).choice(o.size, size=4096, replace=False)).astype(np.int64)
        path = os.path.join(gold, "g21_full_encoder.npz")
        np.savez(path, x_seed=FULL_X_SEED, idx_out=idx, out_sample=o[idx].astype(np.float32), out_sum=o.sum(),
                 out_sumsq=(o * o).sum(), out_abssum=np.abs(o).sum())
        print("g21: full encoder out sumsq %.9e" % (o * o).sum())
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
