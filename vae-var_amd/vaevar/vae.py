"""The whole VAE_lr of nf_model/vae.py:53-107 on the HIP engine, for evaluating a checkpoint (forwards only: no weight
gradient, no LoRA).

  VAE_lr.encoder        vae.py:72-76     enc = LGUnet_all(**encoder block), chunk(2, dim=1)
  VAE_lr.sampling       vae.py:78-81     z = eps * exp(log_var / 2) + mu           (vv_vae_sample)
  VAE_lr.decoder(_hr)   vae.py:83-90     dec = LGUnet_all(**decoder block)
  VAE_lr.forward        vae.py:99-102
  loss_function         vae.py:104-107   MSE / (2 sigma^2) + KLD                   (vv_vae_sse, vv_vae_sample)
  prior samples         model/model.py:651-652   decoder(randn) * err_std          (vv_normal_fill)

Where the reference draws torch.randn_like, the noise here is the engine's counter-based stream, a pure function of
(seed, draw): the same call gives the same bits on every run. engine.VAE_lr (the decoder half the analysis uses) is
unchanged.
"""
from __future__ import annotations

import numpy as np
import torch

from . import config
from .engine import Context, LGUnet, normal_fill, resample_nearest, vae_sample, vae_sse

_KEYS = ("img_size", "patch_size", "stride", "inchans_list", "outchans_list", "enc_dim", "embed_dim", "window_size",
         "enc_depths", "enc_heads", "lg_depths", "lg_heads")


def _engine_cfg(block: dict) -> dict:
    """The keys of a yaml block the engine uses; the others (in_chans, Weather_T, drop_path, ...) are ignored."""
    return {k: block[k] for k in _KEYS}


class VAE_lr:
    """params: the yaml's dict with its `encoder` and `decoder` blocks (config.VAE, config.TINY_VAE). batch: the B of
    every call. state_grid: the grid decoder_hr resamples to (default: the network's)."""

    def __init__(self, params: dict, batch: int = 1, ctx: Context | None = None, state_grid=None):
        enc_cfg, dec_cfg = _engine_cfg(params["encoder"]), _engine_cfg(params["decoder"])
        self.ctx = Context.get(0) if ctx is None else ctx
        self.enc = LGUnet(enc_cfg, batch, 1, ctx=self.ctx)
        self.dec = LGUnet(dec_cfg, batch, 1, ctx=self.ctx)
        if self.enc.out_ch != 2 * self.dec.in_ch:
            raise ValueError(f"the encoder writes {self.enc.out_ch} channels, the decoder reads {self.dec.in_ch}: "
                             f"mu and log_var need twice the latent channels")
        if self.enc.in_ch != self.dec.out_ch or (self.enc.H, self.enc.W) != (self.dec.H, self.dec.W):
            raise ValueError("encoder input and decoder output differ in channels or grid")
        self.batch, self.device = batch, self.enc.device
        self.L, self.C, self.H, self.W = self.dec.in_ch, self.enc.in_ch, self.enc.H, self.enc.W
        self.state_grid = tuple(state_grid) if state_grid else (self.H, self.W)

    def load_state_dict(self, sd: dict):
        """The reference's VAE_lr.state_dict(): `enc.` / `dec.` prefixes, module. / max_logvar filtered."""
        self.enc.load_state_dict(sd, "enc.")
        self.dec.load_state_dict(sd, "dec.")
        return self

    def load_synthetic(self, base_seed: int = 20250620):
        self.enc.load_synthetic(base_seed, "enc.")
        self.dec.load_synthetic(base_seed, "dec.")
        return self

    # --- vae.py:72-102 ---
    def encode(self, x: torch.Tensor, out=None) -> torch.Tensor:
        """self.enc(x): the (B, 2L, H, W) buffer mu and log_var are views of."""
        return self.enc.forward_raw(x, out=out)

    def encoder(self, x: torch.Tensor):
        """(mu, log_var): encode(x).chunk(2, dim=1), views of one buffer."""
        e = self.encode(x)
        return e[:, :self.L], e[:, self.L:]

    def _enc_out(self, enc_out) -> torch.Tensor:
        if isinstance(enc_out, (tuple, list)):  # the (mu, log_var) views encoder() returned
            mu, lv = enc_out
            base = mu._base if mu._base is not None else mu
            if not (lv._base is base and tuple(base.shape) == (mu.shape[0], 2 * self.L) + tuple(mu.shape[2:]) and
                    mu.data_ptr() == base.data_ptr()):
                raise ValueError("mu and log_var must be the two views encoder() returned")
            return base
        return enc_out

    def sampling(self, enc_out, seed: int, draw: int, mean: bool = False) -> torch.Tensor:
        """z = eps * exp(log_var / 2) + mu, eps = normal_fill(seed, draw) at z's element index; the posterior mean mu
        with mean=True. enc_out: encode()'s buffer or encoder()'s pair."""
        return vae_sample(self.ctx, self._enc_out(enc_out), seed, draw, mean)[0]

    def decoder(self, z: torch.Tensor) -> torch.Tensor:
        return self.dec(z)

    def decoder_hr(self, z: torch.Tensor) -> torch.Tensor:
        x = self.dec(z)
        if self.state_grid != tuple(x.shape[-2:]):
            x = resample_nearest(self.ctx, x, self.state_grid)
        return x

    def forward(self, x: torch.Tensor, seed: int, draw: int):
        """(recon, mu, log_var) of vae.py:99-102."""
        e = self.encode(x)
        return self.dec.forward_raw(vae_sample(self.ctx, e, seed, draw)[0]), e[:, :self.L], e[:, self.L:]

    # --- vae.py:104-107 ---
    def loss_tables(self, recon: torch.Tensor, x: torch.Tensor, enc_out):
        """(sse (B, C), stat (B, L, 4)): the float64 device tables loss_function is made of."""
        e = self._enc_out(enc_out)
        stat = torch.empty(e.shape[0], self.L, 4, device=e.device, dtype=torch.float64)
        vae_sample(self.ctx, e, stat=stat, want_z=False)
        return vae_sse(self.ctx, recon, x, C=self.C), stat

    def loss_function(self, recon: torch.Tensor, x: torch.Tensor, enc_out, sigma: float):
        """(MSE + KLD, MSE * 2 sigma^2, KLD) as vae.py:104-107 returns them, three 0-d float64 device tensors: the sums
        of the (B, C) and (B, L) tables, formed on the device without a host wait. The reference sums fp32 terms in
        fp32; here the squared differences are its fp32 elements and the KL terms fp64, both summed in fp64."""
        sse, stat = self.loss_tables(recon, x, enc_out)
        rec = sse.sum()
        kld = -0.5 * stat[:, :, 0].sum()
        return rec / (2.0 * float(sigma) ** 2) + kld, rec, kld

    # --- model/model.py:651-652 ---
    def sample_prior(self, seed: int, draw: int, err_std=config.STD_TR):
        """(z, y): z = randn(B, L, H, W) from normal_fill(seed, draw), y = decoder(z) * err_std, the physical-space
        draws from the prior the reference saves after every epoch."""
        sd = np.asarray(err_std.detach().cpu() if isinstance(err_std, torch.Tensor) else err_std, np.float32)
        if sd.shape != (self.C,):
            raise ValueError(f"err_std must hold {self.C} values, got {sd.shape}")
        n = self.batch * self.L * self.H * self.W
        z = normal_fill(self.ctx, n, seed, draw, device=self.device.index).view(self.batch, self.L, self.H, self.W)
        y = self.dec.forward_raw(z)
        for b in range(self.batch):
            for c in range(self.C):
                self.ctx.scale(y[b, c], float(sd[c]))
        return z, y
