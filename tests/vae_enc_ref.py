"""TEST INFRASTRUCTURE ONLY -- never imported by the product path (longlive_amd/).

CPU restatement of the Wan VAE *encoder* as LongLive uses it (wan/modules/vae.py): WanVAE_.encode (:517-543) feeds the pixel frames
as 1, 4, 4, ... through Encoder3d (:265-366) with per-convolution feature caches, takes mu from conv1 and scales it.  Functional over
a state dict, on the decoder restatement's blocks (oracle/ref_vae.py: causal convolution with its cache idiom, ResidualBlock,
AttentionBlock).  Pinned bit-exact to the reference's own classes by tests/golden/vae_encode.pt (tools/make_golden_vae_encode.py) in
tests/test_vae_encoder_host.py.

What is restated, not "fixed": on the first chunk 'downsample3d' stores its input and skips time_conv (:146-148); afterwards time_conv
(stride 2, no padding) runs over [last cached frame | chunk] and the cache keeps the chunk's last frame (:151-158)."""
from typing import Dict, List

import torch
import torch.nn.functional as F

from oracle import ref_vae as RV

Tensor = torch.Tensor
# the inputs every golden case is made of: (seed, [B, 3, T, H, W]); tools/make_golden_vae_encode.py and the tests build them from here
ENC_SEED = 6                      # synth_vae_encoder_state_dict seed
CASES = {"t1": (61, (1, 3, 1, 64, 96)), "t9": (62, (1, 3, 9, 64, 96)), "t6": (63, (1, 3, 6, 64, 96)), "b2": (64, (2, 3, 5, 64, 96))}


def case_pixels(tag: str) -> Tensor:
    """hash_uniform in [-1, 1] cast to bf16."""
    from longlive_amd import synth
    seed, shape = CASES[tag]
    return (synth.hash_uniform(seed, "vae.pixels." + tag, shape) * 2.0 - 1.0).to(torch.bfloat16)


class RefVaeEncoder(RV.RefVaeDecoder):
    """layers = longlive_amd.synth.vae_encoder_layout(cfg)[1]."""

    def downsample(self, x: Tensor, name: str, mode: str) -> Tensor:          # Resample.forward, downsample modes (:138-160)
        b, c, t, h, w = x.shape
        y = x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
        y = F.conv2d(F.pad(y, (0, 1, 0, 1)), self.sd[name + ".resample.1.weight"], self.sd[name + ".resample.1.bias"], stride=(2, 2))
        x = y.reshape(b, t, c, y.shape[2], y.shape[3]).permute(0, 2, 1, 3, 4)
        if mode == "down3d":
            i = self.idx
            if self.cache[i] is None:
                self.cache[i] = x.clone()
            else:
                cache_x = x[:, :, -1:].clone()
                x = F.conv3d(torch.cat([self.cache[i][:, :, -1:], x], 2), self.sd[name + ".time_conv.weight"],
                             self.sd[name + ".time_conv.bias"], stride=(2, 1, 1))
                self.cache[i] = cache_x
            self.idx += 1
        return x

    def encoder_step(self, x: Tensor) -> Tensor:                              # Encoder3d.forward with feat_cache (:318-366)
        self.idx = 0
        x = self._cached_conv(x, "encoder.conv1")
        for L in self.layers:
            if L[0] == "res":
                x = self.res_block(x, L[1])
            elif L[0] == "attn":
                x = self.attn_block(x, L[1])
            else:
                x = self.downsample(x, L[1], L[0])
        x = F.silu(RV.rms_norm(x, self.sd["encoder.head.0.gamma"]))
        return self._cached_conv(x, "encoder.head.2")

    def encode(self, x: Tensor, mean: Tensor, inv_std: Tensor, chunk: int = 4, keep_cache: bool = False) -> Tensor:
        """WanVAE_.encode (:517-543).  x [1, 3, T, H, W] -> mu [1, 16, T', H/8, W/8]; on a fresh cache 1 frame, then `chunk` (the
        reference: 4) per step; with keep_cache the stream of the previous call continues (steps of `chunk` from its first frame)."""
        assert chunk % 4 == 0
        if not keep_cache:
            self.reset()
        fresh = all(c is None for c in self.cache)
        T = x.shape[2]
        outs: List[Tensor] = []
        i = 0
        while True:
            n = 1 if (fresh and i == 0) else min(chunk, (T - i) // 4 * 4)
            if n <= 0 or i + n > T:
                break
            outs.append(self.encoder_step(x[:, :, i:i + n]))
            i += n
        out = torch.cat(outs, 2)
        mu = F.conv3d(out, self.sd["conv1.weight"], self.sd["conv1.bias"]).chunk(2, dim=1)[0]
        mu = (mu - mean.view(1, -1, 1, 1, 1)) * inv_std.view(1, -1, 1, 1, 1)
        if not keep_cache:
            self.reset()
        return mu


def encode_to_latent(enc: RefVaeEncoder, pixel: Tensor, chunk: int = 4, keep_cache: bool = False) -> Tensor:
    """WanVAEWrapper.encode_to_latent (utils/wan_wrapper.py:80-94): pixel [B, 3, T, H, W] -> [B, T', 16, H/8, W/8] fp32."""
    mean = torch.tensor(RV.VAE_MEAN, dtype=torch.float32).to(pixel.dtype)
    inv_std = 1.0 / torch.tensor(RV.VAE_STD, dtype=torch.float32).to(pixel.dtype)      # wan_wrapper.py:83-84: division in the pixel dtype
    out = [enc.encode(u.unsqueeze(0), mean, inv_std, chunk, keep_cache).float().squeeze(0) for u in pixel]
    return torch.stack(out, 0).permute(0, 2, 1, 3, 4)


def make_encoder(cfg=None, dtype=torch.bfloat16) -> RefVaeEncoder:
    from longlive_amd import synth
    cfg = cfg or synth.VaeConfig()
    return RefVaeEncoder(synth.synth_vae_encoder_state_dict(cfg, seed=ENC_SEED), synth.vae_encoder_layout(cfg)[1], dtype)
