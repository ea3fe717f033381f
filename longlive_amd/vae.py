"""Wan VAE decoder and encoder on the MI355X: the `vae` object the reference pipelines call once per
video (`self.vae.decode_to_pixel(output, use_cache=False)`, pipeline/causal_inference.py:249) or once per streamed
chunk (use_cache=True), behind the reference's WanVAEWrapper interface (utils/wan_wrapper.py:83-117) and the reference's
state-dict names (`decoder.*`, `conv2.*` of wan/modules/vae.py::WanVAE_).

Design (not a translation of the module tree): activations are channels-last bf16 [T, H, W, C]; every CausalConv3d /
Conv2d is ONE implicit-GEMM launch (ll_conv_cl) that gathers its shifted input pixels -- including the two cached
frames of temporal context, the zero padding and the nearest x2 upsample -- straight into LDS; RMS_norm + SiLU is one row
kernel; the middle attention block is GEMM + softmax + GEMM.  The reference feeds latent frames one at a time
(vae.py:555-569); causal convolutions make any chunking equivalent, so after the first frame (whose temporal upsampling
is skipped, the 'Rep' branch of Resample.forward, vae.py:108-112) frames are processed `chunk` at a time to fill the
256 CUs.  There is no CPU path: without liblonglive_hip.so every call raises.

The encoder (`encode_to_latent`, utils/wan_wrapper.py:80-94 -> WanVAE_.encode, vae.py:517-543) is the same machinery run the other
way: Encoder3d's stride-1 convolutions are ll_conv_cl launches with the same history buffers, its two strided gathers -- the
ZeroPad2d((0,1,0,1)) + Conv2d(3, stride 2) of Resample 'downsample2d/3d' and the (3,1,1) stride-(2,1,1) time_conv -- are further
gather modes of that kernel (ll_conv_cl_down, ll_conv_cl_tdown).  The reference feeds 1 frame, then 4 at a time (vae.py:520-535).
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import ops
from .synth import VaeConfig, vae_decoder_layout, vae_decoder_param_shapes, vae_encoder_layout, vae_encoder_param_shapes

bf16 = torch.bfloat16

VAE_MEAN = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508, 0.4134, -0.0715, 0.5517, -0.3632,
            -0.1922, -0.9497, 0.2503, -0.2921]
VAE_STD = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743, 3.2687, 2.1526, 2.8652, 1.5579, 1.6382,
           1.1253, 2.8251, 1.9160]


class _Conv:
    """One convolution: packed weights + (for temporal kernels) its input buffer [2 + T, H, W, Cin], whose first two frames
    are the stream's previous two input frames -- the reference's feat_cache (vae.py:29-34, 207-216) -- kept in the layout
    the kernel reads, so the history costs one 2-frame copy per call and no concatenation."""

    def __init__(self, w: torch.Tensor, b: torch.Tensor):
        self.w, self.b, self.geo = ops.pack_conv_weight(w, b)
        self.temporal = self.geo[3] > 1
        self._hist: Optional[torch.Tensor] = None       # view of the last two input frames seen so far
        self._buf: Optional[torch.Tensor] = None

    def reset(self):
        self._hist = None
        self._buf = None

    def input(self, T: int, H: int, W: int, device) -> torch.Tensor:
        """Where the producer should write this convolution's T input frames."""
        cin = self.geo[0]
        if not self.temporal:
            return torch.empty(T, H, W, cin, dtype=bf16, device=device)
        buf = torch.empty(2 + T, H, W, cin, dtype=bf16, device=device)
        if self._hist is None:
            buf[:2].zero_()
        else:
            buf[:2].copy_(self._hist)
        self._buf = buf
        return buf[2:]

    def __call__(self, x: torch.Tensor, upsample: bool = False, res: Optional[torch.Tensor] = None, rms=None,
                 want_raw: bool = True) -> torch.Tensor:
        """rms = (gamma, out_rms): the convolution's epilogue also writes rms_silu(result) into out_rms (the next convolution's input
        buffer) -- one launch instead of two where ops.conv_cl_rms_ok says so, else the two launches; want_raw = False: the
        un-normalised result is not needed (None is returned when the fused kernel ran)."""
        if not self.temporal:
            buf = x
        else:
            if self._buf is None or x.data_ptr() != self._buf[2:].data_ptr():
                self.input(x.shape[0], x.shape[1], x.shape[2], x.device).copy_(x)     # producer did not write in place
            buf, self._buf = self._buf, None
        if rms is not None and ops.conv_cl_rms_ok(self.geo, x.shape[1], x.shape[2], upsample):
            y = ops.conv_cl_rms(buf, self.w, self.b, self.geo, rms[0], rms[1], upsample=upsample, res=res, want_raw=want_raw)
        else:
            y = ops.conv_cl(buf, self.w, self.b, self.geo, upsample=upsample, res=res)
            if rms is not None:
                ops.rms_silu_cl(y, rms[0], out=rms[1])
        if self.temporal:
            self._hist = buf[-2:]
        return y


class _TDownConv:
    """The time_conv of Resample 'downsample3d' (vae.py:95-96): packed weights + its input buffer [1 + T, H, W, C] whose first frame is
    the stream's previous input frame -- feat_cache[idx][:, :, -1:] (vae.py:151-158) -- so the spatial down-convolution writes its
    result straight behind the history.  `last` is None until the first chunk has been seen (whose time_conv is skipped, vae.py:146-148)."""

    def __init__(self, w: torch.Tensor, b: torch.Tensor):
        self.w, self.b, self.geo = ops.pack_conv_weight(w, b)
        self.last: Optional[torch.Tensor] = None

    def reset(self):
        self.last = None

    def input(self, T: int, H: int, W: int, device) -> torch.Tensor:
        buf = torch.empty(1 + T, H, W, self.geo[0], dtype=bf16, device=device)
        buf[:1].copy_(self.last)
        return buf

    def __call__(self, buf: torch.Tensor) -> torch.Tensor:
        y = ops.conv_cl_tdown(buf, self.w, self.b, self.geo)
        self.last = buf[-1:]
        return y


class _VaeHalfHIP(nn.Module):
    """What Decoder3d and Encoder3d share: parameters under the reference's names, the packed convolutions with their history
    buffers, ResidualBlock and AttentionBlock."""

    _foreign: tuple = ()               # key prefixes of the other half of a WanVAE_ state dict: ignored by a strict load
    _head: tuple = ("", "")            # names of the head's RMS_norm gamma and convolution

    def _init_half(self, cfg: Optional[VaeConfig], layout, shapes, device):
        self.fuse_rms = os.environ.get("LL_VAE_FUSE", "1") != "0"      # kernel A/B only: 0 = RMS_norm + SiLU as their own launches
        self.cfg = cfg or VaeConfig()
        self.dims, self.layers = layout(self.cfg)
        self._names: Dict[str, str] = {}
        for name, shape in shapes(self.cfg).items():
            reg = name.replace(".", "__")
            self._names[name] = reg
            self.register_parameter(reg, nn.Parameter(torch.zeros(shape, dtype=bf16, device=device), requires_grad=False))
        self._packed = False
        self._convs: Dict[str, _Conv] = {}
        self._first = True

    # -- state dict with the reference's dotted names ---------------------------------------------------------------
    def state_dict(self, *a, **k):
        return {name: getattr(self, reg).data for name, reg in self._names.items()}

    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        missing = [n for n in self._names if n not in sd]
        unexpected = [n for n in sd if n not in self._names]
        if strict and (missing or [u for u in unexpected if not u.startswith(self._foreign)]):
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: missing {missing[:4]}, unexpected {unexpected[:4]}")
        for name, reg in self._names.items():
            if name in sd:
                p = getattr(self, reg)
                if tuple(sd[name].shape) != tuple(p.shape):
                    raise RuntimeError(f"{name}: shape {tuple(sd[name].shape)} != {tuple(p.shape)}")
                p.data.copy_(sd[name].to(device=p.device, dtype=bf16))
        self._packed = False
        return missing, unexpected

    def _p(self, name: str) -> torch.Tensor:
        return getattr(self, self._names[name]).data

    def _pack(self):
        """One-time re-layout of the weights for the kernels."""
        c = {}
        names = [n[:-len(".weight")] for n in self._names if n.endswith(".weight")]
        for n in names:
            if ".to_qkv" in n or ".proj" in n:
                continue
            c[n] = self._make_conv(n, self._p(n + ".weight"), self._p(n + ".bias"))
        self._convs = c
        self._attn = {}
        for L in self.layers:
            if L[0] == "attn":
                name, ch = L[1], L[2]
                wqkv = self._p(name + ".to_qkv.weight").reshape(3 * ch, ch)
                bqkv = self._p(name + ".to_qkv.bias")
                self._attn[name] = dict(
                    w=[wqkv[i * ch:(i + 1) * ch].contiguous() for i in range(3)],
                    b=[bqkv[i * ch:(i + 1) * ch].contiguous() for i in range(3)],
                    wo=self._p(name + ".proj.weight").reshape(ch, ch).contiguous(), bo=self._p(name + ".proj.bias").contiguous(),
                    gamma=self._p(name + ".norm.gamma").reshape(-1).contiguous())
        self._gamma = {n: self._p(n).reshape(-1).contiguous() for n in self._names if n.endswith("gamma")}
        self._mean = torch.tensor(VAE_MEAN[:self.cfg.z_dim], dtype=torch.float32).to(bf16).to(self._gamma[self._head[0]].device)
        std = torch.tensor(VAE_STD[:self.cfg.z_dim], dtype=torch.float32).to(bf16)
        self._inv_std = (1.0 / std).to(self._mean.device)                # utils/wan_wrapper.py:83-84, 102-103 (bf16 division)
        self._packed = True

    def _make_conv(self, name: str, w: torch.Tensor, b: torch.Tensor):
        return _Conv(w, b)

    # -- streaming state -------------------------------------------------------------------------------------------
    def clear_cache(self):
        """WanVAE_.clear_cache (vae.py:602-610)."""
        for c in self._convs.values():
            c.reset()
        self._first = True

    # -- blocks ----------------------------------------------------------------------------------------------------
    def _res_block(self, x, name, pre: bool = False, nxt=None):           # ResidualBlock.forward (vae.py:202-220)
        """pre: the producer of x already wrote rms_silu(x) into this block's first convolution's input buffer.  nxt = (gamma, conv) of
        the RMS_norm + SiLU + convolution that consume this block's output next: written by conv2's epilogue (one launch where
        ops.conv_cl_rms_ok, else conv + rms_silu) -- the un-normalised output is returned as well (the next block's shortcut)."""
        T, H, W, _ = x.shape
        c1, c2 = self._convs[name + ".residual.2"], self._convs[name + ".residual.6"]
        h = self._convs[name + ".shortcut"](x) if (name + ".shortcut") in self._convs else x
        if pre:
            y = c1._buf[2:] if c1.temporal else c1._buf
        else:
            y = ops.rms_silu_cl(x, self._gamma[name + ".residual.0.gamma"], out=c1.input(T, H, W, x.device))
        y2 = c2.input(T, H, W, x.device)
        if self.fuse_rms:
            c1(y, rms=(self._gamma[name + ".residual.3.gamma"], y2), want_raw=False)  # conv -> RMS_norm -> SiLU in one launch where covered
        else:
            ops.rms_silu_cl(c1(y), self._gamma[name + ".residual.3.gamma"], out=y2)
        if nxt is None:
            return c2(y2, res=h)
        return c2(y2, res=h, rms=(nxt[0], nxt[1].input(T, H, W, x.device)), want_raw=True)

    def _attn_block(self, x, name):                                      # AttentionBlock.forward (vae.py:240-262)
        a = self._attn[name]
        T, H, W, C = x.shape
        hw = H * W
        hwp = (hw + 63) // 64 * 64
        out = torch.empty_like(x)
        zeros_hw = torch.zeros(hwp, dtype=bf16, device=x.device)
        zeros_c = torch.zeros(C, dtype=bf16, device=x.device)
        for t in range(T):
            xt = x[t].reshape(hw, C)
            y = ops.rms_silu_cl(xt, a["gamma"], silu=False)
            q = ops.gemm(y, a["w"][0], a["b"][0])
            k = torch.zeros(hwp, C, dtype=bf16, device=x.device)
            ops.gemm(y, a["w"][1], a["b"][1], out=k[:hw])
            v = ops.gemm(y, a["w"][2], a["b"][2])
            vt = torch.zeros(C, hwp, dtype=bf16, device=x.device)
            vt[:, :hw].copy_(v.t())
            s = ops.gemm(q, k, zeros_hw)                                 # [hw, hwp] = q k^T
            p = ops.softmax_rows(s, 1.0 / math.sqrt(C), n_valid=hw)
            o = ops.gemm(p, vt, zeros_c)                                 # [hw, C] = p v
            ops.gemm(o, a["wo"], a["bo"], epilogue=ops.EPI_BIAS_RES, res=xt, out=out[t].reshape(hw, C))
        return out

    def _consumer(self, i: int):
        """(gamma, conv) of the RMS_norm + SiLU + convolution that read layer i's output next -- a residual block's first pair, or the
        head's -- when the producer can write the normalised tensor itself; None: an attention block or a resample comes next."""
        if not self.fuse_rms:
            return None
        if i + 1 == len(self.layers):
            c = (self._gamma[self._head[0]], self._convs[self._head[1]])
        elif self.layers[i + 1][0] == "res":
            nl = self.layers[i + 1]
            c = (self._gamma[nl[1] + ".residual.0.gamma"], self._convs[nl[1] + ".residual.2"])
        else:
            return None
        return c if c[1].temporal else None           # (the consumer's input buffer is remembered only by temporal convolutions)


class WanVAEDecoderHIP(_VaeHalfHIP):
    """Decoder3d + conv2 of WanVAE_ (vae.py:369-472, 545-593).  Parameters carry the reference's names so
    `load_state_dict(torch.load('Wan2.1_VAE.pth'), strict=False)` works (encoder keys are ignored)."""

    _foreign = ("encoder.", "conv1.")
    _head = ("decoder.head.0.gamma", "decoder.head.2")

    def __init__(self, cfg: Optional[VaeConfig] = None, device="cuda", chunk: int = 2):
        super().__init__()
        self._init_half(cfg, vae_decoder_layout, vae_decoder_param_shapes, device)
        self.chunk = max(1, int(chunk))

    def _resample(self, x, name, mode, nxt=None):                                  # Resample.forward (vae.py:101-143)
        if mode == "up3d" and not self._first:
            T, H, W, C = x.shape
            y = self._convs[name + ".time_conv"](x)                      # [T,H,W,2C]: two output frames per input frame
            x = y.view(T, H, W, 2, C).permute(0, 3, 1, 2, 4).reshape(2 * T, H, W, C).contiguous()   # vae.py:131-134 interleave
        conv = self._convs[name + ".resample.1"]
        if nxt is None:
            return conv(x, upsample=True)
        return conv(x, upsample=True, rms=(nxt[0], nxt[1].input(x.shape[0], 2 * x.shape[1], 2 * x.shape[2], x.device)), want_raw=True)

    def _decoder_step(self, x):                                          # Decoder3d.forward (vae.py:423-472)
        x = self._convs["decoder.conv1"](x)
        pre = False
        for i, L in enumerate(self.layers):
            nxt = self._consumer(i)
            if L[0] == "res":
                x = self._res_block(x, L[1], pre, nxt)
            elif L[0] == "attn":
                x, nxt = self._attn_block(x, L[1]), None
            else:
                x = self._resample(x, L[1], L[0], nxt)
            pre = nxt is not None
        head = self._convs["decoder.head.2"]
        if pre:
            y = head._buf[2:] if head.temporal else head._buf
        else:
            y = ops.rms_silu_cl(x, self._gamma["decoder.head.0.gamma"], out=head.input(x.shape[0], x.shape[1], x.shape[2], x.device))
        return head(y)                          # [T', H, W, 8] (3 channels + padding)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, keep_cache: bool = False, frames: str = "float") -> torch.Tensor:
        """z [T, 16, h, w] bf16 latent frames of one video -> fp32 [T', 3, 8h, 8w] in [-1, 1];
        T' = 1 + 4 (T - 1) on a fresh cache, 4 T when continuing a stream (WanVAE_.decode / cached_decode, vae.py:545-593).
        frames="uint8": video frames uint8 [T', 8h, 8w, 3] instead, `(255.0 * (v * 0.5 + 0.5).clamp(0, 1)).to(uint8)` of the float
        result v bit for bit, written by one kernel per chunk (ops.cl_to_frames_u8)."""
        if frames not in ("float", "uint8"):
            raise ValueError(f"WanVAEDecoderHIP.decode: frames={frames!r} is not 'float' or 'uint8'")
        if not self._packed:
            self._pack()
        if not keep_cache:
            self.clear_cache()
        x = ops.vae_unscale_cl(z.contiguous(), self._mean, self._inv_std)
        x = self._convs["conv2"](x)
        outs: List[torch.Tensor] = []
        i, T = 0, x.shape[0]
        while i < T:
            n = 1 if self._first else min(self.chunk, T - i)
            y = self._decoder_step(x[i:i + n])
            outs.append(ops.cl_to_tchw_clamp(y) if frames == "float" else ops.cl_to_frames_u8(y))
            self._first = False
            i += n
        if not keep_cache:
            self.clear_cache()
        return torch.cat(outs, 0)


class WanVAEEncoderHIP(_VaeHalfHIP):
    """Encoder3d + conv1 of WanVAE_ (vae.py:265-366, 517-543) on the decoder's machinery.  Only mu is computed: the first z_dim rows
    of conv1 are packed, log_var never exists.  Streaming as the reference states it: the first chunk is ONE frame, on which
    'downsample3d' stores its input and skips time_conv (vae.py:146-148); every later chunk (a multiple of 4 frames; the reference
    feeds exactly 4, causal convolutions make any multiple equivalent) runs time_conv over [cached last frame | chunk]
    (vae.py:151-158); encoder.conv1 / residual / head convolutions see zero history at the start of a stream (vae.py:29-34)."""

    _foreign = ("decoder.", "conv2.")
    _head = ("encoder.head.0.gamma", "encoder.head.2")
    CPAD = 32       # input channels of encoder.conv1 after zero padding: 32 = halo-tile kernel with the fused RMS_norm, 8 = generic decode

    def __init__(self, cfg: Optional[VaeConfig] = None, device="cuda", chunk: int = 4, cpad: Optional[int] = None):
        super().__init__()
        self._init_half(cfg, vae_encoder_layout, vae_encoder_param_shapes, device)
        chunk = int(chunk)
        if chunk < 4 or chunk % 4:
            raise ValueError(f"WanVAEEncoderHIP: chunk={chunk} must be a positive multiple of 4 (vae.py:520-535 feeds 4 frames per step)")
        self.chunk = chunk
        self.cpad = self.CPAD if cpad is None else int(cpad)

    def _make_conv(self, name, w, b):
        if name == "encoder.conv1":                 # 3 -> cpad input channels, zero weights (ll_pixels_to_cl writes zero channels)
            wp = torch.zeros(w.shape[0], self.cpad, *w.shape[2:], dtype=w.dtype, device=w.device)
            wp[:, :w.shape[1]] = w
            return _Conv(wp, b)
        if name == "conv1":                         # mu, log_var = conv1(out).chunk(2, dim=1) (vae.py:536): mu's rows only
            return _Conv(w[:self.cfg.z_dim], b[:self.cfg.z_dim])
        if name.endswith(".time_conv"):
            return _TDownConv(w, b)
        return _Conv(w, b)

    def _downsample(self, x, name, mode):           # Resample.forward, downsample modes (vae.py:138-160)
        conv = self._convs[name + ".resample.1"]
        tc = self._convs[name + ".time_conv"] if mode == "down3d" else None
        T, H, W, _ = x.shape
        if tc is None or tc.last is None:
            y = ops.conv_cl_down(x, conv.w, conv.b, conv.geo)
            if tc is not None:
                tc.last = y[-1:]                    # feat_cache[idx] = x.clone(); time_conv skipped (vae.py:146-148)
            return y
        buf = tc.input(T, H // 2, W // 2, x.device)
        ops.conv_cl_down(x, conv.w, conv.b, conv.geo, out=buf[1:])
        return tc(buf)

    def _encoder_step(self, px, channel_dim: int):   # Encoder3d.forward (vae.py:318-366) + conv1's mu rows
        c1 = self._convs["encoder.conv1"]
        if px.dtype == torch.uint8:                 # video frames [T, H, W, 3]: normalised, rounded and laid out by one kernel
            T, H, W = px.shape[:3]
            x = ops.pixels_u8_to_cl(px, self.cpad, out=c1.input(T, H, W, px.device))
        else:
            T, H, W = px.shape[1 - channel_dim], px.shape[2], px.shape[3]
            x = ops.pixels_to_cl(px, channel_dim, self.cpad, out=c1.input(T, H, W, px.device))
        nxt = self._consumer(-1)
        if nxt is None:
            x = c1(x)
        else:
            x = c1(x, rms=(nxt[0], nxt[1].input(T, H, W, px.device)), want_raw=True)
        pre = nxt is not None
        for i, L in enumerate(self.layers):
            nxt = self._consumer(i)
            if L[0] == "res":
                x = self._res_block(x, L[1], pre, nxt)
            elif L[0] == "attn":
                x, nxt = self._attn_block(x, L[1]), None
            else:
                x, nxt = self._downsample(x, L[1], L[0]), None
            pre = nxt is not None
        head = self._convs["encoder.head.2"]
        if pre:
            y = head._buf[2:]
        else:
            y = ops.rms_silu_cl(x, self._gamma["encoder.head.0.gamma"], out=head.input(x.shape[0], x.shape[1], x.shape[2], x.device))
        return self._convs["conv1"](head(y))        # [T', h, w, z_dim]

    @torch.no_grad()
    def encode(self, x: torch.Tensor, keep_cache: bool = False, channel_dim: int = 0) -> torch.Tensor:
        """x [3, T, H, W] (or [T, 3, H, W] with channel_dim = 1), fp32 or bf16 pixels in [-1, 1] of one video -> fp32 [T', 16, H/8, W/8]
        scaled latent means; T' = 1 + (T - 1) // 4 on a fresh cache (frames beyond 1 + 4k are dropped, vae.py:521), T // 4 when
        keep_cache continues a stream (the mirror of the decoder's streaming decode; the reference has no such flag).
        A uint8 x is video frames [T, H, W, 3] (channel_dim is not read): the same latents as (x.float() / 127.5 - 1) laid out [3, T, H, W]."""
        if not x.is_cuda:
            raise RuntimeError("WanVAEEncoderHIP.encode: expected a device tensor (longlive_amd has no CPU path)")
        if x.dtype == torch.uint8 and (x.dim() != 4 or x.shape[3] != 3):
            raise RuntimeError(f"WanVAEEncoderHIP.encode: uint8 input must be frames [T, H, W, 3], got {tuple(x.shape)}")
        if not self._packed:
            self._pack()
        if not keep_cache:
            self.clear_cache()
        tdim = 0 if x.dtype == torch.uint8 else 1 - channel_dim
        T = x.shape[tdim]
        outs: List[torch.Tensor] = []
        i = 0
        while True:
            n = 1 if self._first else min(self.chunk, (T - i) // 4 * 4)
            if n <= 0 or i + n > T:
                break
            mu = self._encoder_step(x.narrow(tdim, i, n), channel_dim)
            outs.append(ops.vae_scale_tchw(mu, self._mean, self._inv_std))
            self._first = False
            i += n
        if not keep_cache:
            self.clear_cache()
        if not outs:
            raise RuntimeError(f"WanVAEEncoderHIP.encode: {T} frames hold no whole step (1 frame first, then 4 per step)")
        return torch.cat(outs, 0)


class WanVAEWrapper(nn.Module):
    """Drop-in for utils/wan_wrapper.py::WanVAEWrapper: `decode_to_pixel(latent [B,T,16,h,w], use_cache) -> [B,T',3,H,W]` fp32 in
    [-1,1] and `encode_to_latent(pixel [B,3,T,H,W]) -> [B,1+(T-1)//4,16,H/8,W/8]` fp32.  The encoder's device parameters and buffers
    are created at the first encode: until then its weights stay wherever load_state_dict found them (decode-only users pay nothing)."""

    def __init__(self, cfg: Optional[VaeConfig] = None, device="cuda", chunk: int = 2, encode_chunk: int = 4):
        super().__init__()
        self.model = WanVAEDecoderHIP(cfg, device=device, chunk=chunk)
        self.mean = torch.tensor(VAE_MEAN, dtype=torch.float32)
        self.std = torch.tensor(VAE_STD, dtype=torch.float32)
        self._device, self._encode_chunk = device, encode_chunk
        self._encoder_sd: Optional[Dict[str, torch.Tensor]] = None      # the checkpoint's encoder.* / conv1.* tensors, not yet on the device
        self.encoder: Optional[WanVAEEncoderHIP] = None

    def load_state_dict(self, sd, strict: bool = True, assign: bool = False):
        sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
        enc = {k: v for k, v in sd.items() if k.startswith(WanVAEDecoderHIP._foreign)}
        if enc:                                     # a checkpoint without them still loads for decode-only use
            want = vae_encoder_param_shapes(self.model.cfg)
            missing = [n for n in want if n not in enc]
            unexpected = [n for n in enc if n not in want]
            if strict and (missing or unexpected):
                raise RuntimeError(f"WanVAEWrapper.load_state_dict: encoder keys missing {missing[:4]}, unexpected {unexpected[:4]}")
            for n, v in enc.items():
                if n in want and tuple(v.shape) != tuple(want[n]):
                    raise RuntimeError(f"{n}: shape {tuple(v.shape)} != {tuple(want[n])}")
            self._encoder_sd = enc
            if self.encoder is not None:
                self.encoder.load_state_dict(enc, strict=False)
        return self.model.load_state_dict(sd, strict=strict)

    def decode_to_pixel(self, latent: torch.Tensor, use_cache: bool = False) -> torch.Tensor:
        if latent.dtype != bf16:
            latent = latent.to(bf16)
        if use_cache:      # ONE streaming feature cache: a second sample would continue the first one's stream
            assert latent.shape[0] == 1, "Batch size must be 1 when using cache"          # utils/wan_wrapper.py:99
        out = [self.model.decode(u, keep_cache=use_cache) for u in latent]
        return torch.stack(out, 0)

    def decode_to_frames(self, latent: torch.Tensor, use_cache: bool = False) -> torch.Tensor:
        """latent [B, T, 16, h, w] -> video frames uint8 [B, T', H, W, 3]: bit for bit
        `(255.0 * (decode_to_pixel(latent, use_cache) * 0.5 + 0.5).clamp(0, 1).permute(0, 1, 3, 4, 2)).to(torch.uint8)`, without the
        fp32 planes ever existing."""
        if latent.dtype != bf16:
            latent = latent.to(bf16)
        if use_cache:
            assert latent.shape[0] == 1, "Batch size must be 1 when using cache"
        return torch.stack([self.model.decode(u, keep_cache=use_cache, frames="uint8") for u in latent], 0)

    def _get_encoder(self) -> WanVAEEncoderHIP:
        if self.encoder is None:
            if self._encoder_sd is None:
                raise RuntimeError("WanVAEWrapper.encode_to_latent: no encoder weights were loaded (the state dict held no "
                                   "`encoder.*` / `conv1.*` keys): this VAE is decode-only")
            enc = WanVAEEncoderHIP(self.model.cfg, device=self._device, chunk=self._encode_chunk)
            enc.load_state_dict(self._encoder_sd, strict=False)
            self.encoder = enc
        return self.encoder

    def encode_to_latent(self, pixel: torch.Tensor, keep_cache: bool = False) -> torch.Tensor:
        """utils/wan_wrapper.py:80-94.  keep_cache (not in the reference): continue the stream of the previous call (B = 1)."""
        if pixel.dim() != 5 or pixel.shape[1] != 3:
            raise RuntimeError(f"encode_to_latent: expected pixel [B, 3, T, H, W], got {tuple(pixel.shape)}")
        if not pixel.is_cuda:
            raise RuntimeError("encode_to_latent: expected a device tensor (longlive_amd has no CPU path)")
        if keep_cache:
            assert pixel.shape[0] == 1, "Batch size must be 1 when using cache"
        enc = self._get_encoder()
        return torch.stack([enc.encode(u, keep_cache=keep_cache) for u in pixel], 0)

    def encode_frames_to_latent(self, frames: torch.Tensor, keep_cache: bool = False) -> torch.Tensor:
        """Video frames uint8 [B, T, H, W, 3] -> fp32 [B, 1 + (T - 1) // 4, 16, H/8, W/8]: bit for bit
        encode_to_latent((frames.float() / 127.5 - 1).permute(0, 4, 1, 2, 3)), without the fp32 planes ever existing."""
        if frames.dim() != 5 or frames.shape[4] != 3 or frames.dtype != torch.uint8:
            raise RuntimeError(f"encode_frames_to_latent: expected uint8 frames [B, T, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
        if not frames.is_cuda:
            raise RuntimeError("encode_frames_to_latent: expected a device tensor (longlive_amd has no CPU path)")
        if keep_cache:
            assert frames.shape[0] == 1, "Batch size must be 1 when using cache"
        enc = self._get_encoder()
        return torch.stack([enc.encode(u, keep_cache=keep_cache) for u in frames], 0)
