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


class _Staged:
    """A convolution's input where its kernel reads it: `buf` [hist + T, H, W, Cin] -- the stream's previous `hist` input frames, then
    the T new ones -- and `new` = buf[hist:], where a producer writes them.  Made by the convolution (input / stage), held by the
    caller, handed back to the convolution's call."""
    __slots__ = ("buf", "new")

    def __init__(self, buf: torch.Tensor, hist: int):
        self.buf, self.new = buf, buf[hist:]


class _Conv:
    """One convolution: packed weights + (for temporal kernels, hist = 2) a view of the last two input frames it has read -- the
    reference's feat_cache (vae.py:29-34, 207-216) -- kept in the layout the kernel reads, so the history costs one 2-frame copy
    per call and no concatenation.  The view keeps the buffer it lies in alive until the next call."""

    def __init__(self, w: torch.Tensor, b: torch.Tensor, fuse_rms: bool = True):
        self.w, self.b, self.geo = ops.pack_conv_weight(w, b)
        self.hist = 2 if self.geo[3] > 1 else 0
        self.fuse_rms = fuse_rms
        self._hist: Optional[torch.Tensor] = None

    def reset(self):
        self._hist = None

    def input(self, T: int, H: int, W: int, device) -> _Staged:
        """Room for T input frames behind the history (zeros at the start of a stream)."""
        buf = torch.empty(self.hist + T, H, W, self.geo[0], dtype=bf16, device=device)
        if self.hist:
            if self._hist is None:
                buf[:self.hist].zero_()
            else:
                buf[:self.hist].copy_(self._hist)
        return _Staged(buf, self.hist)

    def stage(self, x: torch.Tensor) -> _Staged:
        """An input that already exists as a tensor: copied behind the history -- or, with no history to put in front of it, read
        where it lies."""
        if not self.hist:
            return _Staged(x, 0)
        s = self.input(x.shape[0], x.shape[1], x.shape[2], x.device)
        s.new.copy_(x)
        return s

    def __call__(self, s: _Staged, upsample: bool = False, res: Optional[torch.Tensor] = None, rms=None,
                 want_raw: bool = True) -> torch.Tensor:
        """rms = (gamma, staged): rms_silu(result) is written into staged.new (the next convolution's input) as well -- by this
        convolution's epilogue, one launch instead of two, where fusing is on and ops.conv_cl_rms_ok says so, else by the two launches;
        want_raw = False: the un-normalised result is not needed (None is returned when the fused kernel ran)."""
        H, W = s.new.shape[1:3]
        if rms is not None and self.fuse_rms and ops.conv_cl_rms_ok(self.geo, H, W, upsample):
            y = ops.conv_cl_rms(s.buf, self.w, self.b, self.geo, rms[0], rms[1].new, upsample=upsample, res=res, want_raw=want_raw)
        else:
            y = ops.conv_cl(s.buf, self.w, self.b, self.geo, upsample=upsample, res=res)
            if rms is not None:
                ops.rms_silu_cl(y, rms[0], out=rms[1].new)
        if self.hist:
            self._hist = s.buf[-self.hist:]
        return y


class _TDownConv(_Conv):
    """The time_conv of Resample 'downsample3d' (vae.py:95-96): ONE history frame -- feat_cache[idx][:, :, -1:] (vae.py:151-158) -- in
    front of its input, so the spatial down-convolution writes its result straight behind it.  The stream's first chunk does not
    run it (vae.py:146-148): `skip` takes that chunk instead, and until then there is no input to ask for."""

    def __init__(self, w: torch.Tensor, b: torch.Tensor):
        super().__init__(w, b)
        self.hist = 1

    @property
    def started(self) -> bool:
        return self._hist is not None

    def skip(self, y: torch.Tensor) -> torch.Tensor:
        self._hist = y[-1:]                         # feat_cache[idx] = x.clone(); time_conv skipped (vae.py:146-148)
        return y

    def input(self, T: int, H: int, W: int, device) -> _Staged:
        if self._hist is None:
            raise RuntimeError("time_conv: its input was asked for before the stream's first chunk (which skips it) was seen")
        return super().input(T, H, W, device)

    def __call__(self, s: _Staged) -> torch.Tensor:
        y = ops.conv_cl_tdown(s.buf, self.w, self.b, self.geo)
        self._hist = s.buf[-1:]
        return y


class _VaeHalfHIP(nn.Module):
    """What Decoder3d and Encoder3d share: parameters under the reference's names, the packed convolutions with their history
    buffers, ResidualBlock and AttentionBlock."""

    _foreign: tuple = ()               # key prefixes of the other half of a WanVAE_ state dict: ignored by a strict load
    _head: tuple = ("", "")            # names of the head's RMS_norm gamma and convolution

    def _init_half(self, cfg: Optional[VaeConfig], layout, shapes, device, fuse_rms: Optional[bool]):
        # kernel A/B only: LL_VAE_FUSE=0 (fuse_rms=False) = RMS_norm + SiLU as their own launches
        self.fuse_rms = os.environ.get("LL_VAE_FUSE", "1") != "0" if fuse_rms is None else bool(fuse_rms)
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
        return _Conv(w, b, self.fuse_rms)

    # -- streaming state -------------------------------------------------------------------------------------------
    def clear_cache(self):
        """WanVAE_.clear_cache (vae.py:602-610)."""
        for c in self._convs.values():
            c.reset()
        self._first = True

    # -- blocks ----------------------------------------------------------------------------------------------------
    def _normed(self, x, gamma, conv: _Conv, staged: Optional[_Staged]) -> _Staged:
        """rms_silu(x) as conv's input: the one x's producer handed over, held to x's frames, else written here by its own launch."""
        T, H, W, _ = x.shape
        if staged is None:
            staged = conv.input(T, H, W, x.device)
            ops.rms_silu_cl(x, gamma, out=staged.new)
        elif tuple(staged.buf.shape) != (conv.hist + T, H, W, conv.geo[0]):
            raise RuntimeError(f"staged input {tuple(staged.buf.shape)} does not belong to {tuple(x.shape)} read by a convolution of "
                               f"{conv.geo[0]} channels with {conv.hist} history frames")
        return staged

    def _conv_handoff(self, conv: _Conv, s: _Staged, nxt, upsample: bool = False, res=None):
        """conv(s) -> (raw, staged): nxt = (gamma, conv) of the RMS_norm + SiLU + convolution that read the result next gets
        rms_silu(raw) staged as its input by this launch (or the two, _Conv.__call__), raw being kept for the shortcut; None without nxt."""
        if nxt is None:
            return conv(s, upsample=upsample, res=res), None
        T, H, W, _ = s.new.shape
        out = nxt[1].input(T, H << upsample, W << upsample, s.new.device)
        return conv(s, upsample=upsample, res=res, rms=(nxt[0], out)), out

    def _res_block(self, x, name, staged: Optional[_Staged] = None, nxt=None):   # ResidualBlock.forward (vae.py:202-220)
        """staged: rms_silu(x) as the producer of x wrote it into this block's first convolution's input; nxt: see _conv_handoff."""
        c1, c2 = self._convs[name + ".residual.2"], self._convs[name + ".residual.6"]
        sc = self._convs.get(name + ".shortcut")
        h = sc(sc.stage(x)) if sc is not None else x
        s1 = self._normed(x, self._gamma[name + ".residual.0.gamma"], c1, staged)
        s2 = c2.input(x.shape[0], x.shape[1], x.shape[2], x.device)
        c1(s1, rms=(self._gamma[name + ".residual.3.gamma"], s2), want_raw=False)
        return self._conv_handoff(c2, s2, nxt, res=h)

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
        head's -- when the producer can write the normalised tensor itself; None: an attention block or a resample comes next.
        Offered to temporal convolutions only: in both layouts of the default VaeConfig that is every one of them."""
        if not self.fuse_rms:
            return None
        if i + 1 == len(self.layers):
            c = (self._gamma[self._head[0]], self._convs[self._head[1]])
        elif self.layers[i + 1][0] == "res":
            nl = self.layers[i + 1]
            c = (self._gamma[nl[1] + ".residual.0.gamma"], self._convs[nl[1] + ".residual.2"])
        else:
            return None
        return c if c[1].hist == 2 else None

    def _walk(self, x, staged: Optional[_Staged] = None):
        """The layers behind the front end (which may hand over rms_silu(x) staged for the first block), then the head: RMS_norm +
        SiLU + head convolution.  Decoder3d.forward (vae.py:423-472) and Encoder3d.forward (vae.py:318-366) alike."""
        for i, L in enumerate(self.layers):
            if L[0] == "res":
                x, staged = self._res_block(x, L[1], staged, self._consumer(i))
            elif L[0] == "attn":
                x, staged = self._attn_block(x, L[1]), None
            else:
                x, staged = self._resample(x, L[1], L[0], self._consumer(i))
        head = self._convs[self._head[1]]
        return head(self._normed(x, self._gamma[self._head[0]], head, staged))


class WanVAEDecoderHIP(_VaeHalfHIP):
    """Decoder3d + conv2 of WanVAE_ (vae.py:369-472, 545-593).  Parameters carry the reference's names so
    `load_state_dict(torch.load('Wan2.1_VAE.pth'), strict=False)` works (encoder keys are ignored)."""

    _foreign = ("encoder.", "conv1.")
    _head = ("decoder.head.0.gamma", "decoder.head.2")

    def __init__(self, cfg: Optional[VaeConfig] = None, device="cuda", chunk: int = 2, fuse_rms: Optional[bool] = None):
        super().__init__()
        self._init_half(cfg, vae_decoder_layout, vae_decoder_param_shapes, device, fuse_rms)
        self.chunk = max(1, int(chunk))

    def _resample(self, x, name, mode, nxt):                             # Resample.forward (vae.py:101-143)
        if mode == "up3d" and not self._first:
            T, H, W, C = x.shape
            tc = self._convs[name + ".time_conv"]
            y = tc(tc.stage(x))                                          # [T,H,W,2C]: two output frames per input frame
            x = y.view(T, H, W, 2, C).permute(0, 3, 1, 2, 4).reshape(2 * T, H, W, C).contiguous()   # vae.py:131-134 interleave
        conv = self._convs[name + ".resample.1"]
        return self._conv_handoff(conv, conv.stage(x), nxt, upsample=True)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, keep_cache: bool = False, frames: str = "float", yuv_range: str = "limited") -> torch.Tensor:
        """z [T, 16, h, w] bf16 latent frames of one video -> fp32 [T', 3, 8h, 8w] in [-1, 1];
        T' = 1 + 4 (T - 1) on a fresh cache, 4 T when continuing a stream (WanVAE_.decode / cached_decode, vae.py:545-593).
        frames="uint8": video frames uint8 [T', 8h, 8w, 3] instead, `(255.0 * (v * 0.5 + 0.5).clamp(0, 1)).to(uint8)` of the float
        result v bit for bit, written by one kernel per chunk (ops.cl_to_frames_u8).
        frames="yuv420": those frames as I420 uint8 [T', ops.yuv420_bytes(8h, 8w)] in `yuv_range` (limited | full), bit for bit
        ops.frames_u8_to_yuv420 of the uint8 result, written by one kernel per chunk (ops.cl_to_yuv420)."""
        if frames not in ("float", "uint8", "yuv420"):
            raise ValueError(f"WanVAEDecoderHIP.decode: frames={frames!r} is not 'float', 'uint8' or 'yuv420'")
        if frames == "yuv420" and yuv_range not in ops.YUV_RANGES:
            raise ValueError(f"WanVAEDecoderHIP.decode: yuv_range={yuv_range!r} is not 'limited' or 'full'")
        if not self._packed:
            self._pack()
        if not keep_cache:
            self.clear_cache()
        x = ops.vae_unscale_cl(z.contiguous(), self._mean, self._inv_std)
        conv2, conv1 = self._convs["conv2"], self._convs["decoder.conv1"]
        x = conv2(conv2.stage(x))
        outs: List[torch.Tensor] = []
        i, T = 0, x.shape[0]
        while i < T:
            n = 1 if self._first else min(self.chunk, T - i)
            y = self._walk(conv1(conv1.stage(x[i:i + n])))               # [T', H, W, 8] (3 channels + padding)
            if frames == "yuv420":
                outs.append(ops.cl_to_yuv420(y, yuv_range))
            else:
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

    def __init__(self, cfg: Optional[VaeConfig] = None, device="cuda", chunk: int = 4, cpad: Optional[int] = None,
                 fuse_rms: Optional[bool] = None):
        super().__init__()
        self._init_half(cfg, vae_encoder_layout, vae_encoder_param_shapes, device, fuse_rms)
        chunk = int(chunk)
        if chunk < 4 or chunk % 4:
            raise ValueError(f"WanVAEEncoderHIP: chunk={chunk} must be a positive multiple of 4 (vae.py:520-535 feeds 4 frames per step)")
        self.chunk = chunk
        self.cpad = self.CPAD if cpad is None else int(cpad)

    def _make_conv(self, name, w, b):
        if name == "encoder.conv1":                 # 3 -> cpad input channels, zero weights (ll_pixels_to_cl writes zero channels)
            wp = torch.zeros(w.shape[0], self.cpad, *w.shape[2:], dtype=w.dtype, device=w.device)
            wp[:, :w.shape[1]] = w
            w = wp
        elif name == "conv1":                       # mu, log_var = conv1(out).chunk(2, dim=1) (vae.py:536): mu's rows only
            w, b = w[:self.cfg.z_dim], b[:self.cfg.z_dim]
        elif name.endswith(".time_conv"):
            return _TDownConv(w, b)
        return super()._make_conv(name, w, b)

    def _resample(self, x, name, mode, nxt):        # Resample.forward, downsample modes (vae.py:138-160)
        """Hands nothing over, whatever reads it next: the strided kernels have no RMS_norm epilogue."""
        conv = self._convs[name + ".resample.1"]
        tc = self._convs[name + ".time_conv"] if mode == "down3d" else None
        if tc is None or not tc.started:
            y = ops.conv_cl_down(x, conv.w, conv.b, conv.geo)
            return (y if tc is None else tc.skip(y)), None
        s = tc.input(x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.device)
        ops.conv_cl_down(x, conv.w, conv.b, conv.geo, out=s.new)
        return tc(s), None

    def _encoder_step(self, px, channel_dim: int):   # the pixel front end, Encoder3d.forward (vae.py:318-366), conv1's mu rows
        c1, mu = self._convs["encoder.conv1"], self._convs["conv1"]
        if px.dtype == torch.uint8:                 # video frames [T, H, W, 3]: normalised, rounded and laid out by one kernel
            s = c1.input(px.shape[0], px.shape[1], px.shape[2], px.device)
            ops.pixels_u8_to_cl(px, self.cpad, out=s.new)
        else:
            s = c1.input(px.shape[1 - channel_dim], px.shape[2], px.shape[3], px.device)
            ops.pixels_to_cl(px, channel_dim, self.cpad, out=s.new)
        x, staged = self._conv_handoff(c1, s, self._consumer(-1))
        return mu(mu.stage(self._walk(x, staged)))  # [T', h, w, z_dim]

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

    def _decode(self, latent: torch.Tensor, use_cache: bool, frames: str, yuv_range: str) -> torch.Tensor:
        """`frames` / `yuv_range` are the model's to check (WanVAEDecoderHIP.decode reads the range for "yuv420" alone)."""
        if latent.dtype != bf16:
            latent = latent.to(bf16)
        if use_cache:      # ONE streaming feature cache: a second sample would continue the first one's stream
            assert latent.shape[0] == 1, "Batch size must be 1 when using cache"          # utils/wan_wrapper.py:99
        return torch.stack([self.model.decode(u, keep_cache=use_cache, frames=frames, yuv_range=yuv_range) for u in latent], 0)

    def decode_to_pixel(self, latent: torch.Tensor, use_cache: bool = False) -> torch.Tensor:
        return self._decode(latent, use_cache, "float", "limited")

    def decode_to_frames(self, latent: torch.Tensor, use_cache: bool = False, frames: str = "uint8",
                         yuv_range: str = "limited") -> torch.Tensor:
        """latent [B, T, 16, h, w] -> video frames uint8 [B, T', H, W, 3]: bit for bit
        `(255.0 * (decode_to_pixel(latent, use_cache) * 0.5 + 0.5).clamp(0, 1).permute(0, 1, 3, 4, 2)).to(torch.uint8)`, without the
        fp32 planes ever existing.  frames="yuv420": those frames as I420, uint8 [B, T', ops.yuv420_bytes(H, W)] in `yuv_range`."""
        if frames not in ("uint8", "yuv420"):
            raise ValueError(f"decode_to_frames: frames={frames!r} is not 'uint8' or 'yuv420'")
        return self._decode(latent, use_cache, frames, yuv_range)

    def _get_encoder(self) -> WanVAEEncoderHIP:
        if self.encoder is None:
            if self._encoder_sd is None:
                raise RuntimeError("WanVAEWrapper.encode_to_latent: no encoder weights were loaded (the state dict held no "
                                   "`encoder.*` / `conv1.*` keys): this VAE is decode-only")
            enc = WanVAEEncoderHIP(self.model.cfg, device=self._device, chunk=self._encode_chunk)
            enc.load_state_dict(self._encoder_sd, strict=False)
            self.encoder = enc
        return self.encoder

    def _encode(self, what: str, x: torch.Tensor, keep_cache: bool, wrong: Optional[str]) -> torch.Tensor:
        if wrong is not None:
            raise RuntimeError(f"{what}: expected {wrong}")
        if not x.is_cuda:
            raise RuntimeError(f"{what}: expected a device tensor (longlive_amd has no CPU path)")
        if keep_cache:
            assert x.shape[0] == 1, "Batch size must be 1 when using cache"
        enc = self._get_encoder()
        return torch.stack([enc.encode(u, keep_cache=keep_cache) for u in x], 0)

    def encode_to_latent(self, pixel: torch.Tensor, keep_cache: bool = False) -> torch.Tensor:
        """utils/wan_wrapper.py:80-94.  keep_cache (not in the reference): continue the stream of the previous call (B = 1)."""
        ok = pixel.dim() == 5 and pixel.shape[1] == 3
        return self._encode("encode_to_latent", pixel, keep_cache, None if ok else f"pixel [B, 3, T, H, W], got {tuple(pixel.shape)}")

    def encode_frames_to_latent(self, frames: torch.Tensor, keep_cache: bool = False) -> torch.Tensor:
        """Video frames uint8 [B, T, H, W, 3] -> fp32 [B, 1 + (T - 1) // 4, 16, H/8, W/8]: bit for bit
        encode_to_latent((frames.float() / 127.5 - 1).permute(0, 4, 1, 2, 3)), without the fp32 planes ever existing."""
        ok = frames.dim() == 5 and frames.shape[4] == 3 and frames.dtype == torch.uint8
        return self._encode("encode_frames_to_latent", frames, keep_cache,
                            None if ok else f"uint8 frames [B, T, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
