"""Data constructions of the VAE-encoder edge suite and their fp64 host references (plain helpers, no tests): the strided gathers on
the exact data of tests/vae_exact.py.

Integer codes -4 .. 4 in the input, integer codes -4 .. 4 under one power of two per output channel in the weights, bias on the 2^-3
grid.  K <= 9 x 384 = 3456, far inside the K <= 10368 for which |any partial sum of code products| <= 16 K < 2^24:
every fp32 sum is exact in any order, so the output has one correct bit pattern -- the fp64 F.conv2d / F.conv3d result plus bias,
rounded to bf16 once.  Channel 0 of every tap carries the tap's own code: no two taps are equal, so a pad on the wrong side or a
stride origin off by one changes the expected integers."""
import torch
import torch.nn.functional as F

import vae_exact as E

bf = torch.bfloat16
K_MAX = 9 * 384


class DownData:
    """kind 0 (ll_conv_cl_down): frames [T, H, W, Cin], w [Cout, Cin, 3, 3];  want [T, H//2, W//2, Cout] = ZeroPad2d((0,1,0,1)) +
    Conv2d(3, stride 2).   kind 1 (ll_conv_cl_tdown): frames [1 + T, H, W, Cin] -- the history frame first --, w [Cout, Cin, 3, 1, 1];
    want [T//2, H, W, Cout] = conv3d(stride (2,1,1)) over them, no padding.
    impulse = (f, h, w): index f into `frames` (for kind 1 f = 0 is the history frame); every other input element is zero."""

    def __init__(self, kind, T, H, W, Cin, Cout, seed=1, impulse=None):
        taps = 3 if kind else 9
        K = taps * Cin
        assert K <= K_MAX and 16 * K < 2 ** 24
        self.kind, self.T, self.H, self.W, self.Cin, self.Cout, self.K = kind, T, H, W, Cin, Cout, K
        self.nh = 1 if kind else 0
        self.To, self.Ho, self.Wo = (T // 2, H, W) if kind else (T, H // 2, W // 2)
        self.M = self.To * self.Ho * self.Wo
        self.Kpad = (K + 63) // 64 * 64
        fr = E._codes((self.nh + T, H, W, Cin), seed)
        self.px = None
        if impulse is not None:
            f, h, w = impulse
            px = ((torch.arange(Cin) * 5) % 9 - 4).double()
            px[px == 0] = 1.0
            fr.zero_()
            fr[f, h, w] = px
            self.px = px
        shape = (Cout, Cin, 3, 1, 1) if kind else (Cout, Cin, 3, 3)
        cw = E._codes(shape, seed + 7)
        cw[:, 0] = (torch.arange(taps) - 4).double().view(shape[2:])              # every tap its own code
        ew = ((torch.arange(Cout) * 5) % 7 - 3).double()
        w = cw * torch.pow(2.0, ew).view(-1, *([1] * (len(shape) - 1)))
        bias = E._codes((Cout,), seed + 13, -8, 8) * 2.0 ** -3
        for t in (fr, w, bias):
            assert torch.equal(t.to(bf).double(), t)
        self.frames, self.w, self.bias = fr, w, bias
        self.acc = down_host(kind, fr, w)
        raw = self.acc + bias
        assert raw.abs().max() < 2 ** 21 and torch.equal(raw.float().double(), raw)   # multiples of 2^-3 below 2^24 2^-3: exact in fp32
        self.want = raw.float().to(bf)

    def packed_w(self):
        """[Cout, Kpad] bf16 with k = tap Cin + ci, zero padded (ops.pack_conv_weight's layout)."""
        p = torch.zeros(self.Cout, self.Kpad, dtype=bf)
        w = self.w if self.kind else self.w.unsqueeze(2)
        p[:, :self.K] = w.permute(0, 2, 3, 4, 1).reshape(self.Cout, self.K).to(bf)
        return p


def down_host(kind, frames, w, pad=(0, 1, 0, 1), origin=0):
    """fp64, channels-last result.  The mutations of the host proof: pad = (1, 0, 1, 0) puts the zero row / column on the left / top;
    origin = 1 starts the temporal stride one frame late."""
    x = frames.permute(0, 3, 1, 2)                                               # [F, Cin, H, W]
    if kind == 0:
        return F.conv2d(F.pad(x, pad), w, stride=2).permute(0, 2, 3, 1).contiguous()
    y = F.conv3d(x.permute(1, 0, 2, 3)[None, :, origin:], w, stride=(2, 1, 1))    # [1, Cout, To, H, W]
    return y[0].permute(1, 2, 3, 0).contiguous()
