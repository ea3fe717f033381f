"""Attention kernels that emit the codes + E8M0 scales their output projections read (ops.flash_attn / flash_attn_mx with out_fmt;
ll_flash_attn_q, ll_flash_attn_mx_q): bit for bit the quantiser applied to the bf16 kernel's rows on the same route, nothing written
outside the rows' own bytes, the two-launch path where the generated kernel does not cover the call, and the model with the fusion on
against the model with it off."""
import contextlib

import numpy as np
import pytest
import torch

from attn_qout_exact import hash_qkv as _qkv
from longlive_amd import _lib, synth
from util import bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0xA5                        # neither 0 nor 127
FMTS = ["mx", "mx6", "mx4"]
QID = {"mx": 1, "mx6": 2, "mx4": 3}
BITS = {"mx": 8, "mx6": 6, "mx4": 4}
MX_MODES = ["mxfp8", "mxfp6", "mxfp4_a6", "mxfp4_a4"]


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as O
    return O


def _fmt(ops, name):
    return {"mx": ops.MX, "mx6": ops.MX6, "mx4": ops.MX4}[name]


def hn(name, shape, scale=1.0):
    return (scale * synth.hash_normal(151, name, shape)).to(bf).to(DEV)


@contextlib.contextmanager
def tuning(key, value, default):
    lib = _lib.load()
    assert lib.ll_set_tuning(key.encode(), value) == 0
    try:
        yield
    finally:
        lib.ll_set_tuning(key.encode(), default)


@contextlib.contextmanager
def timed(ops):
    ops.timer = ops.KernelTimer()
    try:
        yield ops.timer
    finally:
        ops.timer = None


def _u8(t):
    return t.view(torch.uint8)


def _same(got, want, what):
    assert torch.equal(_u8(got[1]).reshape(-1), _u8(want[1]).reshape(-1)), what + ": scales"
    assert torch.equal(_u8(got[0]).reshape(-1), _u8(want[0]).reshape(-1)), what + ": codes"


def _raw_q(lib, fmt, q, k, v, segs, scale=None):
    """ll_flash_attn_q into sentinel-filled buffers whose row strides are 16 / 4 bytes wider than the rows and which have two rows to
    spare: -> (codes, scales) of the rows, after checking that every other byte still holds the sentinel"""
    B, Lq, H, D = q.shape
    Sk = k.shape[1]
    (s0, e0), (s1, e1) = segs[0], (segs[1] if len(segs) > 1 else (0, 0))
    wc, ws = H * 16 * BITS[fmt], H * 4
    codes = torch.full((B * Lq + 2, wc + 16), SENT, dtype=torch.uint8, device=DEV)
    scales = torch.full((B * Lq + 2, ws + 4), SENT, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ll_flash_attn_q(QID[fmt], q.data_ptr(), k.data_ptr(), v.data_ptr(), codes.data_ptr(), scales.data_ptr(), B, Lq, H,
                                   H * D, wc + 16, ws + 4, H * D, Sk * H * D, s0, e0 - s0, s1, e1 - s1, scale or 128 ** -0.5,
                                   torch.cuda.current_stream().cuda_stream), "ll_flash_attn_q")
    assert (codes[B * Lq:] == SENT).all() and (codes[:, wc:] == SENT).all(), "codes written outside the rows"
    assert (scales[B * Lq:] == SENT).all() and (scales[:, ws:] == SENT).all(), "scales written outside the rows"
    return codes[: B * Lq, :wc].contiguous(), scales[: B * Lq, :ws].contiguous()


SHAPES = {                         # B, H, Lq, key ranges, attn_asm_min_keys
    "smallest_default_range": (1, 2, 72, [(3, 515)], 512),
    "adjacent_ranges_two_qtiles": (2, 4, 300, [(0, 192), (192, 792)], 512),
    "two_tile_minimum": (1, 2, 64, [(0, 128)], 128),
    "odd_heads": (1, 3, 72, [(0, 512)], 512),
}


@pytest.fixture(scope="module")
def bf16_rows(ops):
    """q, k, v and the bf16 kernel's rows per shape: computed once, shared by the formats"""
    cache = {}

    def get(name):
        if name not in cache:
            B, H, Lq, segs, min_keys = SHAPES[name]
            q, k, v = _qkv(name, B, Lq, H, segs[-1][1])
            with tuning("attn_asm_min_keys", min_keys, 512):
                cache[name] = (q, k, v, ops.flash_attn(q, k, v, segs).view(B, Lq, H * 128))
        return cache[name]
    return get


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fmt", FMTS)
def test_generated_kernel_writes_the_quantiser_bytes(ops, bf16_rows, fmt, shape):
    B, H, Lq, segs, min_keys = SHAPES[shape]
    if H % 2 and fmt != "mx":
        assert not ops.flash_attn_q_ok(_fmt(ops, fmt), H, segs)          # the packed formats pair heads: two launches (tested below)
        return
    q, k, v, rows = bf16_rows(shape)
    want = getattr(ops, "quantize_" + fmt)(rows)
    with tuning("attn_asm_min_keys", min_keys, 512):
        assert ops.flash_attn_q_ok(_fmt(ops, fmt), H, segs)
        _same(_raw_q(_lib.load(), fmt, q, k, v, segs), want, f"{fmt} {shape} (C ABI)")
        with timed(ops) as t:
            got = ops.flash_attn(q, k, v, segs, out_fmt=_fmt(ops, fmt), tag="flash_attn_self")
        torch.cuda.synchronize()
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[0].dtype == want[0].dtype
    _same(got, want, f"{fmt} {shape}")
    assert set(t.records) == {"flash_attn_self"}, set(t.records)          # one launch, under the attention's tag


@pytest.mark.parametrize("fmt", FMTS)
def test_edge_values_through_one_hot_rows(ops, fmt):
    """tests/attn_qout_emu.py's construction (every output row is a chosen V row: all-zero blocks, amax at, one ulp above
    and below the largest code, ties, values that round to the smallest subnormal code and to zero, a block whose exponent clamps
    at -127, one row of halved values) on the device."""
    from attn_qout_emu import one_hot_case
    qb, kb, vb, rows, nkeys, pos = one_hot_case(fmt)

    def t(bits):
        return torch.from_numpy(bits.view(np.int16).copy()).view(bf).unsqueeze(0).to(DEV)
    q, k, v = t(qb), t(kb), t(vb)
    segs = [(3, 3 + nkeys)]
    with tuning("attn_asm_min_keys", 128, 512):
        out = ops.flash_attn(q, k, v, segs)
        assert torch.equal(out[0, 1:, 1], v[0, 3 + torch.from_numpy(pos[1:rows].copy()), 1]), "the output rows are not the chosen V rows"
        want = getattr(ops, "quantize_" + fmt)(out.view(1, rows, 256))
        got = _raw_q(_lib.load(), fmt, q, k, v, segs)
    assert (want[1] == 127).any() and (want[1] == 0).any()               # an all-zero block and a clamped exponent occur
    _same(got, want, f"{fmt} one-hot rows")


@pytest.mark.parametrize("fmt", FMTS)
def test_uncovered_ranges_take_two_launches_with_the_same_bytes(ops, fmt):
    B, H, Lq, segs = 1, 2, 72, [(0, 64), (128, 640)]
    q, k, v = _qkv("gap", B, Lq, H, 640)
    assert not ops.flash_attn_q_ok(_fmt(ops, fmt), H, segs)
    want = getattr(ops, "quantize_" + fmt)(ops.flash_attn(q, k, v, segs).view(B, Lq, H * 128))
    with timed(ops) as t:
        got = ops.flash_attn(q, k, v, segs, out_fmt=_fmt(ops, fmt))
    torch.cuda.synchronize()
    _same(got, want, f"{fmt} non-adjacent ranges")
    assert set(t.records) == {"flash_attn", "quantize_" + fmt}, set(t.records)
    if fmt != "mx":                                        # odd H with a packed format: the same
        q3, k3, v3 = _qkv("odd", 1, 72, 3, 512)
        with pytest.raises(AssertionError):                # ... and such a row (384 channels) is no whole super-block either
            ops.flash_attn(q3, k3, v3, [(0, 512)], out_fmt=_fmt(ops, fmt))
    lib = _lib.load()
    cd, sc = _fmt(ops, fmt).empty((B, Lq, H * 128), DEV)
    rc = lib.ll_flash_attn_q(QID[fmt], q.data_ptr(), k.data_ptr(), v.data_ptr(), cd.data_ptr(), sc.data_ptr(), B, Lq, H, 256, cd.shape[-1],
                             8, 256, 640 * 256, 0, 64, 128, 512, 128 ** -0.5, torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and "not covered" in lib.ll_last_error().decode()      # the entry point refuses, it does not fall back


# ---- MXFP8 attention over the shadow -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,Lq,S,segs", [(2, 2, 150, 157, [(0, 40), (70, 157)]), (1, 2, 32, 37, [(5, 37)])])
@pytest.mark.parametrize("fmt", FMTS)
def test_mx_attention_writes_the_quantiser_bytes(ops, fmt, B, H, Lq, S, segs):
    q, k, v = _qkv(f"mxa{Lq}", B, Lq, H, S)
    shadow = ops.kv_shadow_mx_alloc(k)
    ops.kv_shadow_mx(k, v, shadow, 0, S)
    want = getattr(ops, "quantize_" + fmt)(ops.flash_attn_mx(q, shadow, segs).view(B, Lq, H * 128))
    with timed(ops) as t:
        got = ops.flash_attn_mx(q, shadow, segs, out_fmt=_fmt(ops, fmt))
    torch.cuda.synchronize()
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    _same(got, want, f"{fmt} MX attention Lq={Lq}")
    assert set(t.records) == {"flash_attn_mx"}, set(t.records)
    # the C entry point into wider, sentinel-filled rows
    lib = _lib.load()
    wc, ws = H * 16 * BITS[fmt], H * 4
    codes = torch.full((B * Lq + 2, wc + 16), SENT, dtype=torch.uint8, device=DEV)
    scales = torch.full((B * Lq + 2, ws + 4), SENT, dtype=torch.uint8, device=DEV)
    (s0, e0), (s1, e1) = segs[0], (segs[1] if len(segs) > 1 else (0, 0))
    _lib.check(lib.ll_flash_attn_mx_q(QID[fmt], q.data_ptr(), shadow["kq"].data_ptr(), shadow["ks"].data_ptr(), shadow["vq"].data_ptr(),
                                      shadow["vs"].data_ptr(), codes.data_ptr(), scales.data_ptr(), B, Lq, H, 128, H * 128, wc + 16, ws + 4, S,
                                      shadow["kq"].shape[1], s0, e0 - s0, s1, e1 - s1, 128 ** -0.5, torch.cuda.current_stream().cuda_stream),
               "ll_flash_attn_mx_q")
    assert (codes[B * Lq:] == SENT).all() and (codes[:, wc:] == SENT).all() and (scales[B * Lq:] == SENT).all() and (scales[:, ws:] == SENT).all()
    _same((codes[: B * Lq, :wc].contiguous(), scales[: B * Lq, :ws].contiguous()), want, f"{fmt} MX attention Lq={Lq} (C ABI)")


# ---- model -----------------------------------------------------------------------------------------------------------------------
def _toy(lin, attn_quant):
    """the toy model of tests/test_mx_attn_gpu.py with frames of 128 tokens and 128 text keys, so that under attn_asm_min_keys = 128 the
    generated kernel takes every attention launch of the three cache-filling frames (one key range of 128, 256, 384 slots)"""
    from longlive_amd.wan_wrapper import WanDiffusionWrapper
    cfg = synth.toy_config(local_attn_size=3, sink_size=1, lat_h=16, lat_w=32, text_len=128)
    sd = synth.synth_state_dict(cfg, seed=3)
    gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=3, sink_size=1, cfg=cfg, device=DEV, state_dict=sd)
    S = 3 * cfg.frame_seqlen
    for m in gen.model.modules():
        if hasattr(m, "max_attention_size"):
            m.max_attention_size = S
    gen.model.set_quant(lin).set_attn_quant(attn_quant)
    return cfg, gen, S


def _toy_caches(cfg, S):
    kv = [dict(k=torch.zeros(1, S, cfg.num_heads, 128, dtype=bf, device=DEV), v=torch.zeros(1, S, cfg.num_heads, 128, dtype=bf, device=DEV),
               global_end_index=0, local_end_index=0) for _ in range(cfg.num_layers)]
    ca = [dict(k=torch.zeros(1, cfg.text_len, cfg.num_heads, 128, dtype=bf, device=DEV),
               v=torch.zeros(1, cfg.text_len, cfg.num_heads, 128, dtype=bf, device=DEV), is_init=False) for _ in range(cfg.num_layers)]
    return kv, ca


@pytest.mark.parametrize("lin,attn", [(m, None) for m in MX_MODES] + [("mxfp4_a4", "mxfp8")])
def test_toy_model_is_bit_identical_with_the_fusion_on_and_off(ops, lin, attn):
    cfg, gen, S = _toy(lin, attn)
    assert gen.model.fuse_attn_quant in (True, False)
    fs = cfg.frame_seqlen
    assert fs == 128 and cfg.num_heads % 2 == 0
    noise = synth.synth_noise(cfg, 3, seed=5).to(DEV)
    prompt = synth.synth_prompt_embeds(cfg, seed=7, valid_tokens=9).to(DEV)
    t = torch.full((1, 1), 937.5, device=DEV)
    gen.model._pack()                                      # the weights' quantiser launches happen here, outside the timed forwards
    runs = {}
    try:
        with tuning("attn_asm_min_keys", 128, 512):
            for fuse in (True, False):
                gen.model.fuse_attn_quant = fuse
                kv, ca = _toy_caches(cfg, S)
                x0s = []
                with timed(ops) as tm:
                    for f in range(3):
                        _, x0 = gen(noise[:, f:f + 1], {"prompt_embeds": prompt}, t, kv_cache=kv, crossattn_cache=ca, current_start=f * fs)
                        x0s.append(x0.clone())
                torch.cuda.synchronize()
                runs[fuse] = (x0s, kv, {tag for tag in tm.records if "quantize" in tag}, set(tm.records))
    finally:
        gen.model.set_quant(None).set_attn_quant(None)
    assert runs[True][2] == set(), runs[True][2]           # no quantiser launch is left in a forward
    assert runs[False][2], runs[False][3]
    assert any(tag.startswith("flash_attn") for tag in runs[True][3])
    for a, b in zip(runs[True][0], runs[False][0]):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    for la, lb in zip(runs[True][1], runs[False][1]):
        assert torch.equal(la["k"], lb["k"]) and torch.equal(la["v"], lb["v"])


def test_real_width_block_is_bit_identical_with_the_fusion_on_and_off(ops):
    """dim 1536, 12 heads, three frames (L = 4680) in steady state (roll + insert, keys = [sink | window]) in mxfp4_a4"""
    from longlive_amd.model import CausalWanModelHIP
    from model_runs import kv_fill as _kv_fill
    cfg = synth.longlive_1_3b(num_layers=1)
    fs, S = cfg.frame_seqlen, 12 * cfg.frame_seqlen
    sd = synth.synth_state_dict(cfg, seed=0, device=DEV, layers=[0])
    m = CausalWanModelHIP(cfg, device=DEV)
    m.load_state_dict(sd)
    for mod in m.modules():
        if hasattr(mod, "max_attention_size"):
            mod.max_attention_size = S
    x0 = synth.hash_normal(73, "blk.x", (1, 3 * fs, cfg.dim), device=DEV).to(bf)
    e0 = (0.3 * synth.hash_normal(73, "blk.e0", (1, 3, 6, cfg.dim), device=DEV)).to(bf)
    ctx = synth.hash_normal(73, "blk.ctx", (1, cfg.text_len, cfg.dim), device=DEV).to(bf)
    k, v = _kv_fill(cfg, 0, S)
    m.set_quant("mxfp4_a4")
    m._pack()
    outs = {}
    try:
        for fuse in (True, False):
            m.fuse_attn_quant = fuse
            xs = x0.clone()
            kv = dict(k=k.clone(), v=v.clone(), global_end_index=S, local_end_index=S)
            ca = {"k": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "v": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "is_init": False}
            with timed(ops) as tm:
                m.block_forward(0, xs, e0, ctx, kv, ca, 3, (30, 52), current_start=S)
            torch.cuda.synchronize()
            outs[fuse] = (xs, kv, {tag for tag in tm.records if "quantize" in tag})
    finally:
        m.set_quant(None)
    assert outs[False][2] and not outs[True][2], (outs[True][2], outs[False][2])
    assert torch.isfinite(outs[True][0].float()).all() and torch.equal(outs[True][0], outs[False][0])
    assert torch.equal(outs[True][1]["k"], outs[False][1]["k"]) and torch.equal(outs[True][1]["v"], outs[False][1]["v"])
