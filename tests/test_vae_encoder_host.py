"""Host-side checks of the VAE encoder: the CPU restatement (tests/vae_enc_ref.py) against the goldens the reference itself produced
(tests/golden/vae_encode.pt, tools/make_golden_vae_encode.py) bit for bit; its independence of chunking; the synthetic encoder's
names and shapes; and the new entry points at the C-ABI boundary -- declared, bound, and refusing bad arguments before any launch."""
import ctypes as C
import os
import re

import pytest
import torch

import vae_enc_ref as ER
from conftest import load_golden
from longlive_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ll_conv_cl_down", "ll_conv_cl_tdown", "ll_conv_down_plan", "ll_pixels_to_cl", "ll_vae_scale_tchw")


@pytest.fixture(scope="module")
def golden():
    return load_golden("vae_encode.pt")


@pytest.fixture(scope="module")
def enc():
    return ER.make_encoder()


@pytest.fixture(scope="module")
def ref_t9(enc):
    """The restatement's own T = 9 result at the reference's chunking, computed once."""
    return ER.encode_to_latent(enc, ER.case_pixels("t9"))


# ---- restatement == reference ---------------------------------------------------------------------------------------------------------
def test_golden_is_small_and_holds_outputs_and_seeds_only(golden):
    path = os.path.join(ROOT, "tests", "golden", "vae_encode.pt")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "vae_decode.pt")) and os.path.getsize(path) < 1 << 20
    assert golden["enc_seed"] == ER.ENC_SEED
    assert {k: (v["seed"], tuple(v["shape"])) for k, v in golden["cases"].items()} == ER.CASES
    for tag, (_, (B, _, T, H, W)) in ER.CASES.items():
        assert tuple(golden[tag].shape) == (B, 1 + (T - 1) // 4, 16, H // 8, W // 8), tag


@pytest.mark.parametrize("tag", ["t1", "t6", "b2"])
def test_restatement_equals_the_reference_bit_for_bit(enc, golden, tag):
    got = ER.encode_to_latent(enc, ER.case_pixels(tag))
    assert got.dtype == torch.float32 and torch.equal(got, golden[tag].float()), tag


def test_restatement_equals_the_reference_bit_for_bit_t9(ref_t9, golden):
    assert torch.equal(ref_t9, golden["t9"].float())


def test_frames_beyond_1_plus_4k_are_dropped(enc, golden):
    assert torch.equal(ER.encode_to_latent(enc, ER.case_pixels("t6")[:, :, :5]), golden["t6"].float())


def test_restatement_does_not_depend_on_chunking(enc, ref_t9):
    px = ER.case_pixels("t9")
    assert torch.equal(ER.encode_to_latent(enc, px, chunk=8), ref_t9)
    a = ER.encode_to_latent(enc, px[:, :, :5], keep_cache=True)         # 1 + 4 | 4 with kept caches
    b = ER.encode_to_latent(enc, px[:, :, 5:], keep_cache=True)
    enc.reset()
    assert torch.equal(torch.cat([a, b], 1), ref_t9)


# ---- synthetic encoder ----------------------------------------------------------------------------------------------------------------
def test_encoder_layout_and_names():
    cfg = synth.VaeConfig()
    dims, layers = synth.vae_encoder_layout(cfg)
    assert dims == [96, 96, 192, 384, 384]
    assert [(L[0], L[1]) for L in layers if L[0].startswith("down")] == [("down2d", "encoder.downsamples.2"), ("down3d", "encoder.downsamples.5"),
                                                                        ("down3d", "encoder.downsamples.8")]      # (False, True, True)
    sh = synth.vae_encoder_param_shapes(cfg)
    assert sh["encoder.conv1.weight"] == (96, 3, 3, 3, 3) and sh["conv1.weight"] == (32, 32, 1, 1, 1)
    assert sh["encoder.downsamples.3.shortcut.weight"] == (192, 96, 1, 1, 1) and "encoder.downsamples.4.shortcut.weight" not in sh
    assert sh["encoder.downsamples.2.resample.1.weight"] == (96, 96, 3, 3) and "encoder.downsamples.2.time_conv.weight" not in sh
    assert sh["encoder.downsamples.8.time_conv.weight"] == (384, 384, 3, 1, 1)
    assert sh["encoder.middle.1.to_qkv.weight"] == (1152, 384, 1, 1) and sh["encoder.head.2.weight"] == (32, 384, 3, 3, 3)
    assert not set(sh) & set(synth.vae_decoder_param_shapes(cfg))          # the two halves share no key
    sd = synth.synth_vae_encoder_state_dict(cfg, seed=3)
    assert set(sd) == set(sh) and all(tuple(sd[k].shape) == sh[k] and sd[k].dtype == torch.bfloat16 for k in sh)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "longlive_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 111 == lib.ll_version()
    assert "vae.py:87-94" in header and "vae.py:95-96" in header and "vae.py:537-539" in header      # each cites what it replaces


K96, K192 = 896, 576          # Kpad of 9 x 96 (864 rounded up to 64) and of 3 x 192
PLAN = lambda: C.create_string_buffer(256)


@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_conv_cl_down(1, 1, 1, 1, 1, 1, 1, 8, 96, 96, K96, 96, None), "ll_conv_cl_down: H=1"),
    (lambda L: L.ll_conv_cl_down(1, 1, 1, 1, 1, 1, 8, 1, 96, 96, K96, 96, None), "W=1 must both be >= 2"),
    (lambda L: L.ll_conv_cl_tdown(1, 1, 1, 1, 1, 3, 8, 8, 192, 192, K192, 192, None), "ll_conv_cl_tdown: T=3"),
    (lambda L: L.ll_conv_cl_down(1, 1, 1, 1, 1, 1, 8, 8, 96, 96, K96, 98, None), "ll_conv_cl_down: ldo=98"),
    (lambda L: L.ll_conv_cl_tdown(1, 1, 1, 1, 1, 2, 8, 8, 192, 192, K192, 190, None), "ll_conv_cl_tdown: ldo=190"),
    (lambda L: L.ll_conv_cl_down(1, 1, 1, 1, 1, 1, 8, 8, 96, 96, K96 + 64, 96, None), "ll_conv_cl_down: Kpad=960"),
    (lambda L: L.ll_conv_cl_tdown(1, 1, 1, 1, 1, 2, 8, 8, 192, 192, K96, 192, None), "ll_conv_cl_tdown: Kpad=896"),
    (lambda L: L.ll_conv_cl_down(0, 1, 1, 1, 1, 1, 8, 8, 96, 96, K96, 96, None), "ll_conv_cl_down: null operand"),
    (lambda L: L.ll_conv_cl_tdown(1, 1, 1, 1, 0, 2, 8, 8, 192, 192, K192, 192, None), "ll_conv_cl_tdown: null operand"),
    (lambda L: L.ll_conv_cl_down(1, 1, 1, 1, 1, 1, 8, 8, 100, 96, K96, 96, None), "Cin=100"),
    (lambda L: L.ll_conv_cl_tdown(1, 1, 1, 1, 1, 2, 8, 8, 192, 100, K192, 192, None), "Cout=100"),
    (lambda L: L.ll_conv_down_plan(0, 1, 1, 8, 96, 96, PLAN(), 256), "H=1"),
    (lambda L: L.ll_conv_down_plan(1, 5, 8, 8, 192, 192, PLAN(), 256), "T=5"),
    (lambda L: L.ll_conv_down_plan(2, 4, 8, 8, 192, 192, PLAN(), 256), "kind=2"),
    (lambda L: L.ll_conv_down_plan(0, 1, 8, 8, 96, 96, None, 0), "output buffer"),
    (lambda L: L.ll_pixels_to_cl(0, 1, 64, 192, 1, 1, 8, 8, 8, None), "ll_pixels_to_cl: null operand"),
    (lambda L: L.ll_pixels_to_cl(1, 1, 64, 192, 1, 1, 8, 8, 12, None), "Cpad=12"),
    (lambda L: L.ll_pixels_to_cl(1, 1, 63, 192, 1, 1, 8, 8, 8, None), "strides"),
    (lambda L: L.ll_vae_scale_tchw(1, 1, 0, 1, 1, 16, 8, 8, 16, None), "ll_vae_scale_tchw: null operand"),
    (lambda L: L.ll_vae_scale_tchw(1, 1, 1, 1, 1, 16, 8, 8, 8, None), "z_dim=16 <= ld=8"),
])
def test_bad_arguments_are_rejected_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


def test_conv_down_plan_for_the_shipped_shapes():
    """The three spatial and two temporal down-convolutions of the encoder at 480 x 832, one 4-frame step (what the launcher
    dispatches on: ll_conv_down_plan is built from the same plan struct)."""
    lib = _lib.load()
    buf = C.create_string_buffer(256)

    def plan(*a):
        _lib.check(lib.ll_conv_down_plan(*a, buf, 256), "plan")
        return buf.value.decode()

    assert plan(0, 4, 480, 832, 96, 96) == ("conv_cl_kernel<bias, NT 3, MODE 3> down 4x480x832 -> 4x240x416, tile 256x96, "
                                            "1560 workgroups (1560 m-tiles x 1 n-tiles), 14 k-steps")
    assert plan(0, 4, 240, 416, 192, 192) == ("conv_cl_kernel<bias, NT 3, MODE 3> down 4x240x416 -> 4x120x208, tile 256x96, "
                                              "780 workgroups (390 m-tiles x 2 n-tiles), 27 k-steps")
    assert plan(0, 2, 120, 208, 384, 384) == ("conv_cl_kernel<bias, NT 4, MODE 3> down 2x120x208 -> 2x60x104, tile 256x128, "
                                              "147 workgroups (49 m-tiles x 3 n-tiles), 54 k-steps")
    assert plan(1, 4, 120, 208, 192, 192) == ("conv_cl_kernel<bias, NT 3, MODE 4> tdown 4x120x208 -> 2x120x208, tile 256x96, "
                                              "390 workgroups (195 m-tiles x 2 n-tiles), 9 k-steps")
    assert plan(1, 2, 60, 104, 384, 384) == ("conv_cl_kernel<bias, NT 4, MODE 4> tdown 2x60x104 -> 1x60x104, tile 256x128, "
                                             "75 workgroups (25 m-tiles x 3 n-tiles), 18 k-steps")
    assert plan(0, 1, 2, 2, 64, 8).startswith("conv_cl_kernel<bias, NT 1, MODE 3> down 1x2x2 -> 1x1x1, tile 256x32, 1 workgroups")
    assert plan(0, 1, 5, 4, 16, 64).startswith("conv_cl_kernel<bias, NT 4, MODE 6>")       # Cin < 64: per-lane decode
    assert plan(1, 2, 3, 3, 32, 96).startswith("conv_cl_kernel<bias, NT 3, MODE 5>")


def test_wrapper_and_encoder_refuse_host_tensors_and_bad_chunks():
    from longlive_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pixels_to_cl(torch.zeros(3, 1, 8, 8), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.vae_scale_tchw(torch.zeros(1, 8, 8, 16, dtype=torch.bfloat16), torch.zeros(16, dtype=torch.bfloat16), torch.zeros(16, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.conv_cl_down(torch.zeros(1, 8, 8, 96, dtype=torch.bfloat16), torch.zeros(96, 896, dtype=torch.bfloat16),
                         torch.zeros(96, dtype=torch.bfloat16), (96, 96, 896, 1, 3))
