"""The assembled VAE encoder (longlive_amd/vae.py: WanVAEEncoderHIP behind WanVAEWrapper.encode_to_latent) against the goldens the
reference itself produced (tests/golden/vae_encode.pt; tests/vae_enc_ref.py reproduces them bit for bit on the CPU), its streaming and
chunking identities, state-dict routing, the round trip through the decoder, and one call at the real size."""
import pytest
import torch

import vae_enc_ref as ER
from conftest import load_golden
from longlive_amd import synth
from util import bf, cosine, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _both_halves(cfg=None):
    cfg = cfg or synth.VaeConfig()
    sd = dict(synth.synth_vae_state_dict(cfg, seed=5))
    sd.update(synth.synth_vae_encoder_state_dict(cfg, seed=ER.ENC_SEED))
    return sd


@pytest.fixture(scope="module")
def vae():
    from longlive_amd.vae import WanVAEWrapper
    m = WanVAEWrapper(device=DEV, chunk=2)
    missing, unexpected = m.load_state_dict(_both_halves())
    assert not missing and all(k.startswith(("encoder.", "conv1.")) for k in unexpected)
    return m


@pytest.fixture(scope="module")
def t9(vae):
    """The one-shot T = 9 encode, computed once and left unchanged."""
    return vae.encode_to_latent(ER.case_pixels("t9").to(DEV))


@pytest.mark.parametrize("tag", ["t1", "t9", "t6", "b2"])
def test_encode_matches_reference_golden(vae, tag):
    """Per-forward bound of the project: rel-L2 <= 3e-2 and cosine >= 0.9995 against the reference's own output."""
    want = load_golden("vae_encode.pt")[tag].float()
    got = vae.encode_to_latent(ER.case_pixels(tag).to(DEV))
    assert got.dtype == torch.float32 and got.shape == want.shape
    err, cs = rel_l2(got.cpu(), want), cosine(got.cpu(), want)
    print(f"vae encode {tag}: rel-L2 {err:.3e} cosine {cs:.6f}")
    assert err <= 3e-2 and cs >= 0.9995


def test_fp32_pixels_are_rounded_once(vae, t9):
    px = ER.case_pixels("t9")
    assert torch.equal(vae.encode_to_latent(px.float().to(DEV)), t9)            # bf16-exact values: the same bits either way


def test_streaming_with_kept_caches_is_bit_identical(vae, t9):
    px = ER.case_pixels("t9").to(DEV)
    vae.encoder.clear_cache()
    a = vae.encode_to_latent(px[:, :, :5], keep_cache=True)
    b = vae.encode_to_latent(px[:, :, 5:], keep_cache=True)
    vae.encoder.clear_cache()
    assert a.shape == (1, 2, 16, 8, 12) and b.shape == (1, 1, 16, 8, 12)
    assert torch.equal(torch.cat([a, b], 1), t9)


def test_chunk_4_and_8_are_bit_identical(vae, t9):
    assert vae.encoder.chunk == 4
    vae.encoder.chunk = 8
    try:
        got = vae.encode_to_latent(ER.case_pixels("t9").to(DEV))
    finally:
        vae.encoder.chunk = 4
    assert torch.equal(got, t9)                                                # a pixel's K order does not depend on M


def test_t6_equals_t5_and_b2_equals_two_b1(vae):
    p6 = ER.case_pixels("t6").to(DEV)
    assert torch.equal(vae.encode_to_latent(p6), vae.encode_to_latent(p6[:, :, :5]))
    p2 = ER.case_pixels("b2").to(DEV)
    both = vae.encode_to_latent(p2)
    assert both.shape == (2, 2, 16, 8, 12)
    assert torch.equal(both[:1], vae.encode_to_latent(p2[:1])) and torch.equal(both[1:], vae.encode_to_latent(p2[1:]))


def test_cpad_8_and_32_agree_within_the_bound(vae, t9):
    """encoder.conv1 on the generic path (Cpad 8, RMS_norm as its own launch) against the shipped halo path (Cpad 32, fused): other
    fp32 summation orders, the same bound."""
    from longlive_amd.vae import WanVAEEncoderHIP
    e8 = WanVAEEncoderHIP(device=DEV, cpad=8)
    e8.load_state_dict(synth.synth_vae_encoder_state_dict(synth.VaeConfig(), seed=ER.ENC_SEED))
    got = e8.encode(ER.case_pixels("t9")[0].to(DEV))[None]
    want = load_golden("vae_encode.pt")["t9"].float()
    assert rel_l2(got.cpu(), want) <= 3e-2 and cosine(got.cpu(), want) >= 0.9995
    assert rel_l2(got, t9) <= 3e-2


def test_decoder_only_state_dict_decodes_and_refuses_to_encode():
    from longlive_amd.vae import WanVAEWrapper
    m = WanVAEWrapper(device=DEV, chunk=2)
    m.load_state_dict(synth.synth_vae_state_dict(synth.VaeConfig(), seed=5))
    lat = synth.hash_normal(55, "vae.latent", (1, 2, 16, 8, 12)).to(bf).to(DEV)
    out = m.decode_to_pixel(lat)
    assert out.shape == (1, 5, 3, 64, 96) and bool(torch.isfinite(out).all())
    assert m.encoder is None                                                   # nothing allocated for the half that was not asked for
    with pytest.raises(RuntimeError, match="no encoder weights"):
        m.encode_to_latent(ER.case_pixels("t1").to(DEV))
    with pytest.raises(RuntimeError, match="encoder keys missing"):
        m.load_state_dict(dict(synth.synth_vae_state_dict(synth.VaeConfig(), seed=5), **{"conv1.bias": torch.zeros(32)}))


def test_host_pixels_are_refused(vae):
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae.encode_to_latent(ER.case_pixels("t1"))
    with pytest.raises(RuntimeError, match=r"\[B, 3, T, H, W\]"):
        vae.encode_to_latent(ER.case_pixels("t1")[0].to(DEV))


def test_round_trip_shape_and_finite(vae):
    px = ER.case_pixels("b2").to(DEV)                                          # [2, 3, 5, 64, 96]
    lat = vae.encode_to_latent(px)
    out = vae.decode_to_pixel(lat)
    assert out.shape == (2, 5, 3, 64, 96) and bool(torch.isfinite(out).all())  # random weights: no fidelity claim


def test_real_size_call_finishes_on_the_halo_kernel(vae):
    """T = 5 at 480 x 832: finite, the right shape, and the 96-channel 3x3x3 launches (encoder.conv1 and the four residual
    convolutions of the full-resolution stage) are planned on the halo-tile kernel.  The time is printed, not asserted."""
    from longlive_amd import ops
    px = (synth.hash_uniform(71, "vae.pixels.real", (1, 3, 5, 480, 832), DEV) * 2.0 - 1.0).to(bf)
    vae.encode_to_latent(px[:, :, :1])                                         # warm-up: packing, code objects
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = vae.encode_to_latent(px)
    e1.record()
    torch.cuda.synchronize()
    print(f"vae encode T=5 @480x832: {e0.elapsed_time(e1):.1f} ms")
    assert out.shape == (1, 2, 16, 60, 104) and bool(torch.isfinite(out).all())
    enc = vae.encoder
    for T in (1, 4):
        assert ops.conv_plan(T, 480, 832, enc._convs["encoder.conv1"].geo, rms=True).startswith("conv_halo_kernel<bias, NCB 6, UP 0, RMS 1>")
        for n in ("encoder.downsamples.0", "encoder.downsamples.1"):
            assert ops.conv_plan(T, 480, 832, enc._convs[n + ".residual.2"].geo, rms=True).startswith("conv_halo_kernel<bias, NCB 6, UP 0, RMS 1>")
            assert ops.conv_plan(T, 480, 832, enc._convs[n + ".residual.6"].geo, res=True).startswith("conv_halo_kernel<bias_res, NCB 6, UP 0")
