"""uint8 video intake (csrc/conv.hip: ll_pixels_u8_to_cl) against the CPU expression it is specified by,
`(u.float() / 127.5 - 1).to(torch.bfloat16)`, bit for bit: every byte value in every channel, one pixel, widths that are no multiple
of a lane's 4-pixel group, a tail lane, more than one workgroup, dword-aligned and unaligned frame bases behind a frame stride larger
than the frame, all three channel paddings; guards around input and output.  Then the encoder fed with frames against the encoder fed
with the fp32 planes."""
import pytest
import torch

import vae_enc_ref as ER
from longlive_amd import synth
from util import bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = 0x7FC1                            # a NaN pattern no kernel produces
GUARD = 0x5A                              # input guard byte: as a pixel it would give 90 / 127.5 - 1, never NaN
SHAPES = [(1, 1, 1), (2, 1, 5), (1, 3, 7), (3, 8, 12), (1, 16, 33)]
# a lane owns 4 pixels and a workgroup 256 lanes: 2 x 24 x 43 is 258 groups per frame (the first frame ends inside the second
# workgroup), 516 lanes in 3 workgroups, the last one partly idle
SHAPES.append((2, 24, 43))


def _frames(T, H, W):
    """uint8 [T, H, W, 3]: along the pixels of a frame channel c steps by an odd number, so any 256 consecutive pixels hold every
    byte value in every channel."""
    p = torch.arange(H * W, dtype=torch.int64).view(1, H, W, 1)
    t = torch.arange(T, dtype=torch.int64).view(T, 1, 1, 1)
    mult = torch.tensor([1, 7, 13], dtype=torch.int64).view(1, 1, 1, 3)
    add = torch.tensor([0, 85, 170], dtype=torch.int64).view(1, 1, 1, 3)
    return ((p * mult + add + 11 * t) % 256).to(torch.uint8)


def _want(frames):
    return (frames.float() / 127.5 - 1).to(torch.bfloat16)


def _view(frames, offset, gap):
    """`frames` as a device view whose first byte sits `offset` bytes into a guard-filled buffer, frames `gap` bytes apart."""
    T, H, W, _ = frames.shape
    fb = H * W * 3
    st = fb + gap
    buf = torch.full((offset + T * st + 16,), GUARD, dtype=torch.uint8)
    for t in range(T):
        buf[offset + t * st: offset + t * st + fb] = frames[t].reshape(-1)
    buf = buf.to(DEV)
    v = torch.as_strided(buf, (T, H, W, 3), (st, 3 * W, 3, 1), storage_offset=offset)
    assert torch.equal(v.cpu(), frames)
    return buf, v, st


@pytest.mark.parametrize("offset,gap", [(16, 5), (13, 5), (16, 0)], ids=["aligned_then_not", "unaligned_first", "dense"])
@pytest.mark.parametrize("cpad", [8, 16, 32])
@pytest.mark.parametrize("T,H,W", SHAPES)
def test_pixels_u8_to_cl_bit_exact(T, H, W, cpad, offset, gap):
    from longlive_amd import _lib as L, ops as O
    frames = _frames(T, H, W)
    if H * W >= 256:                                      # the data: every byte value in every channel; 0 -> -1 and 255 -> +1 exactly
        assert all(torch.equal(torch.unique(frames[..., c]), torch.arange(256, dtype=torch.uint8)) for c in range(3))
        assert float(_want(frames)[frames == 0].max()) == -1.0 and float(_want(frames)[frames == 255].min()) == 1.0
    buf, view, st = _view(frames, offset, gap)
    assert view.data_ptr() % 4 == offset % 4 and st == H * W * 3 + gap
    before, G = buf.clone(), 1
    out = torch.full((G + T + G, H, W, cpad), NAN16, dtype=torch.int16, device=DEV)
    L.check(L.load().ll_pixels_u8_to_cl(view.data_ptr(), st, out[G:].data_ptr(), T, H, W, cpad, O._stream()), "ll_pixels_u8_to_cl")
    got = out.cpu()
    assert bool((got[:G] == NAN16).all()) and bool((got[G + T:] == NAN16).all()), "guard frames were written"
    body = got[G:G + T]
    assert torch.equal(body[..., :3].contiguous().view(bf), _want(frames))
    assert bool((body[..., 3:] == 0).all()), "pad channels must be +0"
    assert torch.equal(buf, before)                                          # the input is left alone


def test_ops_wrapper_takes_views_and_copies_what_it_must():
    from longlive_amd import ops as O
    frames = _frames(3, 8, 12)
    _, view, _ = _view(frames, 13, 7)
    want = _want(frames)
    got = O.pixels_u8_to_cl(view, 16)
    assert got.shape == (3, 8, 12, 16) and got.dtype == bf
    assert torch.equal(got[..., :3].cpu(), want) and bool((got[..., 3:] == 0).all())
    assert torch.equal(O.pixels_u8_to_cl(view[1:2])[..., :3].cpu(), want[1:2])
    assert torch.equal(O.pixels_u8_to_cl(frames.to(DEV)[:, :, ::2])[..., :3].cpu(), want[:, :, ::2])      # pixels not contiguous: copied first
    with pytest.raises(RuntimeError, match="expected uint8"):
        O.pixels_u8_to_cl(frames.to(DEV).float())


@pytest.fixture(scope="module")
def vae():
    from longlive_amd.vae import WanVAEWrapper
    cfg = synth.VaeConfig()
    sd = dict(synth.synth_vae_state_dict(cfg, seed=5))
    sd.update(synth.synth_vae_encoder_state_dict(cfg, seed=ER.ENC_SEED))
    m = WanVAEWrapper(device=DEV, chunk=2)
    m.load_state_dict(sd)
    return m


def test_encoding_frames_equals_encoding_their_fp32_planes(vae):
    g = torch.Generator().manual_seed(17)
    f = torch.randint(0, 256, (1, 9, 64, 96, 3), dtype=torch.uint8, generator=g)
    planes = (f.float() / 127.5 - 1).permute(0, 4, 1, 2, 3)
    want = vae.encode_to_latent(planes.to(DEV))
    fd = f.to(DEV)
    got = vae.encode_frames_to_latent(fd)
    assert got.dtype == torch.float32 and got.shape == (1, 3, 16, 8, 12)
    assert torch.equal(got, want)
    a = vae.encode_frames_to_latent(fd[:, :5], keep_cache=True)             # 1 + 4 | 4 with kept caches
    b = vae.encode_frames_to_latent(fd[:, 5:], keep_cache=True)
    vae.encoder.clear_cache()
    assert a.shape[1] == 2 and b.shape[1] == 1 and torch.equal(torch.cat([a, b], 1), want)
    assert torch.equal(vae.encode_frames_to_latent(fd[:, :7]), want[:, :2])  # frames beyond 1 + 4k are dropped, as for planes
    with pytest.raises(RuntimeError, match="uint8 frames"):
        vae.encode_frames_to_latent(fd[0])
