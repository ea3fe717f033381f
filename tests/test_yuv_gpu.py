"""Planar YUV on the GPU ("Planar YUV and Y4M"): the three kernels of csrc/yuv.hip against the numpy restatement
(tests/yuv_ref.py), bit for bit -- the arithmetic is integer, so every comparison is torch.equal -- at the sizes where a lane's
2 x 4 strip or 8-pixel run is partial, unaligned or one more than a workgroup covers; the VAE wrapper and both pipelines with
frames="yuv420" against the conversion of their frames="uint8" results."""
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import yuv_ref as R
from longlive_amd import _lib as L
from longlive_amd import synth, y4m

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 0xA5
bf = torch.bfloat16
RANGES = ("limited", "full")
RUN = 8                                                           # pixels of a lane's run (csrc/yuv.hip: YUV_RUN; FWD_RUN is 4)
# 1x1 .. 9x17: odd and even, partial strips; (2, r - 1), (2, r + 1): around one run, for r = 4 and 8; 2 x 1028 and 2 x 2056: 257
# strips or runs, one more than a workgroup covers
SHAPES = [(1, 1), (2, 2), (1, 7), (3, 5), (8, 16), (9, 17), (2, 3), (2, 5), (2, RUN - 1), (2, RUN + 1), (2, 4 * 256 + 4),
          (2, RUN * 256 + RUN)]


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as o
    return o


def _rgb(T, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (T, H, W, 3), dtype=np.uint8)


def _gapped(rows: np.ndarray, lead: int, stride: int):
    """[T, n] bytes as a guard-filled device buffer: 64 + lead guard bytes, T rows `stride` apart, 64 guard bytes; and the offset."""
    T, n = rows.shape
    buf = torch.full((64 + lead + T * stride + 64,), GUARD, dtype=torch.uint8)
    first = 64 + lead
    for t in range(T):
        buf[first + t * stride:first + t * stride + n] = torch.from_numpy(rows[t])
    return buf.to(DEV), first


def _check_guards(buf, first, T, stride, n):
    body = buf[first:first + T * stride].view(T, stride)
    assert bool((body[:, n:] == GUARD).all()) and bool((buf[:first] == GUARD).all()) and bool((buf[first + T * stride:] == GUARD).all())
    return body[:, :n]


# ---- ll_frames_u8_to_yuv420 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("offset,gap", [(0, 0), (1, 5), (2, 0), (3, 7)])
def test_frames_u8_to_yuv420_shapes_strides_and_guards(ops, H, W, offset, gap):
    lib = L.load()
    n = R.yuv420_bytes(H, W)
    for T in (1, 3):
        frames = _rgb(T, H, W, 100 * H + W + T)
        st, ost = 3 * H * W + gap, n + gap
        src, sfirst = _gapped(frames.reshape(T, -1), offset, st)
        other, _ = _gapped(255 - frames.reshape(T, -1), offset, st)
        for rng in RANGES:
            dst = torch.full((64 + offset + T * ost + 64,), GUARD, dtype=torch.uint8, device=DEV)
            first = 64 + offset
            for source in (other, src):                         # the second call finds the first one's bytes in the buffer
                L.check(lib.ll_frames_u8_to_yuv420(source[sfirst:].data_ptr(), st, T, H, W, int(rng == "full"), dst[first:].data_ptr(), ost,
                                                   ops._stream()), "ll_frames_u8_to_yuv420")
            got = _check_guards(dst, first, T, ost, n)
            assert torch.equal(got.cpu(), torch.from_numpy(R.rgb_to_i420(frames, rng))), (T, rng)


def test_frames_u8_to_yuv420_wrapper(ops):
    frames = _rgb(3, 10, 14, 5)
    dev = torch.from_numpy(frames).to(DEV)
    want = torch.from_numpy(R.rgb_to_i420(frames, "limited"))
    assert torch.equal(ops.frames_u8_to_yuv420(dev).cpu(), want)
    big = torch.full((7, R.yuv420_bytes(10, 14)), GUARD, dtype=torch.uint8, device=DEV)
    out = ops.frames_u8_to_yuv420(dev, out=big[1::2])
    assert out.data_ptr() == big[1].data_ptr() and torch.equal(big[1::2].cpu(), want) and bool((big[0::2] == GUARD).all())
    assert torch.equal(ops.frames_u8_to_yuv420(dev[:, :, ::2], "full").cpu(), torch.from_numpy(R.rgb_to_i420(frames[:, :, ::2], "full")))
    y, cb, cr = ops.yuv420_planes(out, 10, 14)
    ry, rcb, rcr = R.rgb_to_planes(frames, "limited")
    assert torch.equal(y.cpu(), torch.from_numpy(ry)) and torch.equal(cb.cpu(), torch.from_numpy(rcb)) and torch.equal(cr.cpu(), torch.from_numpy(rcr))
    with pytest.raises(RuntimeError, match="expected uint8"):
        ops.frames_u8_to_yuv420(dev.float())


# ---- ll_cl_to_yuv420 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldc", [8, 3])
def test_cl_to_yuv420_every_bf16_bit_pattern(ops, ldc):
    i = torch.arange(65536, dtype=torch.int32)
    x = torch.zeros(1, 256, 256, ldc, dtype=torch.int16)
    for c in range(3):                                          # every channel walks all 65 536 patterns, NaNs and infinities included
        x[0, :, :, c] = ((i + 20001 * c) & 0xFFFF).to(torch.int16).view(256, 256)
    x = x.view(bf).to(DEV)
    u8 = ops.cl_to_frames_u8(x)
    for rng in RANGES:
        got = ops.cl_to_yuv420(x, rng)
        assert got.dtype == torch.uint8 and got.shape == (1, R.yuv420_bytes(256, 256))
        assert torch.equal(got, ops.frames_u8_to_yuv420(u8, rng))
        assert torch.equal(got.cpu(), torch.from_numpy(R.rgb_to_i420(u8.cpu().numpy(), rng)))


@pytest.mark.parametrize("ldc", [3, 8, 16])
@pytest.mark.parametrize("T,H,W", [(1, 1, 1), (2, 3, 5), (3, 9, 17), (1, 2, RUN * 256 + RUN)])
def test_cl_to_yuv420_shapes_and_guards(ops, T, H, W, ldc):
    g = torch.Generator().manual_seed(1000 * T + 10 * W + ldc)
    x = (torch.randn(T, H, W, ldc, generator=g) * 0.8).to(bf).to(DEV)
    u8 = ops.cl_to_frames_u8(x).cpu().numpy()
    n, gap = R.yuv420_bytes(H, W), 3
    for rng in RANGES:
        dst = torch.full((64 + 1 + T * (n + gap) + 64,), GUARD, dtype=torch.uint8, device=DEV)
        L.check(L.load().ll_cl_to_yuv420(x.data_ptr(), T, H, W, ldc, int(rng == "full"), dst[65:].data_ptr(), n + gap, ops._stream()),
                "ll_cl_to_yuv420")
        assert torch.equal(_check_guards(dst, 65, T, n + gap, n).cpu(), torch.from_numpy(R.rgb_to_i420(u8, rng)))
    with pytest.raises(RuntimeError, match="bfloat16"):
        ops.cl_to_yuv420(x.float())


# ---- ll_yuv_to_frames_u8 ---------------------------------------------------------------------------------------------------------------
def _planes(layout, T, H, W, seed):
    g = np.random.default_rng(seed)
    hc, wc = R.chroma_shape(layout, H, W)
    y = g.integers(0, 256, (T, H, W), dtype=np.uint8)
    if layout == "mono":
        return y, None, None
    return y, g.integers(0, 256, (T, hc, wc), dtype=np.uint8), g.integers(0, 256, (T, hc, wc), dtype=np.uint8)


def _raw_inverse(ops, layout, rng, y, cb, cr, offset, gap):
    """Through the raw entry point: planes `gap` bytes apart behind `offset` odd bytes, the output between guards."""
    T, H, W = y.shape
    hc, wc = R.chroma_shape(layout, H, W)
    sty, stc = H * W + gap, hc * wc + gap
    by, fy = _gapped(y.reshape(T, -1), offset, sty)
    if layout == "mono":
        pcb = pcr = 0
    else:
        bcb, fc = _gapped(cb.reshape(T, -1), offset, stc)
        bcr, _ = _gapped(cr.reshape(T, -1), offset, stc)
        pcb, pcr = bcb[fc:].data_ptr(), bcr[fc:].data_ptr()
    ost = 3 * H * W + gap
    out = torch.full((64 + offset + T * ost + 64,), GUARD, dtype=torch.uint8, device=DEV)
    first = 64 + offset
    L.check(L.load().ll_yuv_to_frames_u8(by[fy:].data_ptr(), pcb, pcr, sty, stc, T, H, W, R.LAYOUTS.index(layout), int(rng == "full"),
                                         out[first:].data_ptr(), ost, ops._stream()), "ll_yuv_to_frames_u8")
    torch.cuda.synchronize()
    return _check_guards(out, first, T, ost, 3 * H * W).reshape(T, H, W, 3).cpu()


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_yuv_to_frames_u8_layouts_shapes_strides_and_guards(ops, layout, H, W):
    for T, offset, gap in ((1, 0, 0), (3, 1, 5), (2, 2, 0), (2, 3, 7)):
        y, cb, cr = _planes(layout, T, H, W, 10 * H + W + T)
        for rng in RANGES:
            got = _raw_inverse(ops, layout, rng, y, cb, cr, offset, gap)
            assert torch.equal(got, torch.from_numpy(R.planes_to_rgb(y, cb, cr, layout, rng))), (T, offset, gap, rng)


@pytest.mark.parametrize("layout", R.LAYOUTS[:5])
@pytest.mark.parametrize("H,W", [(8, 16), (9, 17), (2, RUN + 1)])
def test_yuv_to_frames_u8_impulses_at_the_plane_edges(ops, layout, H, W):
    """One bright chroma sample in the last column and row (where the far index is clamped) and one at (0, 0), on flat planes."""
    hc, wc = R.chroma_shape(layout, H, W)
    y = np.full((2, H, W), 128, np.uint8)
    cb, cr = np.full((2, hc, wc), 128, np.uint8), np.full((2, hc, wc), 128, np.uint8)
    cb[0, hc - 1, wc - 1], cr[0, hc - 1, wc - 1] = 255, 0
    cb[1, 0, 0], cr[1, 0, 0] = 0, 255
    for rng in RANGES:
        want = R.planes_to_rgb(y, cb, cr, layout, rng)
        assert (want[0, -1, -1] != want[0, 0, 0]).any() and (want[1, 0, 0] != want[1, -1, -1]).any()
        got = ops.yuv_to_frames_u8(torch.from_numpy(y).to(DEV), torch.from_numpy(cb).to(DEV), torch.from_numpy(cr).to(DEV), layout, rng)
        assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_yuv_to_frames_u8_takes_the_packed_payloads_of_a_y4m_stream(ops):
    frames = _rgb(3, 9, 17, 8)
    i420 = ops.frames_u8_to_yuv420(torch.from_numpy(frames).to(DEV), "full").cpu().numpy()
    raw = io.BytesIO()
    y4m.write_y4m(raw, iter(i420), 17, 9, range="full")
    reader = y4m.Y4MReader(io.BytesIO(raw.getvalue()))
    payloads = list(reader)
    assert (reader.width, reader.height, reader.layout, reader.range) == (17, 9, "420jpeg", "full")
    buf = torch.frombuffer(bytearray(b"".join(payloads)), dtype=torch.uint8).view(3, -1).to(DEV)
    assert torch.equal(buf.cpu(), torch.from_numpy(i420))
    y, cb, cr = ops.yuv420_planes(buf, 9, 17)
    got = ops.yuv_to_frames_u8(y, cb, cr, reader.layout, reader.range)
    want = R.planes_to_rgb(*R.i420_planes(i420, 9, 17), "420jpeg", "full")
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    big = torch.full((5, 9, 17, 3), GUARD, dtype=torch.uint8, device=DEV)
    ops.yuv_to_frames_u8(y, cb, cr, "420jpeg", "full", out=big[1:4])
    assert torch.equal(big[1:4].cpu(), torch.from_numpy(want)) and bool((big[0] == GUARD).all()) and bool((big[4] == GUARD).all())
    assert torch.equal(ops.yuv_to_frames_u8(y, layout="mono", range="full").cpu(), torch.from_numpy(R.planes_to_rgb(y.cpu().numpy(), None, None, "mono", "full")))
    with pytest.raises(RuntimeError, match="needs both"):
        ops.yuv_to_frames_u8(y, cb, None)


@pytest.mark.parametrize("rng", RANGES)
def test_round_trip_equals_the_restatements(ops, rng):
    """RGB -> I420 -> RGB at 64 x 96 with 420jpeg on a smooth image: the arithmetic is exact, so the GPU's PSNR is the restatement's."""
    yy, xx = np.mgrid[0:64, 0:96].astype(np.float64)
    img = np.stack([127.5 + 127.5 * np.sin(xx / 17.0 + yy / 29.0), 127.5 + 127.5 * np.cos(xx / 23.0 - yy / 13.0),
                    255.0 * (xx + yy) / (95 + 63)], -1).round().astype(np.uint8)[None]
    ref = R.planes_to_rgb(*R.rgb_to_planes(img, rng), "420jpeg", rng)
    i420 = ops.frames_u8_to_yuv420(torch.from_numpy(img).to(DEV), rng)
    got = ops.yuv_to_frames_u8(*ops.yuv420_planes(i420, 64, 96), "420jpeg", rng).cpu().numpy()
    print(f"{rng}: round trip PSNR {R.psnr(got, img):.3f} dB (restatement {R.psnr(ref, img):.3f} dB)")
    assert R.psnr(got, img) == R.psnr(ref, img) and np.array_equal(got, ref)
    assert R.psnr(ref, img) > 30.0                              # a smooth image survives 4:2:0: the reference itself is sane


# ---- wrapper and pipelines -------------------------------------------------------------------------------------------------------------
def to_u8(video):
    return (255.0 * video.permute(0, 1, 3, 4, 2)).to(torch.uint8)


@pytest.fixture(scope="module")
def vae():
    from longlive_amd.vae import WanVAEWrapper
    m = WanVAEWrapper(device=DEV, chunk=2)
    m.load_state_dict(synth.synth_vae_state_dict(synth.VaeConfig(), seed=5))
    return m


@pytest.fixture(scope="module")
def pipe(vae):
    """The shrunk synthetic pipeline of tests/test_frames_out_gpu.py; its float and uint8 results are taken BEFORE the new mode runs."""
    import test_model_gpu as TM
    from longlive_amd.pipeline import CausalInferencePipeline
    cfg, gen, enc = TM._pipe_generator()
    noise = synth.synth_noise(cfg, 9, seed=41, device=DEV)
    P = CausalInferencePipeline(TM._pipe_args(), DEV, generator=gen, text_encoder=enc, vae=vae)

    def reseed():
        P.randn_like = TM.TD.HashRandn(43)
        return P

    video, lat = reseed().inference(noise, ["p0"], return_latents=True)
    frames = reseed().inference(noise, ["p0"], frames="uint8")
    assert torch.equal(frames, to_u8(video))
    return SimpleNamespace(P=P, TM=TM, gen=gen, enc=enc, noise=noise, reseed=reseed, video=video, lat=lat, frames=frames)


def _want(ops, frames_u8, rng):
    return torch.stack([ops.frames_u8_to_yuv420(v, rng) for v in frames_u8], 0)


def test_decode_to_frames_yuv420(ops, vae):
    lat = synth.hash_normal(55, "vae.latent", (1, 5, 16, 8, 12)).to(bf).to(DEV)
    u8 = vae.decode_to_frames(lat, use_cache=False)
    for rng in RANGES:
        got = vae.decode_to_frames(lat, use_cache=False, frames="yuv420", yuv_range=rng)
        assert got.dtype == torch.uint8 and got.shape == (1, 17, R.yuv420_bytes(64, 96)) and torch.equal(got, _want(ops, u8, rng))
        assert torch.equal(got.cpu()[0], torch.from_numpy(R.rgb_to_i420(u8[0].cpu().numpy(), rng)))
    vae.model.clear_cache()
    a = vae.decode_to_frames(lat[:, :2], use_cache=True, frames="yuv420")
    b = vae.decode_to_frames(lat[:, 2:], use_cache=True, frames="yuv420")
    vae.model.clear_cache()
    assert torch.equal(torch.cat([a, b], 1), _want(ops, u8, "limited"))
    assert torch.equal(vae.decode_to_frames(lat, use_cache=False), u8)
    with pytest.raises(ValueError, match="yuv_range"):
        vae.model.decode(lat[0], frames="yuv420", yuv_range="tv")
    with pytest.raises(ValueError, match="frames="):
        vae.decode_to_frames(lat, frames="float")


@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("overlap", [False, True])
def test_pipelines_hand_back_i420_frames(pipe, ops, overlap, rng):
    want = _want(ops, pipe.frames, rng)
    P = pipe.reseed()
    got = [(s, v) for s, v in P.stream_video(pipe.noise, ["p0"], overlap_decode=overlap, frames="yuv420", yuv_range=rng)]
    torch.cuda.synchronize()
    assert [s for s, _ in got] == [0, 3, 6] and [v.shape[1] for _, v in got] == [9, 12, 12]
    assert torch.equal(torch.cat([v for _, v in got], 1), want)
    P = pipe.reseed()
    P.overlap_decode = overlap
    try:
        video, lat = P.inference(pipe.noise, ["p0"], return_latents=True, frames="yuv420", yuv_range=rng)
    finally:
        P.overlap_decode = False
    torch.cuda.synchronize()
    assert video.dtype == torch.uint8 and video.shape == (1, 33, R.yuv420_bytes(64, 96))
    assert torch.equal(video, want) and torch.equal(lat, pipe.lat)


def test_interactive_pipeline_hands_back_i420_frames(pipe, ops, vae):
    from longlive_amd.pipeline import InteractiveCausalInferencePipeline
    P = InteractiveCausalInferencePipeline(pipe.TM._pipe_args(), DEV, generator=pipe.gen, text_encoder=pipe.enc, vae=vae)
    kw = dict(text_prompts_list=[["p0"], ["p1"]], switch_frame_indices=[3])
    P.randn_like = pipe.TM.TD.HashRandn(43)
    u8 = P.inference(pipe.noise, frames="uint8", **kw)
    for overlap in (False, True):
        for rng in RANGES:
            P.randn_like = pipe.TM.TD.HashRandn(43)
            P.overlap_decode = overlap
            got = P.inference(pipe.noise, frames="yuv420", yuv_range=rng, **kw)
            torch.cuda.synchronize()
            assert got.dtype == torch.uint8 and torch.equal(got, _want(ops, u8, rng)), (overlap, rng)
    with pytest.raises(ValueError, match="yuv_range"):
        P.inference(pipe.noise, frames="yuv420", yuv_range="tv", **kw)


def test_the_old_modes_are_unchanged_after_the_new_one_ran(pipe, ops):
    """frames="float" and "uint8" against the calls the fixture made before frames="yuv420" was touched in this process."""
    P = pipe.reseed()
    list(P.stream_video(pipe.noise, ["p0"], overlap_decode=True, frames="yuv420"))
    assert torch.equal(pipe.reseed().inference(pipe.noise, ["p0"], frames="float"), pipe.video)
    assert torch.equal(pipe.reseed().inference(pipe.noise, ["p0"], frames="uint8"), pipe.frames)
    got = torch.cat([v for _, v in pipe.reseed().stream_video(pipe.noise, ["p0"], overlap_decode=True, frames="uint8")], 1)
    torch.cuda.synchronize()
    assert torch.equal(got, pipe.frames)
