"""Frames out on the GPU ("Frames out"): ll_cl_to_frames_u8 against the torch chain it replaces, bit for bit;
the JPEG encoder's coefficient stage against the fp64 restatement (tests/jpeg_ref.py), its files byte for byte against the
restatement's entropy coder fed the GPU's own coefficients, and against PIL's decoder and encoder; the VAE wrapper and both pipelines
with frames="uint8" / "jpeg" against the converted float results."""
import functools
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_ref as J
from longlive_amd import _lib as L
from longlive_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 0xA5
bf = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as o
    return o


def to_u8(video):
    """The conversion the uint8 path replaces (cli.py's): [B, T, 3, H, W] in [0, 1] -> uint8 [B, T, H, W, 3]."""
    return (255.0 * video.permute(0, 1, 3, 4, 2)).to(torch.uint8)


def torch_chain(ops, x):
    """channels-last bf16 [T, H, W, C] -> uint8 [T, H, W, 3] through ll_cl_to_tchw_clamp and the torch expressions of the pipelines."""
    v = ops.cl_to_tchw_clamp(x)
    return to_u8(((v * 0.5 + 0.5).clamp(0, 1))[None])[0]


# ---- ll_cl_to_frames_u8 ----------------------------------------------------------------------------------------------------------------
def test_every_bf16_bit_pattern(ops):
    i = torch.arange(65536, dtype=torch.int32)
    x = torch.zeros(1, 256, 256, 8, dtype=torch.int16)
    for c in range(3):                                          # every channel walks all 65 536 patterns, NaNs and infinities included
        x[0, :, :, c] = ((i + 20001 * c) & 0xFFFF).to(torch.int16).view(256, 256)
    x = x.view(bf).to(DEV)
    got = ops.cl_to_frames_u8(x)
    want = torch_chain(ops, x)
    assert got.dtype == torch.uint8 and got.shape == (1, 256, 256, 3)
    assert torch.equal(got, want)
    # NaN: what arithmetic produces is a QUIET NaN, and fminf(fmaxf(NaN, -1), 1) makes it -1, byte 0.  A signalling pattern (quiet bit
    # clear; only a bit cast makes one) leaves the first fmaxf as a quiet NaN and the fminf as +1 in both kernels alike: the equality
    # above covers those 126 patterns, the claim "NaN -> 0" is held for the 128 quiet ones.
    nan = torch.isnan(x[..., :3].float())
    quiet = nan & ((x.view(torch.int16)[..., :3].to(torch.int32) & 0x0040) != 0)
    assert int(nan.sum()) == 3 * 254 and int(quiet.sum()) == 3 * 128 and int(got[quiet].max()) == 0
    assert int(got.max()) == 255 and int(got.min()) == 0


@pytest.mark.parametrize("ldc", [3, 8, 16])
@pytest.mark.parametrize("T,H,W", [(1, 1, 1), (2, 3, 5), (3, 7, 4), (1, 1, 4099)])
@pytest.mark.parametrize("offset,gap", [(0, 0), (1, 5), (2, 0), (3, 7)])
def test_cl_to_frames_u8_shapes_strides_and_guards(ops, T, H, W, ldc, offset, gap):
    g = torch.Generator().manual_seed(1000 * T + 10 * W + ldc)
    x = (torch.randn(T, H, W, ldc, generator=g) * 0.8).to(bf).to(DEV)
    want = torch_chain(ops, x)
    st = 3 * H * W + gap
    buf = torch.full((64 + offset + T * st + 64,), GUARD, dtype=torch.uint8, device=DEV)
    first = 64 + offset
    L.check(L.load().ll_cl_to_frames_u8(x.data_ptr(), buf[first:].data_ptr(), st, T, H, W, ldc, ops._stream()), "ll_cl_to_frames_u8")
    body = buf[first:first + T * st].view(T, st)
    assert torch.equal(body[:, :3 * H * W].reshape(T, H, W, 3), want)
    assert bool((body[:, 3 * H * W:] == GUARD).all()) and bool((buf[:first] == GUARD).all()) and bool((buf[first + T * st:] == GUARD).all())


def test_cl_to_frames_u8_wrapper_writes_into_a_view(ops):
    x = (torch.randn(2, 6, 10, 8, generator=torch.Generator().manual_seed(3)) * 0.8).to(bf).to(DEV)
    big = torch.full((5, 6, 10, 3), GUARD, dtype=torch.uint8, device=DEV)
    out = ops.cl_to_frames_u8(x, out=big[1::2])                 # frames two apart
    assert out.data_ptr() == big[1].data_ptr() and torch.equal(big[1::2], torch_chain(ops, x))
    assert bool((big[0::2] == GUARD).all())
    with pytest.raises(RuntimeError, match="bfloat16"):
        ops.cl_to_frames_u8(x.float())


# ---- the JPEG encoder --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encoded(name: str, quality: int):
    """One case through the raw entry points: frames in a gapped buffer, the output between guards, two calls into one scratch that
    starts as noise.  Computed once and shared by the tests below."""
    from longlive_amd import ops
    lib = L.load()
    frames = J.cases()[name]
    T, H, W, _ = frames.shape
    gap = 7
    st = 3 * H * W + gap
    src = torch.full((T * st,), GUARD, dtype=torch.uint8)
    for t in range(T):
        src[t * st:t * st + 3 * H * W] = torch.from_numpy(frames[t].reshape(-1))
    src = src.to(DEV)
    rows, cols = J.mcu_grid(H, W)
    coef = torch.full((T, rows, cols, 6, 64), 0x5A5A, dtype=torch.int16, device=DEV)
    L.check(lib.ll_jpeg_coefficients_u8(src.data_ptr(), st, T, H, W, quality, coef.data_ptr(), ops._stream()), "coefficients")
    out_stride, scratch_bytes = ops.jpeg_sizes(T, H, W)
    scratch = torch.randint(0, 256, (scratch_bytes,), dtype=torch.uint8, device=DEV, generator=torch.Generator(DEV).manual_seed(7))
    outs = []
    for _ in range(2):                                          # the second call finds the first one's leftovers in scratch
        out = torch.full((T * out_stride + 256,), GUARD, dtype=torch.uint8, device=DEV)
        sizes = torch.full((T + 2,), -1, dtype=torch.int32, device=DEV)
        L.check(lib.ll_jpeg_encode_u8(src.data_ptr(), st, T, H, W, quality, out.data_ptr(), out_stride, sizes.data_ptr(),
                                      scratch.data_ptr(), scratch_bytes, ops._stream()), "encode")
        outs.append((out.cpu().numpy(), sizes.cpu().numpy()))
    return dict(frames=frames, coef=coef.cpu().numpy(), outs=outs, out_stride=out_stride, T=T, H=H, W=W)


CASES = [(n, q) for n in J.cases() for q in J.QUALITIES]


@pytest.mark.parametrize("name,quality", CASES)
def test_coefficients_are_the_rounded_fp64_quotients(name, quality):
    """Every coefficient equals round(fp64 quotient); where the quotient lies within 2^-8 of a tie either neighbour passes.  The band:
    values <= 1024 in magnitude and about 25 fp32 operations of relative error 2^-24 each stay under 1.5e-3 in the worst case, every
    divisor is >= 1, and 2^-8 is 2.6 times that."""
    e = encoded(name, quality)
    for t in range(e["T"]):
        quot = J.quotients(e["frames"][t], quality)
        got = e["coef"][t].astype(np.float64)
        near_tie = np.abs(quot - np.floor(quot) - 0.5) <= 2.0 ** -8
        ok = (got == np.rint(quot)) | (near_tie & ((got == np.floor(quot)) | (got == np.ceil(quot))))
        assert ok.all(), (name, quality, t, int((~ok).sum()), quot[~ok][:4], got[~ok][:4])


@pytest.mark.parametrize("name,quality", CASES)
def test_files_are_the_restatement_of_the_gpu_coefficients_byte_for_byte(name, quality):
    e = encoded(name, quality)
    T, H, W, stride = e["T"], e["H"], e["W"], e["out_stride"]
    assert stride == J.worst_case_bytes(H, W)
    first = None
    for out, sizes in e["outs"]:
        assert (sizes[T:] == -1).all() and (out[T * stride:] == GUARD).all()
        files = []
        for t in range(T):
            want = J.encode_from_coefficients(e["coef"][t], W, H, quality)
            n = int(sizes[t])
            assert n == len(want), (name, quality, t, n, len(want))
            got = out[t * stride:t * stride + n].tobytes()
            assert got == want, (name, quality, t, next(i for i in range(n) if got[i] != want[i]))
            assert (out[t * stride + n:(t + 1) * stride] == GUARD).all()
            files.append(got)
        if first is None:
            first = files
        assert files == first                                   # dirty scratch: the same bytes


def test_the_cases_reach_the_coders_edges():
    """What the GPU files hold, from the restatement's histogram of the GPU's coefficients: FF 00 stuffing, ZRL, DC category 11,
    EOB-only blocks, and a restart count past RST7."""
    def hist(name, quality, t=0):
        e, h = encoded(name, quality), {}
        J.encode_from_coefficients(e["coef"][t], e["W"], e["H"], quality, h)
        return h

    assert hist("23x37_noise", 100).get("ff00", 0) > 0
    assert hist("32x32_pixel_checkerboard", 10).get(("ac", 0xF0), 0) > 0
    assert hist("32x32_block_checkerboard", 100).get(("dc", 11), 0) > 0
    flat = hist("16x16_flat", 90)
    assert [k for k in flat if isinstance(k, tuple) and k[0] == "ac"] == [("ac", 0x00)]
    e = encoded("160x16_smooth", 90)
    out, sizes = e["outs"][0]
    data = out[:int(sizes[0])].tobytes()
    assert [data.count(bytes([0xFF, 0xD0 + m])) >= 1 for m in range(8)] == [True] * 8 and data.endswith(b"\xff\xd9")


@pytest.mark.parametrize("name,quality", CASES)
def test_pil_decodes_the_files_as_well_as_its_own(name, quality):
    Image = pytest.importorskip("PIL.Image")
    e = encoded(name, quality)
    out, sizes = e["outs"][0]
    for t in range(e["T"]):
        src = e["frames"][t]
        im = Image.open(io.BytesIO(out[t * e["out_stride"]:t * e["out_stride"] + int(sizes[t])].tobytes()))
        im.load()
        assert im.size == (e["W"], e["H"]) and im.mode == "RGB"
        b = io.BytesIO()
        Image.fromarray(src).save(b, "JPEG", quality=quality, subsampling=2)
        ours, pil = J.psnr(np.asarray(im), src), J.psnr(np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB")), src)
        print(f"{name} q{quality} frame {t}: ours {ours:.3f} dB, PIL {pil:.3f} dB")
        assert ours >= pil - 0.1, (name, quality, t, ours, pil)


def test_ops_wrappers(ops):
    frames = torch.from_numpy(J.cases()["48x64_x3"]).to(DEV)
    buf, sizes = ops.jpeg_encode(frames, 90)
    files = ops.jpeg_bytes(buf, sizes)
    e = encoded("48x64_x3", 90)
    out, n = e["outs"][0]
    assert files == [out[t * e["out_stride"]:t * e["out_stride"] + int(n[t])].tobytes() for t in range(3)]
    assert torch.equal(ops.jpeg_coefficients(frames, 90).cpu(), torch.from_numpy(e["coef"]))
    assert ops.jpeg_bytes(*ops.jpeg_encode(frames[:, :, ::2], 90)) == ops.jpeg_bytes(*ops.jpeg_encode(frames[:, :, ::2].contiguous(), 90))
    assert ops.jpeg_bytes(*ops.jpeg_encode(frames[1:2], 50))[0] == ops.jpeg_bytes(*ops.jpeg_encode(frames, 50))[1]
    with pytest.raises(RuntimeError, match="quality=0"):
        ops.jpeg_encode(frames, 0)
    with pytest.raises(RuntimeError, match="expected uint8"):
        ops.jpeg_encode(frames.float())


# ---- wrapper and pipelines -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vae():
    from longlive_amd.vae import WanVAEWrapper
    m = WanVAEWrapper(device=DEV, chunk=2)
    m.load_state_dict(synth.synth_vae_state_dict(synth.VaeConfig(), seed=5))
    return m


def test_decode_to_frames_equals_the_converted_pixels(vae):
    lat = synth.hash_normal(55, "vae.latent", (1, 5, 16, 8, 12)).to(bf).to(DEV)
    want = to_u8((vae.decode_to_pixel(lat, use_cache=False) * 0.5 + 0.5).clamp(0, 1))
    got = vae.decode_to_frames(lat, use_cache=False)
    assert got.dtype == torch.uint8 and got.shape == (1, 17, 64, 96, 3) and torch.equal(got, want)
    assert int(got.min()) < 64 and int(got.max()) > 192          # the toy decoder fills the range
    vae.model.clear_cache()
    a = vae.decode_to_frames(lat[:, :2], use_cache=True)
    b = vae.decode_to_frames(lat[:, 2:], use_cache=True)
    vae.model.clear_cache()
    assert torch.equal(torch.cat([a, b], 1), want)
    with pytest.raises(ValueError, match="frames="):
        vae.model.decode(lat[0], frames="int8")


@pytest.fixture(scope="module")
def pipe(vae):
    import test_model_gpu as TM
    from longlive_amd.pipeline import CausalInferencePipeline
    cfg, gen, enc = TM._pipe_generator()
    noise = synth.synth_noise(cfg, 9, seed=41, device=DEV)
    P = CausalInferencePipeline(TM._pipe_args(), DEV, generator=gen, text_encoder=enc, vae=vae)

    def reseed():
        P.randn_like = TM.TD.HashRandn(43)
        return P

    video, lat = reseed().inference(noise, ["p0"], return_latents=True)
    return SimpleNamespace(P=P, TM=TM, gen=gen, enc=enc, noise=noise, reseed=reseed, video=video, lat=lat, frames=to_u8(video))



def test_float_results_are_the_parents_expression(pipe, vae):
    want = (vae.decode_to_pixel(pipe.lat, use_cache=False) * 0.5 + 0.5).clamp(0, 1)
    assert pipe.video.dtype == torch.float32 and torch.equal(pipe.video, want)
    again = pipe.reseed().inference(pipe.noise, ["p0"], frames="float")
    assert torch.equal(again, want)


@pytest.mark.parametrize("overlap", [False, True])
def test_pipelines_hand_back_uint8_frames(pipe, overlap):
    P = pipe.reseed()
    got = [(s, v) for s, v in P.stream_video(pipe.noise, ["p0"], overlap_decode=overlap, frames="uint8")]
    torch.cuda.synchronize()
    assert [s for s, _ in got] == [0, 3, 6] and [v.shape[1] for _, v in got] == [9, 12, 12]
    assert torch.equal(torch.cat([v for _, v in got], 1), pipe.frames)
    P = pipe.reseed()
    P.overlap_decode = overlap
    try:
        video, lat = P.inference(pipe.noise, ["p0"], return_latents=True, frames="uint8")
    finally:
        P.overlap_decode = False
    torch.cuda.synchronize()
    assert video.dtype == torch.uint8 and torch.equal(video, pipe.frames) and torch.equal(lat, pipe.lat)


@pytest.mark.parametrize("overlap", [False, True])
def test_pipelines_hand_back_jpeg_files(pipe, ops, overlap):
    want = ops.jpeg_bytes(*ops.jpeg_encode(pipe.frames[0], 75))
    P = pipe.reseed()
    got = list(P.stream_video(pipe.noise, ["p0"], overlap_decode=overlap, frames="jpeg", jpeg_quality=75))
    assert [s for s, _ in got] == [0, 3, 6] and all(len(v) == 1 for _, v in got)
    assert [f for _, v in got for f in v[0]] == want
    P = pipe.reseed()
    P.overlap_decode = overlap
    try:
        files = P.inference(pipe.noise, ["p0"], frames="jpeg", jpeg_quality=75)
    finally:
        P.overlap_decode = False
    assert files == [want]
    with pytest.raises(ValueError, match="frames"):
        P.inference(pipe.noise, ["p0"], frames="png")
    with pytest.raises(ValueError, match="jpeg_quality"):
        next(P.stream_video(pipe.noise, ["p0"], frames="jpeg", jpeg_quality=0))


def test_interactive_pipeline_hands_back_uint8_frames(pipe, vae):
    from longlive_amd.pipeline import InteractiveCausalInferencePipeline
    P = InteractiveCausalInferencePipeline(pipe.TM._pipe_args(), DEV, generator=pipe.gen, text_encoder=pipe.enc, vae=vae)
    kw = dict(text_prompts_list=[["p0"], ["p1"]], switch_frame_indices=[3])
    P.randn_like = pipe.TM.TD.HashRandn(43)
    want = to_u8(P.inference(pipe.noise, **kw))
    for overlap in (False, True):
        P.randn_like = pipe.TM.TD.HashRandn(43)
        P.overlap_decode = overlap
        got = P.inference(pipe.noise, frames="uint8", **kw)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and torch.equal(got, want), overlap
