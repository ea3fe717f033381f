"""Clip intake on the GPU: the baseline JPEG decoder (csrc/jpeg_dec.hip) and the antialiased resize against tests/jpeg_dec_ref.py, and
the CLI's `input_decode` / `input_fit` keys end to end.  Only well-formed files reach a kernel here; malformed data is the host
program's job (tests/test_clip_gpu_intake_host.py).

Pixel rule (decoder and resize): with v the restatement's unrounded fp64 value, |gpu - byte(v)| <= 1 for every sample, and
gpu == byte(v) wherever v lies more than 2^-8 from a half-integer; the share of samples inside that band is capped where ties are
not the content's nature, so the band cannot hide a failure."""
import functools

import numpy as np
import pytest
import torch

import jpeg_dec_ref as D
import jpeg_ref as J
from longlive_amd import cli, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x7FFF


def _dev(frames):
    return torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)


@functools.lru_cache(maxsize=None)
def _own_files(name, quality):
    """The GPU encoder's files for one case of jpeg_ref.cases()."""
    return tuple(ops.jpeg_bytes(*ops.jpeg_encode(_dev(J.cases()[name]), quality)))


@functools.lru_cache(maxsize=None)
def _pil_files():
    Image = pytest.importorskip("PIL.Image")
    return D.pil_cases(Image)


@functools.lru_cache(maxsize=None)
def _reference(data: bytes):
    """(coefficients int16 [rows, cols, bpm, 64], unrounded fp64 pixels [H, W, 3]) of one file, computed once."""
    info, coef = D.coefficients(data)
    return coef, D.pixels_unrounded(data, coef)


# ---- entropy stage, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", J.QUALITIES)
@pytest.mark.parametrize("name", sorted(J.cases()))
def test_coefficients_are_the_encoders(name, quality):
    frames = _dev(J.cases()[name])
    got = ops.jpeg_decode_coefficients(list(_own_files(name, quality)))
    assert got.dtype == torch.int16 and torch.equal(got, ops.jpeg_coefficients(frames, quality))
    if name == "160x16_smooth":                                  # ten intervals: RST7 is followed by RST0
        assert _own_files(name, quality)[0].count(b"\xff\xd7") >= 1


def _decode_coefficients_guarded(files, dirty=None):
    """The coefficient tensor inside a field of 0x7FFF: (result, buffer, offset); `dirty`: a buffer to decode into again."""
    from longlive_amd import jpeg_files
    pk = jpeg_files.pack_jpegs(files)
    shape = (pk.frames, *pk.grid, 64)
    n, g = int(np.prod(shape)), 192
    buf = torch.full((n + 2 * g,), GUARD, dtype=torch.int16, device=DEV) if dirty is None else dirty
    out = ops.jpeg_decode_coefficients(files, out=buf[g:g + n].view(shape))
    return out, buf, g


def test_pillows_files_decode_to_the_restatements_coefficients():
    """No-DRI files (one lane decodes the whole scan), restart intervals of three blocks, optimised tables and grey; status is all 0
    (check=True raises otherwise); nothing outside the tensor is written, and a second call into the dirty tensor gives it again."""
    for name, data in _pil_files().items():
        want = torch.from_numpy(_reference(data)[0])
        out, buf, g = _decode_coefficients_guarded([data])
        assert torch.equal(out[0].cpu(), want), name
        assert bool((buf[:g] == GUARD).all()) and bool((buf[g + out.numel():] == GUARD).all()), name
        first = out.clone()
        out2, buf2, _ = _decode_coefficients_guarded([data], dirty=buf)
        assert torch.equal(out2, first) and bool((buf2[:g] == GUARD).all()) and bool((buf2[g + out.numel():] == GUARD).all()), name


def test_frames_with_different_tables_decode_in_one_call():
    Image = pytest.importorskip("PIL.Image")
    frames = [J.smooth_noise(37, 53, 1), J.noise(37, 53, 2), J.flat(37, 53), J.smooth_noise(37, 53, 3)]
    kws = [dict(quality=30), dict(quality=95, optimize=True), dict(quality=75, restart_marker_blocks=2), dict(quality=60, optimize=True)]
    for sampling in D.PIL_SAMPLINGS:
        files = [D.pil_file(Image, f, sampling, **kw) for f, kw in zip(frames, kws)]
        got = ops.jpeg_decode_coefficients(files).cpu()
        for t, data in enumerate(files):
            assert torch.equal(got[t], torch.from_numpy(_reference(data)[0])), (sampling, t)
        px = ops.jpeg_decode(files).cpu().numpy()
        for t, data in enumerate(files):
            mx, off, _ = D.band_check(px[t], _reference(data)[1])
            assert mx <= 1 and off == 0, (sampling, t, mx, off)


# ---- pixel stage ----------------------------------------------------------------------------------------------------------------------------
TINY = 1000                                          # samples: below this one sample inside the band is more than 0.1 % of the image


def _band_share(want):
    return D.band_check(D.to_bytes(want), want)[2]


def _pixel_rule(got, want, name, capped=True, cap=0.02):
    """The +-1 / equality rule on one image, and, where `capped`, the cap on the share of its samples inside the band.  Images of
    fewer than TINY samples cannot carry a cap of their own (one of the three samples of a 1 x 1 image is a third of it): theirs is
    on their pooled samples (test_the_band_stays_narrow_on_tiny_images)."""
    mx, off, share = D.band_check(got, want)
    print(f"{name}: max difference {mx}, mismatches outside the band {off}, inside the band {100 * share:.2f} %")
    assert mx <= 1 and off == 0, (name, mx, off)
    if capped and want.size >= TINY:
        assert share <= cap, (name, share)


CAPPED = {"1x1": [True], "8x8_noise": [True], "16x16_flat": [False], "17x33_smooth": [True], "23x37_noise": [True],
          "48x64_x3": [True, True, False], "160x16_smooth": [True], "32x32_pixel_checkerboard": [False],
          "32x32_block_checkerboard": [False]}


@pytest.mark.parametrize("quality", J.QUALITIES)
@pytest.mark.parametrize("name", sorted(J.cases()))
def test_pixels_of_the_encoders_files(name, quality):
    files = list(_own_files(name, quality))
    got = ops.jpeg_decode(files)
    assert got.dtype == torch.uint8 and got.shape == J.cases()[name].shape
    got = got.cpu().numpy()
    for t, data in enumerate(files):
        _pixel_rule(got[t], _reference(data)[1], f"{name}[{t}] q{quality}", capped=CAPPED[name][t])
    if quality == 90 and "smooth" in name and name != "1x1":
        assert J.psnr(got[0], J.cases()[name][0]) > 30.0          # and it is the picture that went in


def test_pixels_of_pillows_files():
    """Every sampling at odd sizes: 17 x 33, 23 x 37 and 37 x 53 pin the component-extent edge rule (the last chroma column / row is
    replicated at ceil(W / 2), ceil(H / 2), not at the MCU padding)."""
    for name, data in _pil_files().items():
        got = ops.jpeg_decode([data])[0].cpu().numpy()
        _pixel_rule(got, _reference(data)[1], name)


def test_the_band_stays_narrow_on_tiny_images():
    """So the band cannot hide a failure: on the smooth and noise contents at most 2 % of the samples lie inside it (checkerboards and
    `flat` are exempt: exact ties are their nature, 12.5 % at quality 10).  Every image of TINY samples or more carries that cap
    itself (_pixel_rule; the restatement alone gives at most 1.6 %).  The 1 x 1 and 8 x 8 images cannot -- Pillow's grey 1 x 1 at
    quality 30 is a tie, 3 of 3 samples, and 8 x 8 noise at quality 90 has 4 of 192 inside, 2.1 % -- so they are capped together:
    11 of 816 samples, 1.3 %."""
    values = [_reference(data)[1] for name in J.cases() for quality in J.QUALITIES
              for t, data in enumerate(_own_files(name, quality)) if CAPPED[name][t]]
    values += [_reference(data)[1] for data in _pil_files().values()]
    tiny = [v for v in values if v.size < TINY]
    inside, total = sum(int(round(_band_share(v) * v.size)) for v in tiny), sum(v.size for v in tiny)
    print(f"{len(tiny)} images under {TINY} samples: {inside} of {total} samples inside the band, {100 * inside / total:.2f} %")
    assert len(tiny) >= 8 and inside <= 0.02 * total, (inside, total)


def test_a_padded_frame_stride_and_dirty_scratch():
    files = list(_own_files("48x64_x3", 90))
    T, H, W = 3, 48, 64
    frame, stride, g = H * W * 3, H * W * 3 + 80, 128
    buf = torch.full((2 * g + T * stride,), 0xA5, dtype=torch.uint8, device=DEV)
    view = buf[g:g + T * stride].view(T, stride)[:, :frame].view(T, H, W, 3)
    coef_bytes, scratch_bytes = ops.jpeg_decode_sizes(T, H, W, 3, 2, 2)
    scratch = (torch.full((T, 3, 4, 6, 64), GUARD, dtype=torch.int16, device=DEV),
               torch.full((scratch_bytes,), 0xFF, dtype=torch.uint8, device=DEV))      # fp32 NaN planes
    assert coef_bytes == scratch[0].numel() * 2
    out = ops.jpeg_decode(files, out=view, scratch=scratch)
    assert out.data_ptr() == view.data_ptr()
    want = ops.jpeg_decode(files)
    assert torch.equal(view, want)
    host = buf.cpu().view(-1)
    assert bool((host[:g] == 0xA5).all()) and bool((host[g + T * stride:] == 0xA5).all())
    for t in range(T):
        assert bool((host[g + t * stride + frame:g + (t + 1) * stride] == 0xA5).all())
    again = ops.jpeg_decode(files, out=view, scratch=scratch)       # the scratch now holds the first call's planes
    assert torch.equal(again, want)


# ---- resize ---------------------------------------------------------------------------------------------------------------------------------
RESIZES = [((1, 1), (8, 8)), ((9, 7), (24, 40)), ((37, 53), (48, 80)), ((100, 60), (33, 47)), ((17, 400), (16, 16)),
           ((270, 480), (120, 208))]


@pytest.mark.parametrize("src,dst", RESIZES)
def test_resize_stretch(src, dst):
    x = J.noise(*src, seed=src[0] + dst[1])
    got = ops.resize_u8(_dev(x[None]), dst, fit="stretch")
    assert got.shape == (1, *dst, 3) and got.dtype == torch.uint8
    _pixel_rule(got[0].cpu().numpy(), D.resize_unrounded(x, *dst), f"{src} -> {dst}", cap=0.03)


@pytest.mark.parametrize("src", [(64, 64), (48, 200)])
def test_resize_cover_with_a_padded_stride(src):
    T, dst = 3, (48, 80)
    x = np.stack([J.noise(*src, seed=s) for s in range(T)])
    frame, stride = src[0] * src[1] * 3, src[0] * src[1] * 3 + 48
    sbuf = torch.full((T, stride), 0x5A, dtype=torch.uint8, device=DEV)
    sview = sbuf[:, :frame].view(T, *src, 3)
    sview.copy_(_dev(x))
    oframe, ostride, g = dst[0] * dst[1] * 3, dst[0] * dst[1] * 3 + 32, 64
    obuf = torch.full((2 * g + T * ostride,), 0xA5, dtype=torch.uint8, device=DEV)
    oview = obuf[g:g + T * ostride].view(T, ostride)[:, :oframe].view(T, *dst, 3)
    ops.resize_u8(sview, dst, fit="cover", out=oview)
    y0, x0, Hc, Wc = D.cover_window(*src, *dst)
    want = D.resize_unrounded(x[:, y0:y0 + Hc, x0:x0 + Wc], *dst)
    _pixel_rule(oview.cpu().numpy(), want, f"cover {src} -> {dst}", cap=0.03)
    host = obuf.cpu()
    assert bool((host[:g] == 0xA5).all()) and bool((host[g + T * ostride:] == 0xA5).all())
    for t in range(T):
        assert bool((host[g + t * ostride + oframe:g + (t + 1) * ostride] == 0xA5).all())


def test_resize_to_the_same_size_is_the_input():
    x = _dev(np.stack([J.noise(37, 53, 1), J.pixel_checkerboard(37, 53)]))
    assert torch.equal(ops.resize_u8(x, (37, 53), fit="stretch"), x)
    assert torch.equal(ops.resize_u8(x, (37, 53), fit="cover"), x)


# ---- end to end, small ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vae():
    from longlive_amd import synth
    from longlive_amd.vae import WanVAEWrapper
    cfg = synth.VaeConfig()
    sd = dict(synth.synth_vae_state_dict(cfg, seed=5))
    sd.update(synth.synth_vae_encoder_state_dict(cfg, seed=6))
    m = WanVAEWrapper(device=DEV)
    m.load_state_dict(sd)
    return m


def test_a_clip_decoded_on_the_gpu_gives_the_decoders_latent(tmp_path, vae):
    """11 frames of 48 x 80 written as MJPEG: `input_decode: gpu` decodes the last 9 chunks only, on the device, and their latent is
    the latent of ops.jpeg_decode's frames."""
    frames = np.stack([J.smooth_noise(48, 80, s) for s in range(11)])
    files = ops.jpeg_bytes(*ops.jpeg_encode(_dev(frames), 90))
    cli.write_avi_mjpeg(str(tmp_path / "clip.avi"), files, 80, 48)
    cfg = cli.Config(input_video=str(tmp_path / "clip.avi"), input_decode="gpu")
    clip, size = cli.load_clip_device(cfg, 6, 10, torch.device(DEV))
    assert size is None and clip.is_cuda and clip.shape == (9, 48, 80, 3)
    want = ops.jpeg_decode(files[2:])                            # the last 1 + 4k of 11
    assert torch.equal(clip, want)
    latent = vae.encode_frames_to_latent(clip.unsqueeze(0))
    assert latent.shape == (1, 3, 16, 6, 10) and torch.equal(latent, vae.encode_frames_to_latent(want.unsqueeze(0)))
    cfg.input_frames = 7
    assert torch.equal(cli.load_clip_device(cfg, 6, 10, torch.device(DEV))[0], ops.jpeg_decode(files[6:]))


def test_a_clip_decoded_on_the_host_differs_through_the_decoder_alone(tmp_path, vae):
    """The same 48 x 80 file with `input_decode: host` (PIL): refused at another size without `input_fit`, uploaded as it is at its
    own; its latent against the GPU-decoded clip's is reported and gates nothing."""
    pytest.importorskip("PIL.Image")
    frames = np.stack([J.smooth_noise(48, 80, s) for s in range(11)])
    files = ops.jpeg_bytes(*ops.jpeg_encode(_dev(frames), 90))
    cli.write_avi_mjpeg(str(tmp_path / "clip.avi"), files, 80, 48)
    cfg = cli.Config(input_video=str(tmp_path / "clip.avi"), input_decode="host")
    with pytest.raises(ValueError, match="80x48.*96x64.*input_fit"):
        cli.load_clip_device(cfg, 8, 12, torch.device(DEV))
    cfg.input_fit = "stretch"
    host_clip, size = cli.load_clip_device(cfg, 6, 10, torch.device(DEV))      # the size fits: nothing is resized
    assert size is None and torch.equal(host_clip.cpu(), cli.read_avi_mjpeg(str(tmp_path / "clip.avi"))[2:])
    host = vae.encode_frames_to_latent(host_clip.unsqueeze(0))
    latent = vae.encode_frames_to_latent(ops.jpeg_decode(files[2:]).unsqueeze(0))
    rel = float((latent.double() - host.double()).norm() / host.double().norm())
    print(f"latent of the GPU-decoded clip against the PIL-decoded one: rel-L2 {rel:.3e}")      # reported, gates nothing


def _config(tmp_path, **kw):
    base = dict(profile=False, denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3), output_folder=str(tmp_path / "out"),
                inference_iter=-1, num_output_frames=3, use_ema=False, seed=0, num_samples=1, save_with_index=True,
                global_sink=True, context_noise=0, synthetic=True,
                synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12))
    base.update(kw)
    return cli.Config(**base)


def test_cli_resizes_footage_of_another_size(tmp_path, monkeypatch):
    """A 96 x 160 Pillow-made 4:2:2 clip through cli.run in synthetic mode at 64 x 96: decoded and resized on the device."""
    Image = pytest.importorskip("PIL.Image")
    from longlive_amd.vae import WanVAEWrapper
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    files = [D.pil_file(Image, J.smooth_noise(96, 160, s), 1, quality=90) for s in range(5)]
    cli.write_avi_mjpeg(str(tmp_path / "footage.avi"), files, 160, 96)
    seen, real = {}, WanVAEWrapper.encode_frames_to_latent

    def spy(self, frames, keep_cache=False):
        seen["frames"] = frames.clone()
        return real(self, frames, keep_cache=keep_cache)

    monkeypatch.setattr(WanVAEWrapper, "encode_frames_to_latent", spy)
    cfg = _config(tmp_path, data_path=str(p), input_video=str(tmp_path / "footage.avi"), input_decode="gpu", input_fit="cover")
    recs = cli.run("inference", cfg, device=torch.device("cuda", 0))
    assert len(recs) == 1 and recs[0]["input_frames"] == 5 and recs[0]["input_size"] == [160, 96]
    assert recs[0]["frames"] == 1 + 4 * (2 + 3 - 1)
    want = ops.resize_u8(ops.jpeg_decode(files), (64, 96), fit="cover")
    assert seen["frames"].is_cuda and seen["frames"].shape == (1, 5, 64, 96, 3) and torch.equal(seen["frames"][0], want)
    y0, x0, Hc, Wc = D.cover_window(96, 160, 64, 96)
    ref = D.resize_unrounded(np.stack([D.decode(f) for f in files])[:, y0:y0 + Hc, x0:x0 + Wc], 64, 96)
    assert float(np.abs(want.cpu().numpy().astype(np.float64) - ref).max()) <= 2.0      # two roundings of one level: decoder, resize
    # host decode with the same key: uploaded, then resized on the device
    cfg.input_decode = "host"
    clip, size = cli.load_clip_device(cfg, 8, 12, torch.device(DEV))
    assert size == [160, 96] and torch.equal(clip, ops.resize_u8(cli.read_avi_mjpeg(str(tmp_path / "footage.avi")).to(DEV), (64, 96)))
    cfg.input_decode, cfg.input_fit = "gpu", None
    with pytest.raises(ValueError, match="160x96.*96x64.*input_fit"):
        cli.run("inference", cfg, device=torch.device("cuda", 0))
