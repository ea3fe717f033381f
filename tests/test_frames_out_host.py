"""Frames out, host side (no GPU): the restatement of the JPEG encoder (tests/jpeg_ref.py) against PIL's decoder and encoder and at
the coder's edges, the MJPEG AVI writer / reader, the new entry points at the C-ABI boundary, and the CLI's `video_codec` /
`jpeg_quality` keys."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import jpeg_ref as J
from longlive_amd import _lib, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ll_cl_to_frames_u8": 8, "ll_jpeg_sizes": 5, "ll_jpeg_encode_u8": 12, "ll_jpeg_coefficients_u8": 8}


# ---- the restatement against PIL -----------------------------------------------------------------------------------------------------
def _pil_encode(Image, frame, quality):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", quality=quality, subsampling=2)
    return b.getvalue()


def _pil_decode(Image, data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


PIL_SHAPES = [(48, 64, "smooth"), (150, 40, "smooth"), (23, 37, "smooth"), (1, 1, "smooth"), (32, 48, "noise"), (16, 16, "flat"),
              (160, 16, "smooth")]


@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("H,W,kind", PIL_SHAPES)
def test_restatement_decodes_in_pil_as_well_as_pils_own_files(H, W, kind, quality):
    """PSNR(ours) >= PSNR(PIL, same quality, 4:2:0) - 0.1 dB: three times the 0.03 dB measured when this was written; the two
    encoders differ only in DCT arithmetic and chroma rounding."""
    Image = pytest.importorskip("PIL.Image")
    frame = {"smooth": J.smooth_noise, "noise": J.noise, "flat": J.flat}[kind](H, W)
    data = J.encode(frame, quality)
    im = _pil_decode(Image, data)
    assert im.size == (W, H) and im.mode == "RGB"
    ours = J.psnr(np.asarray(im), frame)
    pil = J.psnr(np.asarray(_pil_decode(Image, _pil_encode(Image, frame, quality)).convert("RGB")), frame)
    assert ours >= pil - 0.1, (ours, pil)
    if H == 160:                                                # ten intervals: RST0 .. RST7, RST0
        assert [data.count(bytes([0xFF, 0xD0 + m])) for m in range(8)] == [2] + [1] * 7


def test_tables_are_the_ones_pil_writes():
    """Annex K as libjpeg carries it: the four Huffman tables of a non-optimised PIL file and its quantisation tables at several
    qualities equal the ones typed into tests/jpeg_ref.py."""
    Image = pytest.importorskip("PIL.Image")
    data = _pil_encode(Image, J.smooth_noise(16, 16), 75)
    tables, p = {}, 2
    while data[p + 1] != 0xDA:
        n = int.from_bytes(data[p + 2:p + 4], "big")
        if data[p + 1] == 0xC4:
            q = p + 4
            while q < p + 2 + n:
                bits = list(data[q + 1:q + 17])
                tables[data[q]] = (bits, list(data[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        p += 2 + n
    assert tables == {0x00: (J.DC_LUM_BITS, J.DC_VALS), 0x10: (J.AC_LUM_BITS, J.AC_LUM_VALS), 0x01: (J.DC_CHR_BITS, J.DC_VALS),
                      0x11: (J.AC_CHR_BITS, J.AC_CHR_VALS)}
    for quality in (1, 10, 49, 50, 90, 100):
        want = sorted(sorted(int(v) for v in t) for t in J.quant_tables(quality))
        got = _pil_decode(Image, _pil_encode(Image, J.smooth_noise(16, 16), quality)).quantization
        assert sorted(sorted(got[k]) for k in (0, 1)) == want, quality        # (PIL's order of the 64 entries varies with its version)
    assert J.header(37, 23, 90)[20:25] == b"\xff\xdb\x00\x84\x00" and len(J.header(37, 23, 90)) == J.HEADER_BYTES


# ---- edge inputs, proved from the histogram ---------------------------------------------------------------------------------------------
def _histogram(frame, quality):
    h = {}
    data = J.encode(frame, quality, h)
    return h, data


def test_noise_at_quality_100_is_stuffed():
    h, data = _histogram(J.noise(32, 48), 100)
    assert h["ff00"] > 0 and data.count(b"\xff\x00") >= h["ff00"]


def test_a_pixel_checkerboard_emits_zrl():
    h, _ = _histogram(J.pixel_checkerboard(32, 32), 10)          # what survives quality 10 sits at the end of the zigzag
    assert h[("ac", 0xF0)] > 0


def test_alternating_blocks_reach_dc_category_11():
    h, _ = _histogram(J.block_checkerboard(32, 32), 100)         # -1024 next to +1016
    assert h[("dc", 11)] > 0


def test_flat_frames_emit_eob_only():
    for quality in (10, 90, 100):
        h, _ = _histogram(J.flat(16, 16), quality)
        assert [k for k in h if isinstance(k, tuple) and k[0] == "ac"] == [("ac", 0x00)] and h[("ac", 0x00)] == 6


def test_the_block_bound_holds_for_the_widest_codes():
    """208 bytes per block: no (run, size) code of Annex K is longer than 16 bits and no amplitude longer than 10 (DC: 9 + 11)."""
    for bits, vals in ((J.AC_LUM_BITS, J.AC_LUM_VALS), (J.AC_CHR_BITS, J.AC_CHR_VALS)):
        codes = J.huffman_codes(bits, vals)
        assert len(codes) == 162 and max(len(c) + (s & 15) for s, c in codes.items()) <= 26
    for bits in (J.DC_LUM_BITS, J.DC_CHR_BITS):
        assert max(len(c) + s for s, c in J.huffman_codes(bits, J.DC_VALS).items()) <= 26


# ---- AVI -------------------------------------------------------------------------------------------------------------------------------------
def test_mjpeg_avi_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    frames = [J.smooth_noise(23, 37, s) for s in range(4)]
    files = [J.encode(f, 90) for f in frames]
    files[1] += b"\x00" * (1 - len(files[1]) % 2)                # one odd, one even length at least
    files[2] += b"\x00" * (len(files[2]) % 2)
    assert {len(f) % 2 for f in files} == {0, 1}
    path = str(tmp_path / "clip.avi")
    size = cli.write_avi_mjpeg(path, files, 37, 23, fps=16)
    raw = open(path, "rb").read()
    assert size == len(raw) == 8 + int.from_bytes(raw[4:8], "little")
    assert raw.count(b"MJPG") == 2 and cli.avi_compression(path) == b"MJPG"
    got = cli.read_avi_mjpeg(path)
    want = torch.stack([torch.from_numpy(np.asarray(_pil_decode(Image, f).convert("RGB")).copy()) for f in files])
    assert got.dtype == torch.uint8 and got.shape == (4, 23, 37, 3) and torch.equal(got, want)
    assert torch.equal(cli.read_input_video(path), want)
    # chunks start on even offsets; idx1 carries the true sizes and the chunks' offsets from 'movi'
    movi = raw.index(b"movi")
    idx = raw.index(b"idx1", movi + sum(len(f) for f in files))
    assert int.from_bytes(raw[idx + 4:idx + 8], "little") == 16 * 4
    for t, f in enumerate(files):
        tag, flags, off, n = raw[idx + 8 + 16 * t:idx + 12 + 16 * t], *np.frombuffer(raw, "<u4", 3, idx + 12 + 16 * t)
        assert tag == b"00dc" and n == len(f) and off % 2 == 0
        assert raw[movi + off:movi + off + 4] == b"00dc" and raw[movi + off + 8:movi + off + 8 + n] == f


class _Sized:
    """Stands for a frame of n bytes where only its length is asked for."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_mjpeg_avi_refuses_what_passes_4_gib_before_writing(tmp_path):
    path = tmp_path / "big.avi"
    frames = [_Sized(1_000_001)] * 5000                          # 5 GB
    with pytest.raises(ValueError, match=r"4 GiB.*first (\d+) frames fit") as exc:
        cli.write_avi_mjpeg(str(path), frames, 832, 480)
    assert not path.exists()
    fit = int(re.search(r"first (\d+) frames fit", str(exc.value)).group(1))
    per = 8 + 1_000_002 + 16                                     # chunk header + padded data + index entry
    assert fit == (2 ** 32 - 8 - (4 + 200 + 8 + 4 + 8)) // per and fit * per < 2 ** 32 < (fit + 1) * per + 232      # 200: the hdrl list
    with pytest.raises(ValueError, match="no frames"):
        cli.write_avi_mjpeg(str(path), [], 832, 480)


def test_read_input_video_still_reads_rgb24(tmp_path):
    frames = torch.randint(0, 256, (3, 6, 10, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    cli.write_avi_rgb24(str(tmp_path / "raw.avi"), frames)
    assert cli.avi_compression(str(tmp_path / "raw.avi")) == b"\x00\x00\x00\x00"
    assert torch.equal(cli.read_input_video(str(tmp_path / "raw.avi")), frames)


def test_reading_mjpeg_names_pil_when_it_is_absent(tmp_path, monkeypatch):
    import sys
    cli.write_avi_mjpeg(str(tmp_path / "c.avi"), [J.encode(J.flat(16, 16), 90)], 16, 16)
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(RuntimeError, match="PIL"):
        cli.read_input_video(str(tmp_path / "c.avi"))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "longlive_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    version_comment = header[header.index("ABI version of this header"):header.index("#define LL_ABI_VERSION")]
    for name, n in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", body, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n, name
        assert len(_lib.SIGNATURES[name]) == n and hasattr(lib, name) and name in version_comment, name
    assert _lib.ABI_VERSION == 111 == lib.ll_version()


def _sizes(T, H, W):
    a, b = C.c_longlong(-1), C.c_longlong(-1)
    rc = _lib.load().ll_jpeg_sizes(T, H, W, C.byref(a), C.byref(b))
    return rc, a.value, b.value


@pytest.mark.parametrize("T,H,W", [(1, 1, 1), (1, 16, 16), (2, 17, 33), (3, 480, 832), (1, 65535, 16), (1, 16, 65535)])
def test_jpeg_sizes_is_the_bounds_formula(T, H, W):
    rc, stride, scratch = _sizes(T, H, W)
    rows, cols = J.mcu_grid(H, W)
    assert rc == 0 and stride == J.worst_case_bytes(H, W) and stride % 16 == 0
    blocks = T * rows * cols * 6
    # coefficients + a 208-byte slot + two ints per block, a stuffed interval per MCU row, its length
    assert scratch >= blocks * (128 + 208 + 8) + T * rows * (cols * 6 * 416 + 2 + 4)


S1, SCR = J.worst_case_bytes(8, 8), 1 << 20


@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_cl_to_frames_u8(0, 16, 192, 1, 8, 8, 8, None), "ll_cl_to_frames_u8: null operand"),
    (lambda L: L.ll_cl_to_frames_u8(16, 0, 192, 1, 8, 8, 8, None), "ll_cl_to_frames_u8: null operand"),
    (lambda L: L.ll_cl_to_frames_u8(16, 16, 192, 1, 8, 8, 2, None), "ldc=2"),
    (lambda L: L.ll_cl_to_frames_u8(16, 16, 192, 1, 0, 8, 8, None), "empty input"),
    (lambda L: L.ll_cl_to_frames_u8(16, 16, 191, 2, 8, 8, 8, None), "stride_t=191"),
    (lambda L: L.ll_jpeg_encode_u8(0, 192, 1, 8, 8, 90, 16, S1, 16, 16, SCR, None), "ll_jpeg_encode_u8: null operand"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 8, 8, 90, 0, S1, 16, 16, SCR, None), "ll_jpeg_encode_u8: null operand"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 8, 8, 90, 16, S1, 0, 16, SCR, None), "ll_jpeg_encode_u8: null operand"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 8, 8, 90, 16, S1, 16, 0, SCR, None), "ll_jpeg_encode_u8: null operand"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 8, 8, 0, 16, S1, 16, 16, SCR, None), "quality=0"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 8, 8, 101, 16, S1, 16, 16, SCR, None), "quality=101"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 0, 8, 8, 90, 16, S1, 16, 16, SCR, None), "empty input"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 0, 8, 90, 16, S1, 16, 16, SCR, None), "empty input"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 8, 0, 90, 16, S1, 16, 16, SCR, None), "empty input"),
    (lambda L: L.ll_jpeg_encode_u8(16, 3 * 65536 * 8, 1, 65536, 8, 90, 16, 1 << 40, 16, 16, 1 << 40, None), "at most 65535"),
    (lambda L: L.ll_jpeg_encode_u8(16, 3 * 65536 * 8, 1, 8, 65536, 90, 16, 1 << 40, 16, 16, 1 << 40, None), "at most 65535"),
    (lambda L: L.ll_jpeg_encode_u8(16, 191, 2, 8, 8, 90, 16, S1, 16, 16, SCR, None), "stride_t=191"),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 8, 8, 90, 16, S1 - 1, 16, 16, SCR, None), "out_stride="),
    (lambda L: L.ll_jpeg_encode_u8(16, 192, 1, 8, 8, 90, 16, S1, 16, 16, _sizes(1, 8, 8)[2] - 1, None), "scratch_bytes="),
    (lambda L: L.ll_jpeg_coefficients_u8(0, 192, 1, 8, 8, 90, 16, None), "ll_jpeg_coefficients_u8: null operand"),
    (lambda L: L.ll_jpeg_coefficients_u8(16, 192, 1, 8, 8, 90, 0, None), "ll_jpeg_coefficients_u8: null operand"),
    (lambda L: L.ll_jpeg_coefficients_u8(16, 192, 1, 8, 8, 0, 16, None), "quality=0"),
    (lambda L: L.ll_jpeg_coefficients_u8(16, 191, 1, 8, 8, 90, 16, None), "stride_t=191"),
    (lambda L: L.ll_jpeg_sizes(1, 8, 8, None, None), "ll_jpeg_sizes: null operand"),
    (lambda L: _sizes(0, 8, 8)[0], "empty input"),
    (lambda L: _sizes(1, 65536, 8)[0], "at most 65535"),
    (lambda L: _sizes(1, 65535, 65535)[0], "more than one call covers"),
])
def test_entry_points_reject_bad_arguments_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


def test_wrappers_refuse_host_tensors():
    from longlive_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cl_to_frames_u8(torch.zeros(1, 8, 8, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.jpeg_encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.jpeg_coefficients(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    assert ops.jpeg_sizes(1, 8, 8)[0] == S1


# ---- yaml ----------------------------------------------------------------------------------------------------------------------------------
def test_codec_names_and_quality_range():
    assert cli.video_codec(None) is None and cli.video_codec("none") is None
    assert cli.video_codec("mjpeg") == "mjpeg" == cli.video_codec(" MJPEG ")
    for bad in ("h264", "mp4", "", True):
        with pytest.raises(ValueError, match="video_codec"):
            cli.video_codec(bad)
    assert cli.jpeg_quality(None) == 90 and cli.jpeg_quality(1) == 1 and cli.jpeg_quality(100) == 100
    for bad in (0, 101, -5, 90.0, "90", True):
        with pytest.raises(ValueError, match="jpeg_quality"):
            cli.jpeg_quality(bad)


def test_an_unknown_codec_is_refused_before_any_model_is_built(monkeypatch):
    def no_models(*a, **k):
        raise AssertionError("models were built")

    monkeypatch.setattr(cli, "build_models", no_models)
    cfg = cli.Config(seed=0, synthetic=True, model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3),
                     synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12), video_codec="h265")
    with pytest.raises(ValueError, match="video_codec.*h265"):
        cli.run("inference", cfg, device=torch.device("cpu"))
    cfg.video_codec, cfg.jpeg_quality = "mjpeg", 0
    with pytest.raises(ValueError, match="jpeg_quality"):
        cli.run("inference", cfg, device=torch.device("cpu"))


def test_pipeline_keyword_is_checked_before_anything_runs():
    from longlive_amd.pipeline.causal_inference import check_frames_mode
    for ok in ("float", "uint8", "jpeg"):
        check_frames_mode(ok, 90)
    with pytest.raises(ValueError, match="frames"):
        check_frames_mode("rgb", 90)
    with pytest.raises(ValueError, match="jpeg_quality"):
        check_frames_mode("jpeg", 101)
    check_frames_mode("uint8", 101)                             # the quality is read by "jpeg" alone


def test_the_continue_config_names_the_codec():
    text = open(os.path.join(ROOT, "configs", "continue_clip.yaml")).read()
    assert re.search(r"^#\s*video_codec:\s*mjpeg", text, flags=re.M) and "jpeg_quality" in text
    assert "video_codec" not in cli.load_config(os.path.join(ROOT, "configs", "continue_clip.yaml"))
