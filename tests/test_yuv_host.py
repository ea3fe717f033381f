"""Planar YUV and Y4M, host side (no GPU): the numpy restatement (tests/yuv_ref.py) against its check values, the real-valued BT.601
transform and Pillow; csrc/yuv.h as a stand-alone program under the host sanitizers; the Y4M writer and reader; frame selection by
rate; the new entry points at the C-ABI boundary; the CLI's and the pipelines' new keys."""
import io
import os
import re
import shutil
import subprocess
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import yuv_ref as R
from longlive_amd import _lib, cli, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ll_frames_u8_to_yuv420": 9, "ll_cl_to_yuv420": 9, "ll_yuv_to_frames_u8": 13}


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_coefficients_equal_the_check_values():
    assert R.forward_coefficients("full") == ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329))
    assert R.forward_coefficients("limited") == ((16829, 33039, 6416), (-9714, -19071, 28785), (28784, -24103, -4681))
    assert R.inverse_coefficients("full") == (65536, 91881, 116130, 22553, 46802)
    assert R.inverse_coefficients("limited") == (76309, 104597, 132201, 25675, 53279)
    for rng in ("full", "limited"):
        a, b, c = R.forward_coefficients(rng)
        assert sum(b) == 0 == sum(c) and sum(a) == R.rnd(R.scales(rng)[0] * 65536)


@pytest.mark.parametrize("rng", ["full", "limited"])
def test_restatement_stays_within_half_a_step_of_real_bt601(rng):
    """|integer - exact| <= 0.51 on random RGB (0.502 was measured): rounding to an integer costs 0.5, the 2^16 coefficients the rest."""
    g = np.random.default_rng(1)
    rgb = g.integers(0, 256, (1, 64, 96, 3), dtype=np.uint8)
    y, cb, cr = R.rgb_to_planes(rgb, rng)
    sy, sc, yoff = (float(v) for v in R.scales(rng)[:3])
    f = rgb.astype(np.float64)
    yl = 0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]
    assert np.abs(y - (yoff + sy * yl)).max() <= 0.51
    mean = lambda p: (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) / 4.0       # noqa: E731
    ecb = 128 + sc * (mean(f[..., 2]) - mean(yl)) / (2 * (1 - 0.114))
    ecr = 128 + sc * (mean(f[..., 0]) - mean(yl)) / (2 * (1 - 0.299))
    worst = max(np.abs(cb - ecb).max(), np.abs(cr - ecr).max())
    print(f"{rng}: worst chroma error {worst:.4f}")
    assert worst <= 0.51


def test_full_range_against_pillow_in_both_directions():
    """Pillow's convert("YCbCr") is full-range BT.601 in its own fixed point: every sample within 1 (a condition, not a measurement)."""
    Image = pytest.importorskip("PIL.Image")
    g = np.random.default_rng(2)
    quads = g.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    rgb = quads.repeat(2, 0).repeat(2, 1)                           # constant over 2 x 2 quads: the quad's mean is its pixel
    y, cb, cr = R.rgb_to_planes(rgb[None], "full")
    pil = np.asarray(Image.fromarray(rgb).convert("YCbCr")).astype(np.int64)
    dy = np.abs(y[0].astype(np.int64) - pil[..., 0]).max()
    dc = max(np.abs(cb[0].astype(np.int64) - pil[0::2, 0::2, 1]).max(), np.abs(cr[0].astype(np.int64) - pil[0::2, 0::2, 2]).max())
    planes = g.integers(0, 256, (3, 1, 40, 56), dtype=np.uint8)
    back = R.planes_to_rgb(planes[0], planes[1], planes[2], "444", "full")[0]
    pil_back = np.asarray(Image.fromarray(np.stack([p[0] for p in planes], -1), "YCbCr").convert("RGB")).astype(np.int64)
    di = np.abs(back.astype(np.int64) - pil_back).max()
    print(f"against Pillow: luma {dy}, chroma {dc}, inverse {di}")
    assert dy <= 1 and dc <= 1 and di <= 1


def test_grey_is_colourless_and_a_ramp_round_trips():
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, 3)
    for rng, slack in (("full", 0), ("limited", 1)):
        y, cb, cr = R.rgb_to_planes(ramp, rng)
        assert (cb == 128).all() and (cr == 128).all()
        for layout in ("420jpeg", "420mpeg2", "420paldv"):
            back = R.planes_to_rgb(y, cb, cr, layout, rng)
            assert np.abs(back.astype(np.int64) - ramp).max() <= slack
        assert np.array_equal(R.planes_to_rgb(y, None, None, "mono", rng), R.planes_to_rgb(y, cb, cr, "420jpeg", rng))
    assert np.array_equal(R.rgb_to_planes(ramp, "full")[0][..., None].repeat(3, 3), ramp)


# ---- csrc/yuv.h under the host sanitizers ------------------------------------------------------------------------------------------
def _sanitizer_flags(cxx, tmp_path):
    """-fsanitize flags this compiler can link, the runtimes linked statically so that the program carries its own; None when a program
    of an empty main does not build with them (asked BEFORE the program under test is built)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + extra
        r = subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            return flags
    return None


def _lcg_bytes(seed, n):
    out, x = np.empty(n, np.uint8), seed
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = x >> 24
    return out, x


def test_yuv_h_equals_the_restatement_under_host_sanitizers(tmp_path):
    """tests/yuv_host_main.cpp (its own main) built from csrc/yuv.h with the host compiler and -fsanitize=address,undefined: all 2^24
    RGB values through the luma routine, 2 x 2 quads including the all-equal and extreme ones, and the six layouts over exactly-sized
    heap planes of 1x1, 1x2, 2x1, 3x5 and 8x9, both ranges; every printed line equals the restatement's."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = _sanitizer_flags(cxx, tmp_path)
    if flags is None:
        pytest.skip("the host compiler cannot link a sanitized program of an empty main")
    exe = str(tmp_path / "yuv_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "longlive_amd", "csrc"),
                            os.path.join(ROOT, "tests", "yuv_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    want = []
    idx = np.arange(1 << 24, dtype=np.int64)
    rgb = np.stack([idx >> 16, (idx >> 8) & 255, idx & 255], -1)
    weight = (1 + idx % 65521).astype(np.uint64)
    for full, rng in enumerate(("limited", "full")):
        want.append(f"luma {full} {int((R.luma(rgb, rng).astype(np.uint64) * weight).sum(dtype=np.uint64))}")
    quads = [np.full(12, v, np.int64) for v in (0, 1, 127, 128, 254, 255)]
    for c in range(3):
        for hi in range(2):
            quads.append(np.array([255 if (k == c) == (hi == 1) else 0 for _ in range(4) for k in range(3)], np.int64))
    state = 12345
    for _ in range(64):
        q, state = _lcg_bytes(state, 12)
        quads.append(q.astype(np.int64))
    for full, rng in enumerate(("limited", "full")):
        for k, q in enumerate(quads):
            cb, cr = R.chroma_of_sums(q.reshape(4, 3).sum(0), rng)
            want.append(f"quad {full} {k} {int(cb)} {int(cr)}")
    grey = [k for k in range(6)]
    assert all(w.endswith(" 128 128") for w in want if w.startswith("quad") and int(w.split()[2]) in grey)
    state = 777
    for li, layout in enumerate(R.LAYOUTS):
        for full, rng in enumerate(("limited", "full")):
            for H, W in ((1, 1), (1, 2), (2, 1), (3, 5), (8, 9)):
                hc, wc = R.chroma_shape(layout, H, W)
                y, state = _lcg_bytes(state, H * W)
                cb, state = _lcg_bytes(state, hc * wc)
                cr, state = _lcg_bytes(state, hc * wc)
                out = R.planes_to_rgb(y.reshape(1, H, W), cb.reshape(1, hc, wc) if hc else None, cr.reshape(1, hc, wc) if hc else None,
                                      layout, rng).reshape(-1).astype(np.int64)
                want.append(f"up {li} {full} {H} {W} {int((out * (1 + np.arange(out.size) % 251)).sum())}")
    got = run.stdout.split("\n")
    assert got[-1] == "" and got[:-1] == want


# ---- Y4M -----------------------------------------------------------------------------------------------------------------------------
def _payloads(n, H, W, layout="420jpeg", seed=0):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, y4m.frame_bytes(layout, H, W), dtype=np.uint8).tobytes() for _ in range(n)]


def test_writer_to_reader_identity_and_header_tag_order(tmp_path):
    frames = _payloads(5, 6, 10)
    path = str(tmp_path / "a.y4m")
    size = y4m.write_y4m(path, iter(np.frombuffer(f, np.uint8) for f in frames), 10, 6, fps=Fraction(30000, 1001), range="full")
    raw = open(path, "rb").read()
    assert size == len(raw) == os.path.getsize(path)
    assert raw.startswith(b"YUV4MPEG2 W10 H6 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\nFRAME\n")
    with y4m.Y4MReader(path) as r:
        assert (r.width, r.height, r.fps, r.layout, r.range, r.interlace, r.aspect) == (10, 6, Fraction(30000, 1001), "420jpeg", "full", "p", "1:1")
        assert r.frame_bytes == 6 * 10 + 2 * 3 * 5 == len(frames[0])
        assert list(r) == frames and r.frames_read == 5
    y4m.write_y4m(path, frames[:1], 10, 6)
    assert open(path, "rb").read().startswith(b"YUV4MPEG2 W10 H6 F16:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n")
    for bad, needle in ((dict(range="video"), "range"), (dict(fps=0), "fps"), (dict(W=0), "W, H")):
        with pytest.raises(ValueError, match=needle):
            y4m.write_y4m(str(tmp_path / "b.y4m"), frames, **{"W": 10, "H": 6, **bad})
    with pytest.raises(ValueError, match="frame 0: 3 bytes"):
        y4m.write_y4m(str(tmp_path / "b.y4m"), [b"abc"], 10, 6)


def test_reader_takes_tags_in_any_order_frame_parameters_and_every_layout():
    for tag, layout in (("C420jpeg", "420jpeg"), ("C420", "420jpeg"), (None, "420jpeg"), ("C420mpeg2", "420mpeg2"), ("C420paldv", "420paldv"),
                        ("C422", "422"), ("C444", "444"), ("Cmono", "mono")):
        frames = _payloads(3, 5, 7, layout)
        head = " ".join(t for t in ("YUV4MPEG2", tag, "XYSCSS=whatever", "A128:117", "H5", "I?", "F25:1", "W7") if t)
        raw = head.encode() + b"\n" + b"".join(b"FRAME Ip Xsomething=1\n" + f for f in frames)
        r = y4m.Y4MReader(io.BytesIO(raw))
        assert (r.width, r.height, r.fps, r.layout, r.range, r.aspect) == (7, 5, 25, layout, "limited", "128:117")
        assert list(r) == frames
    raw = b"YUV4MPEG2 W2 H2\nFRAME\n" + bytes(6)
    assert y4m.Y4MReader(io.BytesIO(raw), input_range="full").range == "full"
    assert y4m.Y4MReader(io.BytesIO(raw.replace(b"H2", b"H2 XCOLORRANGE=LIMITED")), input_range="full").range == "limited"
    assert y4m.Y4MReader(io.BytesIO(raw)).fps is None


def test_reader_reads_a_fifo(tmp_path):
    frames = _payloads(7, 16, 24, seed=3)
    fifo = str(tmp_path / "pipe")
    os.mkfifo(fifo)

    def feed():
        with open(fifo, "wb") as f:
            y4m.write_y4m(f, frames, 24, 16, fps=24)

    t = threading.Thread(target=feed)
    t.start()
    try:
        with y4m.Y4MReader(fifo) as r:
            got = r.read_last(3)
            assert r.fps == 24 and r.frames_read == 7
    finally:
        t.join()
    assert got == frames[-3:]
    assert cli.is_y4m_input(fifo) and cli.is_y4m_input("x.Y4M") and not cli.is_y4m_input(str(tmp_path / "clip.avi"))


def test_read_last_keeps_a_ring_of_a_longer_stream():
    frames = _payloads(11, 2, 2)
    raw = io.BytesIO()
    y4m.write_y4m(raw, frames, 2, 2)
    for n, want in ((1, frames[-1:]), (4, frames[-4:]), (11, frames), (20, frames), (None, frames)):
        r = y4m.Y4MReader(io.BytesIO(raw.getvalue()))
        assert r.read_last(n) == want and r.frames_read == 11
    with pytest.raises(ValueError, match="read_last"):
        y4m.Y4MReader(io.BytesIO(raw.getvalue())).read_last(0)


@pytest.mark.parametrize("raw,needle", [
    (b"", "YUV4MPEG2"),
    (b"YUV4MPEG W4 H4\n", "YUV4MPEG2"),
    (b"RIFF" + bytes(5000), "YUV4MPEG2"),
    (b"YUV4MPEG2 H4 F16:1\n", "no W tag"),
    (b"YUV4MPEG2 W4 F16:1\n", "no H tag"),
    (b"YUV4MPEG2 W0 H4\n", "W tag"),
    (b"YUV4MPEG2 W4 H4 It\n", "I tag 'It'"),
    (b"YUV4MPEG2 W4 H4 Ib\n", "I tag 'Ib'"),
    (b"YUV4MPEG2 W4 H4 Im\n", "I tag 'Im'"),
    (b"YUV4MPEG2 W4 H4 C420p10\n", "C tag 'C420p10'"),
    (b"YUV4MPEG2 W4 H4 C444alpha\n", "C tag 'C444alpha'"),
    (b"YUV4MPEG2 W4 H4 C411\n", "C tag 'C411'"),
    (b"YUV4MPEG2 W4 H4 F16\n", "F tag"),
    (b"YUV4MPEG2 W4 H4 XCOLORRANGE=PC\n", "XCOLORRANGE"),
])
def test_reader_refuses_by_tag(raw, needle):
    with pytest.raises(ValueError, match=re.escape(needle)):
        y4m.Y4MReader(io.BytesIO(raw))


def test_reader_refuses_short_payloads_unknown_rates_and_bad_ranges():
    frames = _payloads(3, 4, 4)
    raw = b"YUV4MPEG2 W4 H4 F0:0\n" + b"".join(b"FRAME\n" + f for f in frames)
    r = y4m.Y4MReader(io.BytesIO(raw[:-5]))
    with pytest.raises(ValueError, match="frame 2: the payload holds 19 bytes, the header promises 24"):
        list(r)
    assert r.frames_read == 2
    with pytest.raises(ValueError, match="frame 1: expected a FRAME line"):
        list(y4m.Y4MReader(io.BytesIO(raw.replace(b"FRAME\n" + frames[1], b"FRAMF\n" + frames[1]))))
    with pytest.raises(ValueError, match="F0:0"):
        y4m.Y4MReader(io.BytesIO(raw)).rate()
    with pytest.raises(ValueError, match="input_range"):
        y4m.Y4MReader(io.BytesIO(raw), input_range="pc")


# ---- frame selection by rate -----------------------------------------------------------------------------------------------------------
def test_equal_rates_reproduce_select_clip_frames():
    for total in range(1, 41):
        for cap in (None, 1, 2, 4, 5, 8, 9, 13, 40, 100):
            want = list(range(total))[cli.select_clip_frames(total, cap)]
            assert y4m.select_frames_at_rate(total, 16, 16, cap) == want
            assert y4m.select_frames_at_rate(total, Fraction(24000, 1001), "24000:1001", cap) == want


@pytest.mark.parametrize("src", [Fraction(30000, 1001), 24, 25, 30, 60, 8])
def test_selection_by_rate_is_spaced_like_the_rates(src):
    step = Fraction(src) / 16
    for total in (1, 2, 5, 16, 33, 100, 257):
        for cap in (None, 1, 5, 12, 21):
            idx = y4m.select_frames_at_rate(total, src, 16, cap)
            n = len(idx)
            assert n % 4 == 1 and idx[-1] == total - 1 and idx[0] >= 0 and (cap is None or n <= cap)
            assert idx == [total - 1 - R.rnd(j * step) for j in range(n - 1, -1, -1)]
            gaps = [b - a for a, b in zip(idx, idx[1:])]
            lo, hi = step.numerator // step.denominator, -((-step.numerator) // step.denominator)
            assert all(lo <= g <= hi for g in gaps)                          # monotone; no repeat when src >= 16 (lo >= 1)
            if src == 8:
                assert 0 in gaps or n == 1                                   # a slower source is duplicated
            room = n + 4                                                     # the next length does not fit the clip or the cap
            assert (cap is not None and room > cap) or R.rnd((room - 1) * step) > total - 1
            assert y4m.frames_spanned(n, src, 16) == idx[-1] - idx[0] + 1


def test_selection_by_rate_refuses_bad_arguments():
    for args, needle in (((0, 30), "at least 1"), ((True, 30), "at least 1"), ((10, 0), "positive"), ((10, 30, 0), "positive"),
                         ((10, "fast"), "frame rate"), ((10, 30, 16, 0), "input_frames"), ((10, 30, 16, 2.5), "input_frames"),
                         ((10, -24), "positive"), ((10, (30, 0)), "frame rate")):
        with pytest.raises(ValueError, match=needle):
            y4m.select_frames_at_rate(*args)


# ---- C ABI and wrappers -----------------------------------------------------------------------------------------------------------------
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


B88 = R.yuv420_bytes(8, 8)      # 96


@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_frames_u8_to_yuv420(0, 192, 1, 8, 8, 0, 16, B88, None), "ll_frames_u8_to_yuv420: null operand"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 192, 1, 8, 8, 0, 0, B88, None), "ll_frames_u8_to_yuv420: null operand"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 192, 0, 8, 8, 0, 16, B88, None), "empty input"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 192, 1, 0, 8, 0, 16, B88, None), "empty input"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 192, 1, 8, 0, 0, 16, B88, None), "empty input"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 191, 2, 8, 8, 0, 16, B88, None), "stride_t=191"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 192, 2, 8, 8, 0, 16, B88 - 1, None), "out_stride=95"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 1 << 40, 1, 65536, 8, 0, 16, 1 << 40, None), "at most 65535"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 1 << 40, 1, 8, 65536, 0, 16, 1 << 40, None), "at most 65535"),
    (lambda L: L.ll_frames_u8_to_yuv420(16, 1 << 40, 1 << 30, 65535, 65535, 0, 16, 1 << 40, None), "more than one launch covers"),
    (lambda L: L.ll_cl_to_yuv420(0, 1, 8, 8, 8, 0, 16, B88, None), "ll_cl_to_yuv420: null operand"),
    (lambda L: L.ll_cl_to_yuv420(16, 1, 8, 8, 8, 0, 0, B88, None), "ll_cl_to_yuv420: null operand"),
    (lambda L: L.ll_cl_to_yuv420(16, 1, 8, 8, 2, 0, 16, B88, None), "ldc=2"),
    (lambda L: L.ll_cl_to_yuv420(16, 0, 8, 8, 8, 0, 16, B88, None), "empty input"),
    (lambda L: L.ll_cl_to_yuv420(16, 1, 8, 8, 8, 0, 16, B88 - 1, None), "out_stride=95"),
    (lambda L: L.ll_cl_to_yuv420(16, 1, 8, 65536, 8, 0, 16, 1 << 40, None), "at most 65535"),
    (lambda L: L.ll_yuv_to_frames_u8(0, 16, 16, 64, 16, 1, 8, 8, 0, 0, 16, 192, None), "ll_yuv_to_frames_u8: null operand"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 0, 16, 64, 16, 1, 8, 8, 0, 0, 16, 192, None), "ll_yuv_to_frames_u8: null operand"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 0, 64, 16, 1, 8, 8, 4, 0, 16, 192, None), "ll_yuv_to_frames_u8: null operand"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 64, 16, 1, 8, 8, 0, 0, 0, 192, None), "ll_yuv_to_frames_u8: null operand"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 64, 16, 1, 8, 8, 6, 0, 16, 192, None), "layout=6"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 64, 16, 1, 8, 8, -1, 0, 16, 192, None), "layout=-1"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 64, 16, 0, 8, 8, 0, 0, 16, 192, None), "empty input"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 63, 16, 2, 8, 8, 0, 0, 16, 192, None), "stride_y=63"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 64, 15, 2, 8, 8, 0, 0, 16, 192, None), "stride_c=15"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 64, 31, 2, 8, 8, 3, 0, 16, 192, None), "stride_c=31"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 64, 63, 2, 8, 8, 4, 0, 16, 192, None), "stride_c=63"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 64, 16, 2, 8, 8, 0, 0, 16, 191, None), "out_stride_t=191"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 1 << 40, 1 << 40, 1, 65536, 8, 0, 0, 16, 1 << 40, None), "at most 65535"),
    (lambda L: L.ll_yuv_to_frames_u8(16, 16, 16, 1 << 40, 1 << 40, 1 << 30, 65535, 65535, 0, 0, 16, 1 << 40, None), "more than one launch covers"),
])
def test_entry_points_reject_bad_arguments_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


def test_wrappers_refuse_host_tensors_and_unknown_names():
    from longlive_amd import ops
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.frames_u8_to_yuv420(u8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cl_to_yuv420(torch.zeros(1, 8, 8, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.yuv_to_frames_u8(u8[..., 0], u8[:, :4, :4, 0], u8[:, :4, :4, 0])
    with pytest.raises(ValueError, match="range"):
        ops.frames_u8_to_yuv420(u8, range="video")
    with pytest.raises(ValueError, match="layout"):
        ops.yuv_to_frames_u8(u8[..., 0], None, None, layout="411")
    assert ops.yuv420_bytes(8, 8) == 96 and ops.yuv420_bytes(3, 5) == 15 + 2 * 6 == R.yuv420_bytes(3, 5)
    assert [ops.yuv_chroma_shape(n, 5, 7) for n in ops.YUV_LAYOUTS] == [R.chroma_shape(n, 5, 7) for n in R.LAYOUTS]
    buf = torch.arange(2 * 27, dtype=torch.uint8).view(2, 27)
    y, cb, cr = ops.yuv420_planes(buf, 3, 5)
    assert y.shape == (2, 3, 5) and cb.shape == cr.shape == (2, 2, 3)
    assert y.data_ptr() == buf.data_ptr() and cb[1, 0, 0] == 27 + 15 and cr[0, 1, 2] == 26


# ---- keys and documents ------------------------------------------------------------------------------------------------------------------
def test_yaml_keys_and_their_refusals():
    assert cli.video_codec("y4m") == "y4m" == cli.video_codec(" Y4M ")
    assert cli.yuv_range(None) == "limited" == cli.yuv_range("Limited") and cli.yuv_range("full") == "full"
    assert cli.input_rate(None) == "keep" == cli.input_rate("keep") and cli.input_rate("match") == "match"
    assert cli.input_range(None) is None and cli.input_range("full") == "full" and cli.input_range("limited") == "limited"
    for fn, name in ((cli.yuv_range, "yuv_range"), (cli.input_rate, "input_rate"), (cli.input_range, "input_range")):
        for bad in ("pc", "", True, 16):
            with pytest.raises(ValueError, match=name):
                fn(bad)


def test_new_keys_are_refused_before_any_model_is_built(monkeypatch, tmp_path):
    def no_models(*a, **k):
        raise AssertionError("models were built")

    monkeypatch.setattr(cli, "build_models", no_models)
    base = dict(seed=0, synthetic=True, model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3),
                synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12))
    for key, bad in (("yuv_range", "tv"), ("input_rate", "fast"), ("input_range", "pc")):
        with pytest.raises(ValueError, match=f"{key}.*{bad}"):
            cli.run("inference", cli.Config(**base, video_codec="y4m", **{key: bad}), device=torch.device("cpu"))
    clip = str(tmp_path / "clip.y4m")
    open(clip, "wb").write(b"YUV4MPEG2 W96 H64 F0:0 C420p10\n")
    with pytest.raises(ValueError, match="C420p10"):
        cli.run("inference", cli.Config(**base, input_video=clip), device=torch.device("cpu"))
    open(clip, "wb").write(b"YUV4MPEG2 W96 H64 F0:0\n")
    with pytest.raises(ValueError, match="F0:0"):
        cli.run("inference", cli.Config(**base, input_video=clip, input_rate="match"), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="load_clip_y4m"):                  # the host route names the device route
        cli.load_clip(cli.Config(input_video=clip), 8, 12)


def test_pipeline_keyword_takes_yuv420_and_a_range():
    from longlive_amd.pipeline.causal_inference import FRAME_MODES, check_frames_mode
    assert "yuv420" in FRAME_MODES
    check_frames_mode("yuv420", 90, "limited")
    check_frames_mode("yuv420", 90, "full")
    check_frames_mode("yuv420")
    check_frames_mode("uint8", 90, "nonsense")                               # read by "yuv420" alone
    check_frames_mode("yuv420", 0, "full")                                   # as the quality is by "jpeg" alone
    for bad in ("tv", None, 1):
        with pytest.raises(ValueError, match="yuv_range"):
            check_frames_mode("yuv420", 90, bad)


def test_the_example_config_loads():
    cfg = cli.load_config(os.path.join(ROOT, "configs", "continue_y4m.yaml"))
    assert cli.video_codec(cfg.get("video_codec")) == "y4m" and cli.is_y4m_input(cfg.input_video)
    assert cli.yuv_range(cfg.get("yuv_range")) in ("limited", "full") and cli.input_rate(cfg.get("input_rate")) == "match"
    cli.input_range(cfg.get("input_range")), cli.input_fit(cfg.get("input_fit"))
    text = open(os.path.join(ROOT, "configs", "continue_y4m.yaml")).read()
    assert "ffmpeg -i" in text and "-f yuv4mpegpipe" in text and ".mp4" in text
