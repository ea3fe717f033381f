"""Clip intake on the GPU, host side (no GPU): the restatement (tests/jpeg_dec_ref.py) against the encoder's restatement and against
Pillow's decoder, the marker parser and segment table (longlive_amd/jpeg_files.py) on Pillow-made and hand-patched files, the resize
formula against torch's antialiased bilinear interpolation, the AVI chunk reader, the yaml keys, the C-ABI boundary, and the bounds
contract of csrc/jpeg_dec.h as a stand-alone host program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import jpeg_dec_ref as D
import jpeg_ref as J
from longlive_amd import _lib, cli, jpeg_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ll_jpeg_decode_sizes": 8, "ll_jpeg_decode_coefficients": 15, "ll_jpeg_decode_pixels": 13, "ll_jpeg_decode_u8": 20,
       "ll_resize_u8": 22}


def _destuffed(data: bytes, off: int, n: int) -> bytes:
    return data[off:off + n].replace(b"\xff\x00", b"\xff")


# ---- coefficient round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", J.QUALITIES)
@pytest.mark.parametrize("name", sorted(J.cases()))
def test_restatement_decodes_the_encoders_coefficients(name, quality):
    for frame in J.cases()[name]:
        info, coef = D.coefficients(J.encode(frame, quality))
        assert (info["H"], info["W"], info["hs"], info["vs"]) == (*frame.shape[:2], 2, 2)
        assert np.array_equal(coef, J.coefficients(frame, quality))


# ---- parser -------------------------------------------------------------------------------------------------------------------------------
def _check_parse(data: bytes):
    info, ref = jpeg_files.parse_jpeg(data), D.parse(data)
    assert (info.height, info.width, info.components, info.hs, info.vs) == (ref["H"], ref["W"], ref["nc"], ref["hs"], ref["vs"])
    assert info.restart_interval == ref["ri"] and info.grid == D.grid(ref)
    for c in range(ref["nc"]):
        assert np.array_equal(info.qt[c][jpeg_files.ZIGZAG], ref["qt"][c])
        for cls, key in ((0, "dc"), (1, "ac")):
            bits, vals = ref[key][c]
            tab = info.huff[2 * cls + ((int(info.sel[c]) >> (4 * cls)) & 15)]
            assert list(tab[:16]) == bits and list(tab[16:16 + len(vals)]) == vals
    rows, cols, _ = info.grid
    assert [_destuffed(data, off, n) for off, n, _, _ in info.segments] == ref["segs"]
    per = ref["ri"] or rows * cols
    assert [(m0, mc) for _, _, m0, mc in info.segments] == [(i, min(per, rows * cols - i)) for i in range(0, rows * cols, per)]
    return info


def test_parser_reads_pillows_files():
    Image = pytest.importorskip("PIL.Image")
    seen = set()
    for name, data in D.pil_cases(Image).items():
        info = _check_parse(data)
        seen.add((info.components, info.hs, info.vs, info.restart_interval > 0))
    assert seen == {(nc, hs, vs, r) for nc, hs, vs in ((1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)) for r in (False, True)}
    with pytest.raises(ValueError, match=r"frame 3: progressive \(SOF2\)"):
        jpeg_files.parse_jpeg(D.pil_file(Image, J.smooth_noise(17, 33), 2, quality=90, progressive=True), 3)


def test_parser_reads_the_encoders_files_and_packs_several():
    files = [J.encode(f, q) for f, q in zip(J.cases()["48x64_x3"], (10, 90, 100))]
    for f in files:
        _check_parse(f)
    pk = jpeg_files.pack_jpegs(files)
    assert (pk.frames, pk.height, pk.width, pk.components, pk.hs, pk.vs, pk.grid) == (3, 48, 64, 3, 2, 2, (3, 4, 6))
    assert pk.segs.shape == (9, 5) and pk.segs.dtype == np.int32 and pk.qt.shape == (3, 3, 64) and pk.qt.dtype == np.uint16
    assert pk.huff.shape == (3, 4, 272) and pk.sel.shape == (3, 4) and not np.array_equal(pk.qt[0], pk.qt[1])
    assert pk.segs[:, 2].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and pk.segs[:, 3].tolist() == [0, 4, 8] * 3 and set(pk.segs[:, 4]) == {4}
    blob = pk.data.tobytes()
    want = [s for f in files for s in D.parse(f)["segs"]]
    assert [_destuffed(blob, int(r[0]), int(r[1])) for r in pk.segs] == want
    with pytest.raises(ValueError, match="frame 1: .*differs from frame 0"):
        jpeg_files.pack_jpegs([files[0], J.encode(J.flat(16, 16), 90)])
    with pytest.raises(ValueError, match="no frames"):
        jpeg_files.pack_jpegs([])


def test_fill_bytes_before_markers_are_skipped():
    data = J.encode(J.smooth_noise(33, 17, 1), 90)               # three intervals
    rst = data.index(b"\xff\xd0", J.HEADER_BYTES)
    padded = data[:2] + b"\xff\xff" + data[2:rst] + b"\xff\xff\xff" + data[rst:-2] + b"\xff" + data[-2:]
    a, b = jpeg_files.parse_jpeg(data), jpeg_files.parse_jpeg(padded)
    assert [padded[o:o + n] for o, n, _, _ in b.segments] == [data[o:o + n] for o, n, _, _ in a.segments]


def _patched(base: bytes, at: int, new: bytes) -> bytes:
    return base[:at] + new + base[at + len(new):]


def _refusals():
    """name -> (file, what the message must say).  The base is the encoder's file, whose 613-byte header has fixed offsets: DQT at
    20, SOF0 at 154, DHT at 173, DRI at 593, SOS at 599."""
    base = J.encode(J.smooth_noise(33, 17, 1), 90)
    sof4 = b"\xff\xc0\x00\x14\x08\x00\x21\x00\x11\x04\x01\x22\x00\x02\x11\x01\x03\x11\x01\x04\x11\x01"
    rst = base.index(b"\xff\xd0", J.HEADER_BYTES)
    return {
        "sof1": (_patched(base, 155, b"\xc1"), "SOF1"),
        "sof2": (_patched(base, 155, b"\xc2"), "progressive"),
        "arithmetic": (_patched(base, 155, b"\xc9"), "arithmetic"),
        "12_bit": (_patched(base, 158, b"\x0c"), "12-bit samples"),
        "16_bit_dqt": (_patched(base, 24, b"\x10"), "16-bit quantisation"),
        "sampling": (_patched(base, 165, b"\x41"), "sampling factors"),
        "chroma_sampling": (_patched(base, 168, b"\x21"), "sampling factors"),
        "four_components": (base[:154] + sof4 + base[173:], "4 components"),
        "adobe_rgb": (base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + base[2:], "Adobe APP14"),
        "scan_of_one": (base[:599] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + base[613:], "several scans"),
        "second_scan": (base[:-2] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\x00\xff\xd9", "several scans"),
        "progression": (_patched(base, 610, b"\x01\x05"), "Ss = 1, Se = 5"),
        "huffman_undefined": (_patched(base, 177, b"\x01"), "Huffman table class 0 id 0 is referenced but never defined"),
        "quant_undefined": (_patched(base, 166, b"\x02"), "quantisation table 2 is referenced but never defined"),
        "huffman_id": (_patched(base, 607, b"\x22"), "ids 0 and 1"),
        "oversubscribed": (_patched(base, 178, b"\x02\x01\x03"), "over-subscribes"),
        "no_eoi": (base[:-2], "no EOI"),
        "rst_order": (_patched(base, rst + 1, b"\xd1"), "out of sequence"),
        "rst_count": (base[:rst] + base[rst + 2:], "restart markers"),
        "rst_without_dri": (_patched(base, 597, b"\x00\x00"), "without a restart interval"),
        "height_0": (_patched(base, 159, b"\x00\x00"), "H = 0"),
        "width_0": (_patched(base, 161, b"\x00\x00"), "W = 0"),
        "not_a_jpeg": (b"RIFF" + base, "no SOI"),
        "cut_in_header": (base[:300], "passes the end"),
    }


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_parser_refuses(name):
    data, needle = _refusals()[name]
    with pytest.raises(ValueError, match="frame 5: ") as exc:
        jpeg_files.parse_jpeg(data, 5)
    assert needle in str(exc.value), str(exc.value)


# ---- the restatement against Pillow's decoder ----------------------------------------------------------------------------------------------
def test_restatement_agrees_with_pillows_decoder(capsys):
    """Maximum difference <= 4 levels and at most 5 % of the samples off by more than 1: libjpeg's integer IDCT and fixed-point colour
    tables are not reproduced.  Measured with Pillow 12.2 (libjpeg-turbo) on these files: maximum 3, share <= 4.4 % (17 x 33, 4:2:2,
    quality 30; every other file <= 3.6 %); 4:2:2 is the worst sampling throughout."""
    Image = pytest.importorskip("PIL.Image")
    files = dict(D.pil_cases(Image))
    files.update({f"ours_{n}_q{q}": J.encode(f[0], q) for n, f in J.cases().items() for q in (50, 90)})
    worst = (0, 0.0)
    for name, data in files.items():
        d = np.abs(D.decode(data).astype(np.int64) - D.pil_decode(Image, data).astype(np.int64))
        mx, share = int(d.max()), float((d > 1).mean())
        with capsys.disabled():
            print(f"{name}: max {mx}, share above 1: {100 * share:.2f} %")
        assert mx <= 4 and share <= 0.05, (name, mx, share)
        worst = (max(worst[0], mx), max(worst[1], share))
    with capsys.disabled():
        print(f"worst: max {worst[0]}, share {100 * worst[1]:.2f} %")


# ---- resize ---------------------------------------------------------------------------------------------------------------------------------
RESIZE_GEOMETRIES = [((1, 1), (8, 8)), ((9, 7), (24, 40)), ((37, 53), (48, 80)), ((100, 60), (33, 47)), ((17, 400), (16, 16)),
                     ((270, 480), (120, 208)), ((48, 80), (48, 80)), ((64, 31), (9, 200))]


@pytest.mark.parametrize("src,dst", RESIZE_GEOMETRIES)
def test_resize_formula_is_torchs_antialiased_bilinear(src, dst):
    import torch.nn.functional as F
    x = np.random.default_rng(7).integers(0, 256, (*src, 3)).astype(np.float64)
    got = D.resize_unrounded(x, *dst, rounded=False)
    want = F.interpolate(torch.from_numpy(x).permute(2, 0, 1)[None], size=dst, mode="bilinear", antialias=True, align_corners=False)
    err = float(np.abs(got - want[0].permute(1, 2, 0).numpy()).max())
    assert err < 1e-9, err


@pytest.mark.parametrize("n_in,n_out,most", [(1, 8, 1), (400, 16, 50), (60, 47, 3), (100, 33, 6), (80, 80, 2), (7, 40, 2), (1080, 480, 5)])
def test_tap_tables_are_the_formula(n_in, n_out, most):
    from longlive_amd import ops
    start, count, w = ops.resize_taps(n_in, n_out)
    assert start.dtype == count.dtype == np.int32 and w.dtype == np.float32 and w.shape == (n_out, int(count.max()))
    assert int(count.max()) == most and int(count.min()) >= 1 and int((start + count).max()) <= n_in and int(start.min()) >= 0
    for o, (lo, wt) in enumerate(D.taps(n_in, n_out)):
        assert start[o] == lo and count[o] == len(wt)
        assert np.array_equal(w[o, :len(wt)], wt.astype(np.float32)) and not w[o, len(wt):].any()
    if n_in == n_out:
        assert np.array_equal(start, np.arange(n_in)) and np.all(w[:, 0] == 1.0) and not w[:, 1:].any()


def test_cover_windows():
    from longlive_amd import ops
    for args, want in (((64, 64, 48, 80), (13, 0, 38, 64)),         # equal sides into a wide target: rows are cut
                       ((48, 200, 48, 80), (0, 60, 48, 80)),        # wide source: columns are cut
                       ((200, 48, 48, 80), (85, 0, 29, 48)),        # tall source
                       ((96, 160, 48, 80), (0, 0, 96, 160)),        # equal aspect: the whole frame
                       ((1080, 1920, 480, 832), (0, 24, 1080, 1872)),
                       ((1, 1, 48, 80), (0, 0, 1, 1)), ((3, 1000, 480, 832), (0, 497, 3, 5))):
        assert ops.cover_window(*args) == want == D.cover_window(*args), args
        y0, x0, Hc, Wc = want
        assert 0 <= y0 and y0 + Hc <= args[0] and 0 <= x0 and x0 + Wc <= args[1]
    with pytest.raises(ValueError, match="fit"):
        ops.resize_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4), fit="contain")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resize_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.jpeg_decode([J.encode(J.flat(16, 16), 90)], device="cpu")


def test_a_failed_segment_names_its_frame():
    """What ops.jpeg_decode(check=True) does with the status it reads back (the kernels only ever see well-formed files in the GPU
    tests; malformed data is the host program's, below)."""
    from longlive_amd import ops
    pk = jpeg_files.pack_jpegs([J.encode(f, 90) for f in J.cases()["48x64_x3"]])
    ops._jpeg_status(torch.zeros(9, dtype=torch.int32), pk)
    with pytest.raises(ValueError, match=r"malformed entropy-coded data in frame 1 \(code 2\)$"):
        ops._jpeg_status(torch.tensor([0, 0, 0, 0, 2, 1, 0, 0, 0], dtype=torch.int32), pk)
    with pytest.raises(ValueError, match=r"in frames 0 \(code 5\), 2 \(code 1\)$"):
        ops._jpeg_status(torch.tensor([0, 5, 0, 0, 0, 0, 0, 0, 1], dtype=torch.int32), pk)


# ---- AVI reader, yaml keys ----------------------------------------------------------------------------------------------------------------
def test_avi_chunks_come_back_as_written(tmp_path):
    files = [J.encode(J.smooth_noise(23, 37, s), 90) for s in range(4)]
    files[1] += b"\x00" * (1 - len(files[1]) % 2)
    files[2] += b"\x00" * (len(files[2]) % 2)
    assert {len(f) % 2 for f in files} == {0, 1}
    cli.write_avi_mjpeg(str(tmp_path / "c.avi"), files, 37, 23)
    assert cli.read_avi_mjpeg_files(str(tmp_path / "c.avi")) == files
    cli.write_avi_rgb24(str(tmp_path / "raw.avi"), torch.zeros(2, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no '00dc' frame"):
        cli.read_avi_mjpeg_files(str(tmp_path / "raw.avi"))


def test_yaml_keys_refuse_bad_values():
    assert cli.input_decode(None) == "host" == cli.input_decode("host") and cli.input_decode(" GPU ") == "gpu"
    for bad in ("cuda", "", True, 1):
        with pytest.raises(ValueError, match="input_decode"):
            cli.input_decode(bad)
    assert cli.input_fit(None) is None and cli.input_fit("cover") == "cover" and cli.input_fit(" Stretch ") == "stretch"
    for bad in ("contain", "", True, 0):
        with pytest.raises(ValueError, match="input_fit"):
            cli.input_fit(bad)


def test_bad_keys_are_refused_before_any_model_is_built(monkeypatch, tmp_path):
    def no_models(*a, **k):
        raise AssertionError("models were built")

    monkeypatch.setattr(cli, "build_models", no_models)
    cfg = cli.Config(seed=0, synthetic=True, model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3),
                     synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12), input_decode="nvdec")
    with pytest.raises(ValueError, match="input_decode.*nvdec"):
        cli.run("inference", cfg, device=torch.device("cpu"))
    cfg.input_decode, cfg.input_fit = "gpu", "letterbox"
    with pytest.raises(ValueError, match="input_fit.*letterbox"):
        cli.run("inference", cfg, device=torch.device("cpu"))
    cli.write_avi_rgb24(str(tmp_path / "raw.avi"), torch.zeros(5, 64, 96, 3, dtype=torch.uint8))
    cfg.input_fit, cfg.input_video = None, str(tmp_path / "raw.avi")
    with pytest.raises(ValueError, match="input_decode: gpu reads a Motion-JPEG .avi"):
        cli.run("inference", cfg, device=torch.device("cpu"))


def test_the_footage_config_names_the_keys():
    cfg = cli.load_config(os.path.join(ROOT, "configs", "continue_footage.yaml"))
    assert cli.input_decode(cfg.get("input_decode")) == "gpu" and cli.input_fit(cfg.get("input_fit")) == "cover" and cfg.get("input_video")
    assert "input_decode" not in cli.load_config(os.path.join(ROOT, "configs", "continue_clip.yaml"))


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


def _sizes(T, H, W, nc, hs, vs):
    a, b = C.c_longlong(-1), C.c_longlong(-1)
    rc = _lib.load().ll_jpeg_decode_sizes(T, H, W, nc, hs, vs, C.byref(a), C.byref(b))
    return rc, a.value, b.value


@pytest.mark.parametrize("T,H,W,nc,hs,vs", [(1, 1, 1, 3, 2, 2), (2, 17, 33, 3, 2, 1), (3, 480, 832, 3, 2, 2), (1, 23, 37, 1, 1, 1),
                                           (2, 37, 53, 3, 1, 1)])
def test_decode_sizes_is_the_grid_formula(T, H, W, nc, hs, vs):
    rc, coef, scratch = _sizes(T, H, W, nc, hs, vs)
    rows, cols, bpm = jpeg_files.mcu_grid(H, W, nc, hs, vs)
    assert rc == 0 and coef == T * rows * cols * bpm * 128
    assert scratch >= T * rows * cols * bpm * 64 * 4 and scratch % 256 == 0          # fp32 planes, MCU padded


_E = (16, 100, 16, 1, 16, 16)                        # data, nbytes, segs, nseg, huff, sel
_G = (1, 8, 8, 3, 2, 2)                              # T, H, W, components, hs, vs
_SCR = 1 << 20
_RS = (16, 192, 8, 8, 0, 0, 8, 8, 16, 48, 4, 4, 1, 16, 16, 16, 2, 16, 16, 16, 2, None)


def _rs(**kw):
    names = "src sst Hs Ws y0 x0 Hc Wc dst dst_st Hd Wd T ys yn yw ky xs xn xw kx stream".split()
    a = dict(zip(names, _RS))
    a.update(kw)
    return tuple(a[n] for n in names)


@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_jpeg_decode_sizes(*_G, None, None), "ll_jpeg_decode_sizes: null operand"),
    (lambda L: _sizes(0, 8, 8, 3, 2, 2)[0], "empty input"),
    (lambda L: _sizes(1, 65536, 8, 3, 2, 2)[0], "at most 65535"),
    (lambda L: _sizes(1, 8, 8, 4, 1, 1)[0], "components=4"),
    (lambda L: _sizes(1, 8, 8, 3, 1, 2)[0], "luma sampling 1 x 2"),
    (lambda L: _sizes(1, 8, 8, 3, 4, 1)[0], "luma sampling 4 x 1"),
    (lambda L: _sizes(1, 8, 8, 1, 2, 2)[0], "a grey frame is 1 x 1"),
    (lambda L: _sizes(40000, 65535, 65535, 3, 1, 1)[0], "more than one call covers"),
    (lambda L: L.ll_jpeg_decode_coefficients(0, 100, 16, 1, 16, 16, *_G, 16, 16, None), "ll_jpeg_decode_coefficients: null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients(16, 100, 0, 1, 16, 16, *_G, 16, 16, None), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients(16, 100, 16, 1, 0, 16, *_G, 16, 16, None), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients(16, 100, 16, 1, 16, 0, *_G, 16, 16, None), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients(*_E, *_G, 0, 16, None), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients(*_E, *_G, 16, 0, None), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients(16, -1, 16, 1, 16, 16, *_G, 16, 16, None), "nbytes=-1"),
    (lambda L: L.ll_jpeg_decode_coefficients(16, 1 << 31, 16, 1, 16, 16, *_G, 16, 16, None), "nbytes=2147483648"),
    (lambda L: L.ll_jpeg_decode_coefficients(16, 100, 16, 0, 16, 16, *_G, 16, 16, None), "nseg=0"),
    (lambda L: L.ll_jpeg_decode_coefficients(16, 100, 18, 1, 16, 16, *_G, 16, 16, None), "4-byte aligned"),
    (lambda L: L.ll_jpeg_decode_coefficients(*_E, *_G, 18, 16, None), "coef must be 16-byte aligned"),
    (lambda L: L.ll_jpeg_decode_coefficients(*_E, 1, 8, 8, 3, 2, 4, 16, 16, None), "luma sampling 2 x 4"),
    (lambda L: L.ll_jpeg_decode_coefficients(*_E, 1, 0, 8, 3, 2, 2, 16, 16, None), "empty input"),
    (lambda L: L.ll_jpeg_decode_pixels(0, 16, *_G, 16, 192, 16, _SCR, None), "ll_jpeg_decode_pixels: null operand"),
    (lambda L: L.ll_jpeg_decode_pixels(16, 0, *_G, 16, 192, 16, _SCR, None), "null operand"),
    (lambda L: L.ll_jpeg_decode_pixels(16, 16, *_G, 0, 192, 16, _SCR, None), "null operand"),
    (lambda L: L.ll_jpeg_decode_pixels(16, 16, *_G, 16, 192, 0, _SCR, None), "null operand"),
    (lambda L: L.ll_jpeg_decode_pixels(16, 16, *_G, 16, 191, 16, _SCR, None), "stride_t=191"),
    (lambda L: L.ll_jpeg_decode_pixels(16, 16, *_G, 16, 192, 16, _sizes(*_G)[2] - 1, None), "scratch_bytes="),
    (lambda L: L.ll_jpeg_decode_pixels(16, 16, *_G, 16, 192, 24, _SCR, None), "scratch must be 16-byte aligned"),
    (lambda L: L.ll_jpeg_decode_pixels(16, 16, 1, 8, 8, 2, 1, 1, 16, 192, 16, _SCR, None), "components=2"),
    (lambda L: L.ll_jpeg_decode_u8(*_E, 0, *_G, 16, 16, 16, 192, 16, _SCR, None), "ll_jpeg_decode_u8: null operand"),
    (lambda L: L.ll_jpeg_decode_u8(*_E, 16, *_G, 16, 16, 0, 192, 16, _SCR, None), "ll_jpeg_decode_u8: null operand"),
    (lambda L: L.ll_jpeg_decode_u8(0, 100, 16, 1, 16, 16, 16, *_G, 16, 16, 16, 192, 16, _SCR, None), "ll_jpeg_decode_u8: null operand"),
    (lambda L: L.ll_jpeg_decode_u8(*_E, 16, *_G, 16, 16, 16, 100, 16, _SCR, None), "stride_t=100"),
    (lambda L: L.ll_jpeg_decode_u8(*_E, 16, *_G, 16, 16, 16, 192, 16, 64, None), "scratch_bytes=64"),
    (lambda L: L.ll_jpeg_decode_u8(*_E, 16, 1, 8, 8, 3, 3, 1, 16, 16, 16, 192, 16, _SCR, None), "luma sampling 3 x 1"),
    (lambda L: L.ll_resize_u8(*_rs(src=0)), "ll_resize_u8: null operand"),
    (lambda L: L.ll_resize_u8(*_rs(dst=0)), "ll_resize_u8: null operand"),
    (lambda L: L.ll_resize_u8(*_rs(yw=0)), "ll_resize_u8: null operand"),
    (lambda L: L.ll_resize_u8(*_rs(xs=0)), "ll_resize_u8: null operand"),
    (lambda L: L.ll_resize_u8(*_rs(T=0)), "empty input"),
    (lambda L: L.ll_resize_u8(*_rs(Hd=0)), "empty input"),
    (lambda L: L.ll_resize_u8(*_rs(Ws=65536, sst=1 << 40)), "at most 65535"),
    (lambda L: L.ll_resize_u8(*_rs(y0=1)), "crop window 8 x 8 at (1, 0) leaves"),
    (lambda L: L.ll_resize_u8(*_rs(x0=-1)), "crop window"),
    (lambda L: L.ll_resize_u8(*_rs(Wc=9)), "crop window"),
    (lambda L: L.ll_resize_u8(*_rs(Hc=0)), "crop window"),
    (lambda L: L.ll_resize_u8(*_rs(sst=191)), "src_stride_t=191"),
    (lambda L: L.ll_resize_u8(*_rs(dst_st=47)), "dst_stride_t=47"),
    (lambda L: L.ll_resize_u8(*_rs(ky=0)), "ky=0"),
    (lambda L: L.ll_resize_u8(*_rs(kx=10)), "kx=10"),
])
def test_entry_points_reject_bad_arguments_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


# ---- the bounds contract of csrc/jpeg_dec.h under host sanitizers ---------------------------------------------------------------------------
def _case(flags, info, seg, data):
    return struct.pack("<IIiii", flags, int(np.frombuffer(info.sel.tobytes(), "<u4")[0]), seg[3], info.grid[2], len(data)) + \
        info.huff.tobytes() + data


def _sanitizer_flags(cxx, tmp_path):
    """-fsanitize flags this compiler can link, the runtimes linked statically so that the program carries its own; None when a
    program of an empty main does not build with them (asked BEFORE the program under test is built, so that an error in jpeg_dec.h
    can never be read as missing tooling)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + extra
        r = subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            return flags
    return None


def test_segment_decoder_keeps_its_bounds_under_host_sanitizers(tmp_path):
    """A stand-alone program (its own main, tests/jpeg_dec_host_main.cpp) built from csrc/jpeg_dec.h with the host compiler and
    -fsanitize=address,undefined: valid segments, every truncation of one, 2000 single-bit flips and an empty segment.  The program
    reports how many blocks it decoded whole: before that index nothing is left unwritten, from it on every sample is zero, and a
    truncated segment's whole blocks are the valid segment's."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = _sanitizer_flags(cxx, tmp_path)
    if flags is None:
        pytest.skip("the host compiler cannot link a sanitized program of an empty main")
    exe = str(tmp_path / "jpeg_dec_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "longlive_amd", "csrc"),
                            os.path.join(ROOT, "tests", "jpeg_dec_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    files = [J.encode(J.smooth_noise(17, 33, 2), 90), J.encode(J.noise(23, 37, 3), 50), J.encode(J.block_checkerboard(32, 32), 100)]
    infos = [jpeg_files.parse_jpeg(f) for f in files]
    valid = [(t, s) for t, info in enumerate(infos) for s in info.segments]
    seg_bytes = lambda t, s: files[t][s[0]:s[0] + s[1]]          # noqa: E731
    cases = [_case(1, infos[t], s, seg_bytes(t, s)) for t, s in valid]
    t0, s0 = valid[0]
    whole = seg_bytes(t0, s0)
    cases += [_case(1, infos[t0], s0, whole[:n]) for n in range(len(whole))]                    # n = 0: an empty segment
    rng = np.random.default_rng(20)
    for _ in range(2000):
        t, s = valid[int(rng.integers(len(valid)))]
        d = bytearray(seg_bytes(t, s))
        bit = int(rng.integers(8 * len(d)))
        d[bit >> 3] ^= 1 << (bit & 7)
        cases.append(_case(0, infos[t], s, bytes(d)))
    (tmp_path / "in.bin").write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    out = (tmp_path / "out.bin").read_bytes()
    pos, codes, dones = 0, [], []
    want = {t: D.coefficients(f)[1].reshape(-1, infos[t].grid[2], 64) for t, f in enumerate(files)}
    bpm0, n0 = infos[t0].grid[2], s0[3] * infos[t0].grid[2]
    for i in range(len(cases)):
        status, ok, done = struct.unpack_from("<iii", out, pos)
        pos += 12
        assert ok == 1, (i, status, done)
        if i < len(valid):
            t, s = valid[i]
            n = s[3] * infos[t].grid[2]
            got = np.frombuffer(out, "<i2", n * 64, pos).reshape(-1, infos[t].grid[2], 64)
            pos += 128 * n
            assert status == 0 and done == n and np.array_equal(got, want[t][s[2]:s[2] + s[3]]), (i, status)
            continue
        assert 0 <= status <= 8
        codes.append(status)
        if i < len(valid) + len(whole):                                     # a truncation: its whole blocks are the valid segment's
            got = np.frombuffer(out, "<i2", n0 * 64, pos).reshape(n0, 64)
            pos += 128 * n0
            ref = want[t0][s0[2]:s0[2] + s0[3]].reshape(n0, 64)
            assert np.array_equal(got[:done], ref[:done]) and not got[done:].any(), (i, status, done)
            dones.append(done)
    assert pos == len(out)
    cut = codes[:len(whole)]
    assert cut[0] == 1 and all(c != 0 for c in cut[:len(whole) - 1])           # every real truncation is noticed, mostly as an overrun
    assert dones[0] == 0 and dones == sorted(dones) and dones[-1] >= n0 - 1 and len(set(dones)) > n0 // 2
    flips = codes[len(whole):]
    assert len(flips) == 2000 and any(flips) and {1, 2} & set(flips)
