"""The split route through the JPEG entropy stage, host side (no GPU): the split table (longlive_amd/jpeg_files.split_segments) and its
properties, the restatement (tests/jpeg_split_ref.py) against the serial restatement's coefficients, the C-ABI boundary of the new
entry points, the yaml key, and csrc/jpeg_dec.h's resumable decoder as a stand-alone host program under AddressSanitizer and UBSan
that plays the passes next to jpeg_decode_segment."""
import ctypes as C
import functools
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_dec_ref as D
import jpeg_ref as J
import jpeg_split_ref as S
from longlive_amd import _lib, cli, jpeg_files, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ll_jpeg_decode_split_sizes": 3, "ll_jpeg_decode_coefficients_split": 21, "ll_jpeg_decode_u8_split": 26}
SUBS = (8, 16, 64, 512)


@functools.lru_cache(maxsize=None)
def _clips():
    Image = pytest.importorskip("PIL.Image")
    return S.clips(Image)


@functools.lru_cache(maxsize=None)
def _decoded(data: bytes, sub: int):
    return S.decode(data, sub)


# ---- split table ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_split_table_tiles_every_long_segment_once(sub):
    cut = 0
    for name, (files, _, _) in _clips().items():
        pk = jpeg_files.pack_jpegs(files)
        rows = jpeg_files.split_segments(pk, sub)
        assert rows.dtype == np.int32 and rows.shape[1:] == (3,), name
        first = np.cumsum([0] + [len(S.raw_segments(f)) for f in files])
        want = [(int(first[t]) + s, o, n) for t, f in enumerate(files) for s, o, n in S.split_table(S.raw_segments(f), sub)]
        assert [tuple(r) for r in rows.tolist()] == want, name
        blob = pk.data
        for s, (off, length) in enumerate(pk.segs[:, :2].tolist()):
            mine = rows[rows[:, 0] == s]
            if length < 4 * sub:
                assert mine.shape[0] == 0, (name, s)                       # short segments have no rows
                continue
            cut += 1
            assert mine.shape[0] == length // sub and mine[0, 1] == 0 and mine[-1, 1] + mine[-1, 2] == length, (name, s)
            assert np.array_equal(mine[1:, 1], mine[:-1, 1] + mine[:-1, 2]) and int(mine[:, 2].min()) >= sub - 1, (name, s)
            starts = off + mine[1:, 1]
            assert not np.any((blob[starts] == 0) & (blob[starts - 1] == 0xFF)), (name, s)       # no start on a stuffing byte
            assert np.all(np.abs(mine[:, 1] - sub * np.arange(mine.shape[0])) <= 1), (name, s)
    assert cut >= 1 or sub == 512
    for bad in (0, 4, 10, -8, True, 8.0, "8"):
        with pytest.raises(ValueError, match="sub_bytes"):
            jpeg_files.split_segments(pk, bad)


def test_a_nominal_cut_lands_on_a_stuffing_byte():
    files, sub, _ = _clips()[S.STUFFED]
    raws = S.raw_segments(files[0])
    assert S.nominal_cuts_on_stuffing(raws, sub) >= 1
    rows = jpeg_files.split_segments(jpeg_files.pack_jpegs(files), sub)
    moved = rows[rows[:, 1] % sub != 0]
    assert moved.shape[0] == S.nominal_cuts_on_stuffing(raws, sub) and np.all(moved[:, 1] % sub == 1)


# ---- restatement ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.clip_names())
def test_restatement_gives_the_serial_coefficients_and_settles(name):
    files, sub, rounds = _clips()[name]
    for data in files:
        info, coef, settled, table = _decoded(data, sub)
        assert np.array_equal(coef, D.coefficients(data)[1]), name
        assert all(0 <= r <= rounds for r in settled), (name, settled, rounds)       # the GPU test's condition: no fallback
        if name.startswith("restart3"):
            assert settled == [0] * len(settled) and len(settled) >= 10 and not table
        elif not name.startswith("mixed"):
            assert min(settled) >= 1, (name, settled)
    if name == S.UNSETTLED:
        assert max(settled) > 1                                   # the designated case: one round leaves it unsettled


def test_some_clip_needs_several_rounds_and_some_subsequence_begins_no_block():
    files, sub, _ = _clips()["noise_40x56_0_sub8"]
    info, coef, settled, table = _decoded(files[0], sub)
    assert settled[0] >= 3
    raws = S.raw_segments(files[0])
    seg = S.Segment(raws[0], info)
    _, entries, res = S.settle(seg, [(o, n) for _, o, n in table])
    assert any(b == 0 for _, b, _ in res) and any(e[2] != 0 for e in entries)      # a block spans several subsequences


# ---- ops and yaml keys ----------------------------------------------------------------------------------------------------------------------
def test_split_arguments_are_checked_on_the_host():
    assert ops._jpeg_split_bytes(None) is None and ops._jpeg_split_bytes("auto") == ops.JPEG_SPLIT_AUTO and ops._jpeg_split_bytes(64) == 64
    for bad in (0, 4, 12 + 2, True, "fast", 8.0):
        with pytest.raises(ValueError, match="split"):
            ops._jpeg_split_bytes(bad)
    assert ops._jpeg_rounds(None) == ops.JPEG_SPLIT_ROUNDS and ops._jpeg_rounds(64) == 64
    for bad in (0, 65, True, 1.0):
        with pytest.raises(ValueError, match="rounds"):
            ops._jpeg_rounds(bad)
    assert cli.input_split(None) == cli.INPUT_SPLIT_DEFAULT and cli.input_split("off") is None and cli.input_split(" Auto ") == "auto"
    assert cli.input_split(64) == 64 and cli.input_split("512") == 512
    for bad in ("on", True, 10, 4, -8, 1.5):
        with pytest.raises(ValueError, match="input_split"):
            cli.input_split(bad)
    cfg = cli.load_config(os.path.join(ROOT, "configs", "continue_footage.yaml"))
    assert "input_split" in cfg and cli.input_split(cfg.get("input_split")) == cli.INPUT_SPLIT_DEFAULT


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


def _work(nseg, nsub):
    a = C.c_longlong(-1)
    rc = _lib.load().ll_jpeg_decode_split_sizes(nseg, nsub, C.byref(a))
    return rc, a.value


def test_work_size_grows_with_both_counts():
    assert _work(1, 1) == (0, 32 * 4 + 20 * 4) and _work(5, 9)[1] == 32 * 12 + 20 * 8
    assert _work(81, 27000)[1] < 1 << 20 and _work(4, 8)[1] % 16 == 0


_E = (16, 100, 16, 1, 16, 16)                        # data, nbytes, segs, nseg, huff, sel
_G = (1, 8, 8, 3, 2, 2)                              # T, H, W, components, hs, vs
_SCR = 1 << 20
_P = (16, 192, 16, _SCR)                             # out, stride_t, scratch, scratch_bytes


def _tail(**kw):
    a = dict(subs=16, nsub=4, rounds=12, info=16, work=32, work_bytes=1 << 16, stream=None)
    a.update(kw)
    return tuple(a[k] for k in "subs nsub rounds info work work_bytes stream".split())


@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_jpeg_decode_split_sizes(1, 1, None), "ll_jpeg_decode_split_sizes: null operand"),
    (lambda L: _work(0, 1)[0], "nseg=0"),
    (lambda L: _work(1, 0)[0], "nsub=0"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(subs=0)), "ll_jpeg_decode_coefficients_split: null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(info=0)), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(work=0)), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(0, 100, 16, 1, 16, 16, *_G, 16, 16, *_tail()), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 0, *_tail()), "null operand"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(nsub=0)), "nsub=0"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(rounds=0)), "rounds=0"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(rounds=65)), "rounds=65"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(work=40)), "work must be 16-byte aligned"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(subs=18)), "subs and info must be 4-byte aligned"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 16, 16, *_tail(work_bytes=_work(1, 4)[1] - 1)), "work_bytes="),
    (lambda L: L.ll_jpeg_decode_coefficients_split(16, 1 << 31, 16, 1, 16, 16, *_G, 16, 16, *_tail()), "nbytes=2147483648"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(16, 100, 16, 0, 16, 16, *_G, 16, 16, *_tail()), "nseg=0"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, *_G, 18, 16, *_tail()), "coef must be 16-byte aligned"),
    (lambda L: L.ll_jpeg_decode_coefficients_split(*_E, 1, 8, 8, 3, 2, 4, 16, 16, *_tail()), "luma sampling 2 x 4"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, *_G, 16, 16, *_P, *_tail(subs=0)), "ll_jpeg_decode_u8_split: null operand"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 0, *_G, 16, 16, *_P, *_tail()), "ll_jpeg_decode_u8_split: null operand"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, *_G, 16, 16, 0, 192, 16, _SCR, *_tail()), "null operand"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, *_G, 16, 16, *_P, *_tail(rounds=-1)), "rounds=-1"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, *_G, 16, 16, *_P, *_tail(nsub=-3)), "nsub=-3"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, *_G, 16, 16, *_P, *_tail(work_bytes=16)), "work_bytes=16"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, *_G, 16, 16, *_P, *_tail(work=36)), "work must be 16-byte aligned"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, *_G, 16, 16, 16, 100, 16, _SCR, *_tail()), "stride_t=100"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, *_G, 16, 16, 16, 192, 16, 64, *_tail()), "scratch_bytes=64"),
    (lambda L: L.ll_jpeg_decode_u8_split(*_E, 16, 1, 8, 8, 3, 3, 1, 16, 16, *_P, *_tail()), "luma sampling 3 x 1"),
    (lambda L: L.ll_set_tuning(b"jpeg_split_lanes", 32), "jpeg_split_lanes=32"),
])
def test_invalid_arguments_are_rejected_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


# ---- csrc/jpeg_dec.h's resumable decoder under host sanitizers ------------------------------------------------------------------------------
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


def _rows(data: bytes, sub: int):
    """The split table of one segment's bytes, or the one row that covers it where it is too short to cut."""
    rows = [(o, n) for _, o, n in S.split_table([data], sub)]
    return rows or [(0, len(data))]


def _case(flags, info, seg, data, rounds, rows):
    return struct.pack("<IIiiiii", flags, int(np.frombuffer(info.sel.tobytes(), "<u4")[0]), seg[3], info.grid[2], len(data), rounds,
                       len(rows)) + info.huff.tobytes() + data + b"".join(struct.pack("<ii", *r) for r in rows)


def test_split_passes_equal_the_serial_routine_under_host_sanitizers(tmp_path):
    """A stand-alone program (its own main, tests/jpeg_split_host_main.cpp) built from csrc/jpeg_dec.h with the host compiler and
    -fsanitize=address,undefined.  Valid segments at 8 / 16 / 64 bytes (settle round = the restatement's, coefficients = the serial
    restatement's), every truncation of one segment, 2000 single-bit flips, split tables with overlapping, reversed and out-of-range
    rows, an empty segment: coefficients, status and `done` equal jpeg_decode_segment's in every case, and every buffer has its exact
    size, so a write outside the segment's blocks is the sanitizer's to report."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = _sanitizer_flags(cxx, tmp_path)
    if flags is None:
        pytest.skip("the host compiler cannot link a sanitized program of an empty main")
    exe = str(tmp_path / "jpeg_split_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "longlive_amd", "csrc"),
                            os.path.join(ROOT, "tests", "jpeg_split_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    files = [J.encode(S.textured(40, 56, 2), 90), J.encode(J.noise(24, 40, 3), 50), J.encode(J.block_checkerboard(32, 32), 100),
             J.encode(J.flat(48, 64), 90)]
    infos = [jpeg_files.parse_jpeg(f) for f in files]
    segs = [(t, s) for t, info in enumerate(infos) for s in info.segments]
    seg_bytes = lambda t, s: files[t][s[0]:s[0] + s[1]]          # noqa: E731
    ROUNDS = 64
    valid = [(t, s, sub) for t, s in segs for sub in (8, 16, 64)]
    cases = [_case(1, infos[t], s, seg_bytes(t, s), ROUNDS, _rows(seg_bytes(t, s), sub)) for t, s, sub in valid]
    t0, s0 = segs[0]
    whole = seg_bytes(t0, s0)
    cases += [_case(0, infos[t0], s0, whole[:n], 12, _rows(whole[:n], 8)) for n in range(len(whole))]       # n = 0: an empty segment
    rng = np.random.default_rng(21)
    for i in range(2000):
        t, s = segs[int(rng.integers(len(segs)))]
        d = bytearray(seg_bytes(t, s))
        bit = int(rng.integers(8 * len(d)))
        d[bit >> 3] ^= 1 << (bit & 7)
        cases.append(_case(0, infos[t], s, bytes(d), 12, _rows(bytes(d), (8, 16)[i & 1])))
    good = _rows(whole, 8)
    assert len(good) >= 6
    tables = {"overlap": good[:2] + [(good[2][0] - 4, good[2][1] + 4)] + good[3:], "reversed": good[::-1],
              "gap": good[:3] + good[4:], "past_the_end": good[:-1] + [(good[-1][0], good[-1][1] + 64)],
              "negative": [(-8, 16)] + good[1:], "short_row": good[:1] + [(good[1][0], 3), (good[1][0] + 3, good[1][1] - 3)] + good[2:],
              "huge": [(0, 0x7FFFFFFF)], "starts_late": good[1:], "stops_early": good[:-1]}
    cases += [_case(0, infos[t0], s0, whole, 12, rows) for rows in tables.values()]
    (tmp_path / "in.bin").write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    out = (tmp_path / "out.bin").read_bytes()
    want = {t: D.coefficients(f)[1].reshape(-1, infos[t].grid[2], 64) for t, f in enumerate(files)}
    pos, settled, fell = 0, [], []
    for i in range(len(cases)):
        same, status, done, info = struct.unpack_from("<iiii", out, pos)
        pos += 16
        assert same == 1, (i, status, done, info)
        if i < len(valid):
            t, s, sub = valid[i]
            n = s[3] * infos[t].grid[2]
            got = np.frombuffer(out, "<i2", n * 64, pos).reshape(-1, infos[t].grid[2], 64)
            pos += 128 * n
            assert status == 0 and done == n and np.array_equal(got, want[t][s[2]:s[2] + s[3]]), (i, status)
            rows = S.split_table([seg_bytes(t, s)], sub)
            if rows:                                              # cut: the round is the restatement's
                r = S.settle(S.Segment(seg_bytes(t, s), D.parse(files[t])), [(o, m) for _, o, m in rows])[0]
                assert info == (r if r <= ROUNDS else -1), (i, info, r)
                settled.append(info)
            else:                                                 # one row over the whole segment: settled at once
                assert info == 1, (i, info)
        else:
            fell.append((status, info))
    assert pos == len(out)
    assert len(settled) >= 8 and max(settled) >= 3 and min(settled) >= 1
    bad_tables = fell[-len(tables):]
    assert all(info == -2 and status == 0 for status, info in bad_tables), bad_tables
    flips = fell[len(whole):-len(tables)]
    assert len(flips) == 2000 and any(s for s, _ in flips) and any(i == -2 for _, i in flips) and any(i >= 1 for _, i in flips)
    assert all(i < 0 for s, i in fell if s != 0)                  # a JD_* code only ever comes from the serial routine
