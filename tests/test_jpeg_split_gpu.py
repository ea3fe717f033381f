"""The split route through the JPEG entropy stage on the GPU (csrc/jpeg_dec.hip: subsequences of a restart segment decode side by
side) against the serial route, the serial restatement's coefficients (tests/jpeg_dec_ref.py) and the split restatement's settle rounds
(tests/jpeg_split_ref.py).  Only well-formed files reach a kernel here; malformed data, bad split tables and truncations are the host
program's (tests/test_jpeg_split_host.py).  The clips are chosen, and checked on the CPU there and here, so that the restatement settles
within `rounds` for every segment: `info` must then name that round exactly, so no fallback can hide a wrong split route.  Status: both
routes run with check=True, which raises on any non-zero status, so equal means all zero on both."""
import functools

import numpy as np
import pytest
import torch

import jpeg_dec_ref as D
import jpeg_ref as J
import jpeg_split_ref as S
from longlive_amd import _lib, cli, jpeg_files, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, IGUARD, BGUARD = 0x7FFF, -77, 0xA5


@functools.lru_cache(maxsize=None)
def _clips():
    Image = pytest.importorskip("PIL.Image")
    return S.clips(Image)


@functools.lru_cache(maxsize=None)
def _expected(files: tuple, sub: int):
    """(coefficients int16 [T, rows, cols, bpm, 64] of the serial restatement, settle round per segment of the split restatement)."""
    coef, rounds = [], []
    for data in files:
        _, c, r, _ = S.decode(data, sub)
        assert np.array_equal(c, D.coefficients(data)[1])
        coef.append(c)
        rounds += r
    return torch.from_numpy(np.stack(coef)), rounds


class Guarded:
    """coef, info and work inside guard fields; every call decodes into the same (by then dirty) buffers."""

    def __init__(self, files, sub, slack=0):
        pk = jpeg_files.pack_jpegs(files)
        self.shape = (pk.frames, *pk.grid, 64)
        self.n, self.nseg, self.g = int(np.prod(self.shape)), pk.segs.shape[0], 192
        nsub = max(jpeg_files.split_segments(pk, sub).shape[0], 1)
        self.work_bytes = ops.jpeg_decode_sizes(pk.frames, pk.height, pk.width, pk.components, pk.hs, pk.vs, split=(self.nseg, nsub))[2] + slack
        self.cbuf = torch.full((self.n + 2 * self.g,), GUARD, dtype=torch.int16, device=DEV)
        self.ibuf = torch.full((self.nseg + 2 * self.g,), IGUARD, dtype=torch.int32, device=DEV)
        self.wbuf = torch.full((self.work_bytes + 2 * self.g,), BGUARD, dtype=torch.uint8, device=DEV)
        assert (self.wbuf.data_ptr() + self.g) % 16 == 0

    def views(self):
        g = self.g
        return self.cbuf[g:g + self.n].view(self.shape), self.ibuf[g:g + self.nseg], self.wbuf[g:g + self.work_bytes]

    def intact(self):
        g = self.g
        return all(bool((b[:g] == v).all()) and bool((b[g + n:] == v).all())
                   for b, n, v in ((self.cbuf, self.n, GUARD), (self.ibuf, self.nseg, IGUARD), (self.wbuf, self.work_bytes, BGUARD)))


def _same_pixels(files, sub, rounds, want_info):
    T = len(files)
    pk = jpeg_files.pack_jpegs(files)
    frame, g = pk.height * pk.width * 3, 128
    buf = torch.full((2 * g + T * frame,), BGUARD, dtype=torch.uint8, device=DEV)
    view = buf[g:g + T * frame].view(T, pk.height, pk.width, 3)
    out, info = ops.jpeg_decode(files, split=sub, rounds=rounds, out=view, return_info=True)
    assert out.data_ptr() == view.data_ptr() and torch.equal(view, ops.jpeg_decode(files))
    assert info.cpu().tolist() == want_info
    assert bool((buf[:g] == BGUARD).all()) and bool((buf[g + T * frame:] == BGUARD).all())


@pytest.mark.parametrize("name", S.clip_names())
def test_split_route_equals_the_serial_route_and_settles_as_restated(name):
    files, sub, rounds = _clips()[name]
    want, want_info = _expected(tuple(files), sub)
    assert all(0 <= r <= rounds for r in want_info), (name, want_info)           # the restatement settles: nothing may fall back
    box = Guarded(files, sub)
    coef, info, work = box.views()
    got = ops.jpeg_decode_coefficients(files, out=coef, split=sub, rounds=rounds, info=info, work=work)
    assert got.data_ptr() == coef.data_ptr()
    assert info.cpu().tolist() == want_info, name
    assert torch.equal(coef, ops.jpeg_decode_coefficients(files)) and torch.equal(coef.cpu(), want), name
    assert box.intact(), name
    if name.startswith("restart3"):
        assert want_info == [0] * len(want_info)                                  # every segment is too short to cut
    _same_pixels(files, sub, rounds, want_info)


def test_one_round_leaves_the_designated_clip_unsettled_and_the_result_equal():
    files, sub, _ = _clips()[S.UNSETTLED]
    want, want_info = _expected(tuple(files), sub)
    assert len(want_info) == 1 and want_info[0] > 1                              # the restatement: not settled after one round
    box = Guarded(files, sub)
    coef, info, work = box.views()
    ops.jpeg_decode_coefficients(files, out=coef, split=sub, rounds=1, info=info, work=work)
    assert info.cpu().tolist() == [-1] and torch.equal(coef.cpu(), want) and box.intact()
    ops.jpeg_decode_coefficients(files, out=coef, split=sub, rounds=want_info[0] - 1, info=info, work=work)
    assert info.cpu().tolist() == [-1] and torch.equal(coef.cpu(), want)          # one round short is still unsettled
    ops.jpeg_decode_coefficients(files, out=coef, split=sub, rounds=want_info[0], info=info, work=work)
    assert info.cpu().tolist() == want_info and torch.equal(coef.cpu(), want) and box.intact()
    _same_pixels(files, sub, 1, [-1])


def test_a_nominal_cut_on_a_stuffing_byte_is_exercised():
    files, sub, rounds = _clips()[S.STUFFED]
    pk = jpeg_files.pack_jpegs(files)
    rows = jpeg_files.split_segments(pk, sub)
    moved = rows[rows[:, 1] % sub == 1]
    assert moved.shape[0] >= 1                                                    # the input still exercises the moved cut
    at = pk.segs[moved[:, 0], 0] + moved[:, 1]
    assert np.all(pk.data[at - 1] == 0) and np.all(pk.data[at - 2] == 0xFF)
    want, want_info = _expected(tuple(files), sub)
    got, info = ops.jpeg_decode_coefficients(files, split=sub, rounds=rounds, return_info=True)
    assert torch.equal(got.cpu(), want) and info.cpu().tolist() == want_info


def test_a_second_clip_into_dirty_work_and_scratch():
    Image = pytest.importorskip("PIL.Image")
    first = [D.pil_file(Image, S.textured(40, 56, s), 2, quality=75) for s in (1, 2)]
    second = [D.pil_file(Image, J.noise(40, 56, s), 2, quality=30) for s in (11, 12)]
    sub, rounds = 8, 64
    box = Guarded(first, sub, slack=4096)                                         # room for the longer table of the second clip
    coef, info, work = box.views()
    planes = torch.full((ops.jpeg_decode_sizes(2, 40, 56, 3, 2, 2)[1],), 0xFF, dtype=torch.uint8, device=DEV)
    for files in (first, second, first):
        want, want_info = _expected(tuple(files), sub)
        assert all(1 <= r <= rounds for r in want_info)
        out, got_info = ops.jpeg_decode(files, split=sub, rounds=rounds, scratch=(coef, planes, work), info=info, return_info=True)
        assert got_info.data_ptr() == info.data_ptr() and info.cpu().tolist() == want_info
        assert torch.equal(coef.cpu(), want) and torch.equal(out, ops.jpeg_decode(files)) and box.intact()


@pytest.mark.parametrize("lanes", [1, 64])
def test_both_lane_counts_per_wave(lanes):
    lib = _lib.load()
    try:
        assert lib.ll_set_tuning(b"jpeg_split_lanes", lanes) == 0
        for name in ("mixed_tables_48x80_sub16", "textured_96x136_2_sub64", "noise_40x56_grey_sub8"):
            files, sub, rounds = _clips()[name]
            want, want_info = _expected(tuple(files), sub)
            got, info = ops.jpeg_decode_coefficients(files, split=sub, rounds=rounds, return_info=True)
            assert torch.equal(got.cpu(), want) and info.cpu().tolist() == want_info, (lanes, name)
    finally:
        assert lib.ll_set_tuning(b"jpeg_split_lanes", 0) == 0


def test_auto_and_the_default_rounds(monkeypatch):
    files, _, _ = _clips()["noise_96x136_0_sub512"]
    want, want_info = _expected(tuple(files), ops.JPEG_SPLIT_AUTO)
    assert all(1 <= r <= ops.JPEG_SPLIT_ROUNDS for r in want_info)
    out, info = ops.jpeg_decode(files, split="auto", return_info=True)
    assert info.cpu().tolist() == want_info and torch.equal(out, ops.jpeg_decode(files))
    monkeypatch.setattr(ops, "JPEG_SPLIT_AUTO_SEGMENTS", 1)                       # a clip with that many segments is left to them
    out, info = ops.jpeg_decode(files, split="auto", return_info=True)
    assert info.cpu().tolist() == [0] and torch.equal(out, ops.jpeg_decode(files))
    out, info = ops.jpeg_decode(files, split=ops.JPEG_SPLIT_AUTO, return_info=True)         # an explicit size is always honoured
    assert info.cpu().tolist() == want_info
    with pytest.raises(ValueError, match="split"):
        ops.jpeg_decode(files, return_info=True)


def test_cli_input_split_gives_the_same_clip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    files = [D.pil_file(Image, S.textured(48, 80, s), 2, quality=90) for s in range(5)]
    cli.write_avi_mjpeg(str(tmp_path / "clip.avi"), files, 80, 48)
    cfg = cli.Config(input_video=str(tmp_path / "clip.avi"), input_decode="gpu", input_split="off")
    want, size = cli.load_clip_device(cfg, 6, 10, torch.device(DEV))
    assert size is None and want.shape == (5, 48, 80, 3) and torch.equal(want, ops.jpeg_decode(files))
    cfg.input_split = 64
    got, _ = cli.load_clip_device(cfg, 6, 10, torch.device(DEV))
    assert torch.equal(got, want)
    assert jpeg_files.split_segments(jpeg_files.pack_jpegs(files), 64).shape[0] > 5         # and 64 bytes did cut these frames
    cfg.input_split = "auto"
    assert torch.equal(cli.load_clip_device(cfg, 6, 10, torch.device(DEV))[0], want)
