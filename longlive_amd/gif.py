"""Animated previews ("Animated previews: GIF"): the GPU palette quantiser and LZW coder of csrc/gif.hip behind
tensor wrappers, and the host side of an animation -- write_gif joins single-image files into one looping GIF, read_gif_frames reads one
back through PIL.

The entry points are declared in include/longlive_gif.h and exported by the same liblonglive_hip.so under ABI version 111; this module
binds them itself on the handle of _lib.load(), so longlive_hip.h, _lib.SIGNATURES and ops.py stay as they are."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import _lib
from .ops import _call, _encode, _frames_u8, _sizes, _u8_items, jpeg_bytes

PALETTES = ("clip", "frame")        # the index is the entry points' `palette`
DITHERS = ("none", "bayer")         # ... and `dither`
CHUNK = 3584                        # csrc/gif.h: GIF_CHUNK

_p, _i, _ll = C.c_void_p, C.c_int, C.c_longlong
SIGNATURES = {                      # mirrors include/longlive_gif.h 1:1
    "ll_gif_sizes": [_i, _i, _i, _i, C.POINTER(_ll), C.POINTER(_ll)],
    "ll_gif_encode_u8": [_p, _ll, _i, _i, _i, _i, _i, _p, _ll, _p, _p, _ll, _p],
    "ll_gif_quantize_u8": [_p, _ll, _i, _i, _i, _i, _i, _p, _p, _p, _p, _ll, _p],
    "ll_gif_lzw_sizes": [_i, _ll, C.POINTER(_ll), C.POINTER(_ll)],
    "ll_gif_lzw_u8": [_p, _ll, _i, _ll, _p, _ll, _p, _p, _ll, _p],
}
_bound = False


def bind() -> C.CDLL:
    """The library's handle with the GIF entry points typed (once).  A library built before they existed is refused."""
    global _bound
    lib = _lib.load()
    if not _bound:
        missing = [name for name in SIGNATURES if not hasattr(lib, name)]
        if missing:
            raise RuntimeError(f"{_lib.LIB_PATH} does not export {', '.join(missing)}: it was built before the GIF encoder existed; "
                               "rebuild it (make -C longlive_amd/csrc)")
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True
    return lib


def _choice(key: str, value, choices) -> int:
    if value not in choices:
        raise ValueError(f"{key}: {value!r} is not one of {', '.join(choices)}")
    return choices.index(value)


def sizes(T: int, H: int, W: int, palette: str = "clip"):
    """(out_stride, scratch_bytes) of ll_gif_encode_u8 and ll_gif_quantize_u8 for T frames of H x W (host only)."""
    bind()
    return _sizes("ll_gif_sizes", T, H, W, _choice("palette", palette, PALETTES))


def lzw_sizes(T: int, n: int):
    """(out_stride, scratch_bytes) of ll_gif_lzw_u8 for T rows of n indices (host only)."""
    bind()
    return _sizes("ll_gif_lzw_sizes", T, n)


def encode(frames, palette: str = "clip", dither: str = "bayer"):
    """uint8 frames [T, H, W, 3] RGB (or a view with contiguous frames) -> (buf uint8 [T, out_stride], sizes int32 [T]): frame t's
    complete single-image GIF89a file is buf[t, :sizes[t]].  palette "clip": one table of 256 colours for the T frames, "frame": one
    each; dither "bayer": 8 x 8 ordered, fixed to the pixel's position.  Stream-ordered: nothing is read back."""
    pal, dit = _choice("palette", palette, PALETTES), _choice("dither", dither, DITHERS)
    frames, stride_t = _frames_u8(frames, "frames")
    T, H, W, _ = frames.shape
    return _encode("ll_gif_encode_u8", sizes(T, H, W, palette), frames, stride_t, T, H, W, pal, dit)


files = jpeg_bytes      # the files of encode (the streams of lzw) on the host: the same one read


def quantize(frames, palette: str = "clip", dither: str = "bayer"):
    """The encoder's first stages alone: (indices uint8 [T, H, W], palettes uint8 [T or 1, 256, 3], used int32 [T or 1])."""
    pal, dit = _choice("palette", palette, PALETTES), _choice("dither", dither, DITHERS)
    frames, stride_t = _frames_u8(frames, "frames")
    T, H, W, _ = frames.shape
    P = T if palette == "frame" else 1
    scratch_bytes = sizes(T, H, W, palette)[1]
    indices = torch.empty(T, H, W, dtype=torch.uint8, device=frames.device)
    palettes = torch.empty(P, 256, 3, dtype=torch.uint8, device=frames.device)
    used = torch.empty(P, dtype=torch.int32, device=frames.device)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=frames.device)
    _call("ll_gif_quantize_u8", frames.data_ptr(), stride_t, T, H, W, pal, dit, indices.data_ptr(), palettes.data_ptr(), used.data_ptr(),
          scratch.data_ptr(), scratch_bytes)
    return indices, palettes, used


def lzw(rows):
    """uint8 index rows [T, n] (unit stride along n, any row stride) -> (buf uint8 [T, out_stride], sizes int32 [T]): row t's GIF LZW
    stream at minimum code size 8 (before sub-blocking) is buf[t, :sizes[t]].  Stream-ordered."""
    rows, stride = _u8_items(rows, "rows", rows.dim() == 2, "[T, n]")
    T, n = rows.shape
    return _encode("ll_gif_lzw_u8", lzw_sizes(T, n), rows, stride, T, n)


# ---- the animation, on the host ----------------------------------------------------------------------------------------------------
_SCREEN, _GCE = 13, 21        # a single-image file: header + screen descriptor end at 13, the graphic control extension at 21


def _half_up(num: int, den: int) -> int:
    return (2 * num + den) // (2 * den)


def delays(count: int, every: int = 1, fps: int = 16) -> list:
    """Centiseconds each of `count` kept frames is shown when every `every`-th frame of an fps stream is kept: the differences of the
    rounded time stamps, so the rounding never accumulates (16 frames/s: 6, 7, 6, 6, ...)."""
    return [_half_up(100 * (k + 1) * every, fps) - _half_up(100 * k * every, fps) for k in range(count)]


def write_gif(path: str, files: Sequence[bytes], every: int = 1, loop: int = 0, fps: int = 16) -> int:
    """One animated GIF from complete single-image files of one size (what `encode` makes): the first file's header and screen
    descriptor, a NETSCAPE2.0 loop extension (`loop` = 0: forever), then per frame its graphic control extension with the delay set, its
    image descriptor, local colour table and data as they are, and one trailer.  `every` only sets the delays: the caller subsamples.
    Returns the file's bytes."""
    if not files:
        raise ValueError("write_gif: no frames")
    for key, v, low in (("every", every, 1), ("fps", fps, 1), ("loop", loop, 0)):
        if isinstance(v, bool) or not isinstance(v, int) or not low <= v <= 65535:
            raise ValueError(f"write_gif: {key}={v!r} must be an integer {low}..65535")
    first = files[0]
    out = [first[:_SCREEN], b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + int(loop).to_bytes(2, "little") + b"\x00"]
    for t, (data, delay) in enumerate(zip(files, delays(len(files), every, fps))):
        if data[:6] != b"GIF89a" or data[_SCREEN:_SCREEN + 3] != b"\x21\xF9\x04" or data[_GCE] != 0x2C or data[-1:] != b"\x3B":
            raise ValueError(f"write_gif: frame {t} is not a single-image file of this encoder")
        if data[:_SCREEN] != first[:_SCREEN]:
            raise ValueError(f"write_gif: frame {t}'s screen descriptor differs from frame 0's")
        if delay > 65535:
            raise ValueError(f"write_gif: a delay of {delay} centiseconds does not fit the format")
        out.append(data[_SCREEN:_SCREEN + 4] + delay.to_bytes(2, "little") + data[_SCREEN + 6:_GCE])
        out.append(data[_GCE:-1])
    out.append(b"\x3B")
    blob = b"".join(out)
    with open(path, "wb") as f:
        f.write(blob)
    return len(blob)


def read_gif_frames(path: str) -> torch.Tensor:
    """uint8 [T, H, W, 3] RGB frames of a GIF file through PIL, each frame as a viewer composes it."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        frames = []
        for t in range(getattr(im, "n_frames", 1)):
            im.seek(t)
            frames.append(torch.from_numpy(np.asarray(im.convert("RGB")).copy()))
    return torch.stack(frames)
