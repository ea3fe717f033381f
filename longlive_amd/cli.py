"""Command-line parity with the reference's entry points:

    python -m longlive_amd.cli inference   --config_path configs/longlive_inference.yaml              (inference.py)
    python -m longlive_amd.cli interactive --config_path configs/longlive_interactive_inference.yaml  (interactive_inference.py)

Same yaml keys (configs/longlive_inference.yaml, configs/longlive_interactive_inference.yaml), same prompt file formats
(utils/dataset.py:20-42 one prompt per line; :80-123 jsonl with a "prompts" list per line), same rank partition
(DistributedSampler(shuffle=False, drop_last=True), seed + local_rank: inference.py:49,146), same `inference_iter` stop rule
(inference.py:246) and output names (`rank{r}-{idx}-{seed_idx}_{lora|ema|regular}.mp4`, inference.py:226-243).  Everything
here is host logic; the models are longlive_amd's HIP modules (generator, VAE decoder, umT5 encoder).

Extra key, because this repository cannot ship checkpoints: `synthetic: true` (or `--synthetic`) runs random-init weights
(longlive_amd.synth) and a hash tokenizer, optionally shrunk by `synthetic_overrides: {num_layers, t5_layers, lat_h, lat_w}`.

Extra keys, both modes: `input_video: <path>` continues a clip -- every prompt of the data file continues the same one -- and
`input_frames: <int>` caps how many of its frames are used (the LAST 1 + 4k frames that fit).
`video_codec: mjpeg` writes `<name>.avi` as Motion JPEG, encoded on the GPU at `jpeg_quality: 90` ("Frames
out"); without the key the video is written as before.  An MJPEG .avi is also read back as `input_video` (through PIL).
`video_codec: y4m` writes `<name>.y4m` instead: I420 frames from the decoder's last kernel (`yuv_range: limited | full`) in a
YUV4MPEG2 stream, which any ffmpeg encodes (`ffmpeg -i out.y4m out.mp4`); `input_video: clip.y4m` (or a FIFO that
`ffmpeg -i any.mp4 -f yuv4mpegpipe` writes into) is converted on the device, `input_rate: match` picks its frames by the header's
rate, `input_range: full` names the range of a header without one ("Planar YUV and Y4M").
`input_decode: gpu` decodes such a file's frames on the GPU instead (ops.jpeg_decode: baseline JPEG as this project, libjpeg, Pillow
or ffmpeg write it), and `input_fit: cover | stretch` resizes a clip of another size to the model's on the GPU (ops.resize_u8);
without the two keys intake is as before ("Clip intake on the GPU").
`video_codec: png` writes the exact frames as `<name>.frames/00000.png ...`, `video_codec: apng` as one animated `<name>.png` at
16 frames/s, both encoded on the GPU (ops.png_encode; DESIGN.md section 5c, "Lossless frames: PNG"); `input_video: clip.png` (a
still or an APNG, through PIL) continues from exactly those frames.
`gif_preview: true` writes an animated `<name>.gif` beside the video, whatever `video_codec` is: 256 colours per clip
(`gif_palette: clip | frame`), ordered dither (`gif_dither: bayer | none`), every `gif_every`-th frame, resized to `gif_size: [H, W]`,
quantised and LZW-coded on the GPU (longlive_amd.gif; DESIGN.md section 5c, "Animated previews: GIF").  It is a preview, not a codec:
`video_codec: gif` stays refused.  `input_video: clip.gif` is read through PIL.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import struct
import sys
import time
import zlib
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from .ops import YUV_RANGES
from .replicas import replica_seed, shard_prompts


# ---- config ------------------------------------------------------------------------------------------------------------
class Config(SimpleNamespace):
    """Attribute view of the yaml (what the reference gets from OmegaConf.load, inference.py:26)."""

    def get(self, key, default=None):
        return getattr(self, key, default)

    def __contains__(self, key):
        return hasattr(self, key)


def _wrap(obj):
    if isinstance(obj, dict):
        return Config(**{k: _wrap(v) for k, v in obj.items()})
    if isinstance(obj, list):
        return [_wrap(v) for v in obj]
    return obj


def load_config(path: str) -> Config:
    import yaml
    with open(path, encoding="utf-8") as f:
        raw = yaml.safe_load(f) or {}
    if not isinstance(raw, dict):
        raise ValueError(f"{path}: top level of the config must be a mapping")
    return _wrap(raw)


def parse_switch_frame_indices(value) -> List[int]:
    """interactive_inference.py:146-152: an int, or a comma-separated string ("40, 80, 120")."""
    if isinstance(value, bool):
        raise ValueError("switch_frame_indices must be an int or a comma-separated list")
    if isinstance(value, int):
        return [int(value)]
    if isinstance(value, (list, tuple)):
        return [int(v) for v in value]
    return [int(x) for x in str(value).split(",") if str(x).strip()]


# ---- prompt files ------------------------------------------------------------------------------------------------------
class TextDataset:
    """utils/dataset.py:20-42: one prompt per line (`line.rstrip()`), optional parallel file of extended prompts."""

    def __init__(self, prompt_path: str, extended_prompt_path: Optional[str] = None):
        with open(prompt_path, encoding="utf-8") as f:
            self.prompt_list = [line.rstrip() for line in f]
        self.extended_prompt_list = None
        if extended_prompt_path is not None:
            with open(extended_prompt_path, encoding="utf-8") as f:
                self.extended_prompt_list = [line.rstrip() for line in f]
            assert len(self.extended_prompt_list) == len(self.prompt_list)

    def __len__(self):
        return len(self.prompt_list)

    def __getitem__(self, idx):
        batch = {"prompts": self.prompt_list[idx], "idx": idx}
        if self.extended_prompt_list is not None:
            batch["extended_prompts"] = self.extended_prompt_list[idx]
        return batch


class MultiTextDataset:
    """utils/dataset.py:80-123: jsonl, each line `{"prompts": [segment prompts...]}`, all lines the same length."""

    def __init__(self, prompt_path: str, field: str = "prompts"):
        self.rows: List[List[str]] = []
        with open(prompt_path, encoding="utf-8") as f:
            for i, line in enumerate(f):
                if not line.strip():
                    continue
                ex = json.loads(line)
                assert field in ex, f"Missing field '{field}'"
                val = ex[field]
                assert isinstance(val, list), f"Line {i} field '{field}' is not a list"
                self.rows.append([str(v) for v in val])
        assert len(self.rows) > 0, "JSONL is empty"
        seg_len = len(self.rows[0])
        for i, val in enumerate(self.rows):
            assert len(val) == seg_len, f"Line {i} list length mismatch"
        self.field = field

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, idx: int):
        return {"idx": idx, "prompts_list": self.rows[idx]}


def rank_indices(n: int, rank: int, world: int) -> List[int]:
    """Sample order of DistributedSampler(dataset, shuffle=False, drop_last=True) on `rank` (inference.py:146), or
    SequentialSampler when world == 1."""
    return shard_prompts(list(range(n)), rank, world) if world > 1 else list(range(n))


def output_name(rank: int, idx: int, seed_idx: int, model_type: str, save_with_index: bool, prompt: str,
                interactive: bool = False, ext: str = ".mp4") -> str:
    """inference.py:236-242 / interactive_inference.py:222-229."""
    if save_with_index:
        return f"rank{rank}-{idx}-{seed_idx}_{model_type}{ext}"
    if interactive:
        return f"rank{rank}-{prompt[:100].replace('/', '_')}-{seed_idx}_{model_type}{ext}"
    return f"rank{rank}-{prompt[:100]}-{seed_idx}{ext}"


def model_type_of(config, lora_enabled: bool) -> str:
    return "lora" if lora_enabled else ("ema" if config.get("use_ema", False) else "regular")


# ---- video files -------------------------------------------------------------------------------------------------------
def _riff_chunk(tag: bytes, payload: bytes) -> bytes:
    return tag + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


def _riff_list(tag: bytes, payload: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", len(payload) + 4) + tag + payload


def write_avi_rgb24(path: str, frames: torch.Tensor, fps: int = 16) -> None:
    """Uncompressed AVI (RIFF, one 'vids' stream of bottom-up BGR24 DIBs + idx1).  frames uint8 [T, H, W, 3] RGB.
    Streamed to disk one frame at a time: all sizes are known up front, so a 3840-frame clip never exists twice in memory."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3
    T, H, W, _ = frames.shape
    stride = (W * 3 + 3) & ~3
    fsz = stride * H
    avih = struct.pack("<IIIIIIIIII4I", 1000000 // fps, fsz * fps, 0, 0x10, T, 0, 1, fsz, W, H, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"DIB ", 0, 0, 0, 0, 1, fps, 0, T, fsz, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHHIIiiII", 40, W, H, 1, 24, 0, fsz, 0, 0, 0, 0)
    strl = _riff_list(b"strl", _riff_chunk(b"strh", strh) + _riff_chunk(b"strf", strf))
    hdrl = _riff_list(b"hdrl", _riff_chunk(b"avih", avih) + strl)
    movi_len = 4 + T * (8 + fsz)                                    # 'movi' + T x ('00db' size data); fsz is even
    idx_len = 16 * T
    riff_len = 4 + len(hdrl) + 8 + movi_len + 8 + idx_len
    pad = bytes(stride - W * 3)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", riff_len) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_len) + b"movi")
        for t in range(T):
            rows = frames[t].flip(0).flip(-1).contiguous().numpy().reshape(H, W * 3)      # bottom-up rows, BGR
            f.write(b"00db" + struct.pack("<I", fsz))
            if pad:
                for r in rows:
                    f.write(r.tobytes() + pad)
            else:
                f.write(rows.tobytes())
        f.write(b"idx1" + struct.pack("<I", idx_len))
        off = 4
        for t in range(T):
            f.write(b"00db" + struct.pack("<III", 0x10, off, fsz))
            off += 8 + fsz


def read_avi_rgb24(path: str) -> torch.Tensor:
    """Inverse of write_avi_rgb24 (tests / round trips)."""
    import numpy as np
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"AVI "
    p = raw.index(b"strf") + 8
    _, W, H = struct.unpack("<Iii", raw[p:p + 12])
    stride = (W * 3 + 3) & ~3
    frames, q = [], raw.index(b"movi") + 4
    while raw[q:q + 4] == b"00db":
        n = struct.unpack("<I", raw[q + 4:q + 8])[0]
        rows = np.frombuffer(raw, dtype=np.uint8, count=n, offset=q + 8).reshape(H, stride)[:, :W * 3].reshape(H, W, 3)
        frames.append(torch.from_numpy(rows[::-1, :, ::-1].copy()))
        q += 8 + n
    return torch.stack(frames, 0)


AVI_LIMIT = (1 << 32) - 8                           # riff_len: the whole file, RIFF header included, stays within 4 GiB


def _avi_mjpeg_layout(sizes: Sequence[int], hdrl_len: int):
    """(movi_len, idx_len, riff_len) of an MJPEG AVI with these frame sizes: every frame is '00dc' + length + data padded to even."""
    movi_len = 4 + sum(8 + n + (n & 1) for n in sizes)
    idx_len = 16 * len(sizes)
    return movi_len, idx_len, 4 + hdrl_len + 8 + movi_len + 8 + idx_len


def write_avi_mjpeg(path: str, frames: Sequence[bytes], width: int, height: int, fps: int = 16) -> int:
    """Motion-JPEG AVI: one 'vids' stream (fccHandler and biCompression 'MJPG') of '00dc' chunks, each one complete JPEG file padded to
    even length, + idx1 with the true sizes.  Frames are written as they come; all lengths are known from the frames' sizes up front,
    and a file that would pass 4 GiB is refused before anything is written.  Returns the file's size in bytes."""
    sizes = [len(f) for f in frames]
    T = len(sizes)
    if T < 1:
        raise ValueError("write_avi_mjpeg: no frames")
    biggest = max(sizes)
    avih = struct.pack("<IIIIIIIIII4I", 1000000 // fps, biggest * fps, 0, 0x10, T, 0, 1, biggest, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, T, biggest, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    strl = _riff_list(b"strl", _riff_chunk(b"strh", strh) + _riff_chunk(b"strf", strf))
    hdrl = _riff_list(b"hdrl", _riff_chunk(b"avih", avih) + strl)
    movi_len, idx_len, riff_len = _avi_mjpeg_layout(sizes, len(hdrl))
    if riff_len > AVI_LIMIT:
        fit = T
        while fit > 0 and _avi_mjpeg_layout(sizes[:fit], len(hdrl))[2] > AVI_LIMIT:
            fit -= 1
        raise ValueError(f"write_avi_mjpeg: {T} frames make a {riff_len + 8}-byte file, past the 4 GiB an AVI can hold; "
                         f"the first {fit} frames fit")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", riff_len) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_len) + b"movi")
        for data in frames:
            f.write(b"00dc" + struct.pack("<I", len(data)))
            f.write(data)
            if len(data) & 1:
                f.write(b"\x00")
        f.write(b"idx1" + struct.pack("<I", idx_len))
        off = 4
        for n in sizes:
            f.write(b"00dc" + struct.pack("<III", 0x10, off, n))
            off += 8 + n + (n & 1)
    return riff_len + 8


def avi_compression(path: str) -> bytes:
    """biCompression of the first stream's `strf` chunk as four bytes (b"\\0\\0\\0\\0" = uncompressed RGB)."""
    with open(path, "rb") as f:
        head = f.read(4096)
    if head[:4] != b"RIFF" or head[8:12] != b"AVI " or b"strf" not in head:
        raise ValueError(f"{path!r} is not an AVI file")
    p = head.index(b"strf") + 8
    return head[p + 16:p + 20]


def read_avi_mjpeg(path: str) -> torch.Tensor:
    """uint8 [T, H, W, 3] RGB frames of a Motion-JPEG AVI (write_avi_mjpeg), each decoded by PIL."""
    try:
        from PIL import Image                       # noqa: WPS433 (optional dependency)
    except ImportError:
        raise RuntimeError(f"input_video: reading the MJPEG file {path!r} needs PIL (Pillow) to decode its frames; without it the "
                           f"formats read are an uncompressed RGB24 .avi and a .pt holding a uint8 [T, H, W, 3] tensor") from None
    import io
    import numpy as np
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"AVI "
    frames, q = [], raw.index(b"movi") + 4
    while raw[q:q + 4] == b"00dc":
        n = struct.unpack("<I", raw[q + 4:q + 8])[0]
        img = Image.open(io.BytesIO(raw[q + 8:q + 8 + n]))
        frames.append(torch.from_numpy(np.array(img.convert("RGB"), dtype=np.uint8)))
        q += 8 + n + (n & 1)
    if not frames:
        raise ValueError(f"input_video: {path!r} holds no '00dc' frame")
    return torch.stack(frames, 0)


def read_avi_mjpeg_files(path: str) -> List[bytes]:
    """The '00dc' chunks of a Motion-JPEG AVI, undecoded: one complete JPEG file per frame (what write_avi_mjpeg was given)."""
    raw = open(path, "rb").read()
    if raw[:4] != b"RIFF" or raw[8:12] != b"AVI " or b"movi" not in raw:
        raise ValueError(f"input_video: {path!r} is not an AVI file")
    files, q = [], raw.index(b"movi") + 4
    while raw[q:q + 4] == b"00dc":
        n = struct.unpack("<I", raw[q + 4:q + 8])[0]
        files.append(raw[q + 8:q + 8 + n])
        q += 8 + n + (n & 1)
    if not files:
        raise ValueError(f"input_video: {path!r} holds no '00dc' frame")
    return files


def _one_of(key: str, value, choices, default, absent: str = ""):
    """A yaml key that names one of `choices` (absent = default), refused by name otherwise."""
    if value is None:
        return default
    v = str(value).strip().lower()
    if isinstance(value, bool) or v not in choices:
        raise ValueError(f"{key}: {value!r} is not one of {', '.join(choices)}{absent}")
    return v


INPUT_DECODES = ("host", "gpu")
INPUT_FITS = ("cover", "stretch")


def input_decode(value) -> str:
    """The yaml's `input_decode:` key: absent / host = MJPEG frames decoded by PIL, gpu = by ops.jpeg_decode."""
    return _one_of("input_decode", value, INPUT_DECODES, "host", " (or absent)")


def input_fit(value) -> Optional[str]:
    """The yaml's `input_fit:` key: absent = a clip of another size is refused, cover / stretch = ops.resize_u8's `fit`."""
    return _one_of("input_fit", value, INPUT_FITS, None, " (or absent)")


INPUT_SPLIT_DEFAULT = "auto"    # what an absent `input_split:` means: None = off, or "auto" (DESIGN.md section 5c holds the measurement)


def input_split(value):
    """The yaml's `input_split:` key for `input_decode: gpu`: off = one lane per restart segment (None), auto = ops.jpeg_decode's
    split="auto", an integer = that many bytes per subsequence (a multiple of 4, at least 8); absent = INPUT_SPLIT_DEFAULT."""
    if value is None:
        return INPUT_SPLIT_DEFAULT
    if value is False:                                  # a bare `off` in yaml 1.1 is the boolean
        return None
    v = str(value).strip().lower()
    if not isinstance(value, bool) and isinstance(value, (int, str)):
        if v == "off":
            return None
        if v == "auto":
            return "auto"
        if v.isdigit() and int(v) >= 8 and int(v) % 4 == 0:
            return int(v)
    raise ValueError(f"input_split: {value!r} is not auto, off or a number of bytes (a multiple of 4, at least 8)")


def yuv_range(value) -> str:
    """The yaml's `yuv_range:` key for `video_codec: y4m`: limited (default) | full."""
    return _one_of("yuv_range", value, YUV_RANGES, "limited")


def input_range(value) -> Optional[str]:
    """The yaml's `input_range:` key: the range of a .y4m `input_video` whose header has no XCOLORRANGE tag (absent = limited)."""
    return _one_of("input_range", value, YUV_RANGES, None)


def input_rate(value) -> str:
    """The yaml's `input_rate:` key for a .y4m `input_video`: keep (default) = its last frames as they are (select_clip_frames),
    match = frames picked at the header's rate so that the clip plays at 16 frames/s (y4m.select_frames_at_rate)."""
    return _one_of("input_rate", value, ("keep", "match"), "keep")


def is_y4m_input(path) -> bool:
    """A `.y4m` file, or a FIFO (what `ffmpeg -f yuv4mpegpipe` writes into)."""
    import stat
    path = str(path)
    if os.path.splitext(path)[1].lower() == ".y4m":
        return True
    try:
        return stat.S_ISFIFO(os.stat(path).st_mode)
    except OSError:
        return False


VIDEO_CODECS = ("mjpeg", "y4m", "png", "apng")


def video_codec(value) -> Optional[str]:
    """The yaml's `video_codec:` key: absent / none = write_video's path, `mjpeg` = Motion JPEG in an .avi from the GPU encoder,
    `y4m` = I420 frames from the decoder's last kernel in a YUV4MPEG2 stream (`ffmpeg -i out.y4m out.mp4` makes an mp4 of it),
    `png` = one lossless PNG file per frame from the GPU encoder, `apng` = the same frames as one animated PNG."""
    if str(value).strip().lower() == "none":                    # the word, or the absent key
        return None
    return _one_of("video_codec", value, VIDEO_CODECS, None, " (or absent)")


def jpeg_quality(value) -> int:
    """The yaml's `jpeg_quality:` key (1..100, default 90)."""
    from .pipeline.frames_out import check_jpeg_quality
    return 90 if value is None else check_jpeg_quality(value)


def write_video(path: str, frames: torch.Tensor, fps: int = 16) -> str:
    """torchvision.io.write_video(path, uint8 [T,H,W,C], fps) (inference.py:243) when torchvision + PyAV exist; otherwise
    the same frames as an uncompressed .avi next to the requested name.  Returns the path written."""
    frames = frames.to(torch.uint8).cpu()
    try:
        from torchvision.io import write_video as tv_write          # noqa: WPS433 (optional dependency)
        import av                                                   # noqa: F401  (what torchvision's writer needs)
    except ImportError:                                             # torchvision / PyAV missing: keep the frames anyway
        alt = os.path.splitext(path)[0] + ".avi"
        write_avi_rgb24(alt, frames, fps)
        return alt
    tv_write(path, frames, fps=fps)                                 # real I/O errors propagate
    return path


# One writer per `video_codec`: (run()'s .mp4 name, one sample's frames in the form the pipeline was asked for) -> (the path written,
# its frame count, the record's codec keys).  Absent key: uint8 [T', H, W, 3] on the host; mjpeg, png, apng: the same on the device;
# y4m: I420.
def _write_default(path: str, frames: torch.Tensor):
    return write_video(path, frames, fps=16), int(frames.shape[0]), {}


def _write_mjpeg(path: str, frames: torch.Tensor, quality: int):
    from . import ops
    files = ops.jpeg_bytes(*ops.jpeg_encode(frames, quality))
    path = os.path.splitext(path)[0] + ".avi"
    size = write_avi_mjpeg(path, files, int(frames.shape[2]), int(frames.shape[1]), fps=16)
    return path, len(files), {"codec": "mjpeg", "bytes": size}


def _write_y4m(path: str, frames: torch.Tensor, width: int, height: int, out_range: str):
    from . import y4m
    host = frames.cpu().numpy()                                     # I420 [T', bytes]: written frame by frame
    path = os.path.splitext(path)[0] + ".y4m"
    size = y4m.write_y4m(path, iter(host), width, height, fps=16, range=out_range)
    return path, int(host.shape[0]), {"codec": "y4m", "bytes": size, "range": out_range}


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_chunks(data: bytes) -> List:
    """[(type, payload)] of a PNG file; the signature and every chunk's length and CRC-32 are checked."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("png_chunks: not a PNG file")
    at, out = 8, []
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError(f"png_chunks: a chunk header at byte {at} passes the end of the file")
        n, = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        if at + 12 + n > len(data) or struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != zlib.crc32(kind + payload):
            raise ValueError(f"png_chunks: the {kind!r} chunk at byte {at} is cut short or fails its CRC-32")
        out.append((kind, payload))
        at += 12 + n
    return out


def write_apng(path: str, files: Sequence[bytes], fps: int = 16) -> int:
    """One animated PNG from complete PNG files of one size and format (what ops.png_encode makes): the first file's IHDR, acTL, then
    per frame an fcTL and its image data -- the first frame's IDAT chunks as they are, later frames' re-wrapped as fdAT behind a
    sequence number, which changes their CRC-32s (recomputed here, on the host) -- and IEND.  Returns the file's bytes."""
    if not files:
        raise ValueError("write_apng: no frames")
    if isinstance(fps, bool) or not isinstance(fps, int) or not 1 <= fps <= 65535:
        raise ValueError(f"write_apng: fps={fps!r} must be an integer 1..65535")
    parsed = [png_chunks(f) for f in files]
    ihdr = parsed[0][0]
    if ihdr[0] != b"IHDR":
        raise ValueError("write_apng: frame 0 does not begin with IHDR")
    width, height = struct.unpack(">II", ihdr[1][:8])
    out = [b"\x89PNG\r\n\x1a\n", _png_chunk(*ihdr), _png_chunk(b"acTL", struct.pack(">II", len(files), 0))]
    seq = 0
    for t, chunks in enumerate(parsed):
        if chunks[0] != ihdr:
            raise ValueError(f"write_apng: frame {t}'s IHDR differs from frame 0's")
        out.append(_png_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, width, height, 0, 0, 1, fps, 0, 0)))
        seq += 1
        for kind, payload in chunks:
            if kind != b"IDAT":
                continue
            if t == 0:
                out.append(_png_chunk(b"IDAT", payload))
            else:
                out.append(_png_chunk(b"fdAT", struct.pack(">I", seq) + payload))
                seq += 1
    out.append(_png_chunk(b"IEND", b""))
    blob = b"".join(out)
    with open(path, "wb") as f:
        f.write(blob)
    return len(blob)


def read_png_frames(path: str) -> torch.Tensor:
    """uint8 [T, H, W, 3] RGB frames of a PNG file through PIL: a still gives one frame, an APNG all of its frames."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        frames = []
        for t in range(getattr(im, "n_frames", 1)):
            im.seek(t)
            frames.append(torch.from_numpy(np.asarray(im.convert("RGB")).copy()))
    return torch.stack(frames)


def _write_png(path: str, frames: torch.Tensor):
    from . import ops
    files = ops.png_bytes(*ops.png_encode(frames))
    folder = os.path.splitext(path)[0] + ".frames"
    os.makedirs(folder, exist_ok=True)
    for t, data in enumerate(files):
        with open(os.path.join(folder, f"{t:05d}.png"), "wb") as f:
            f.write(data)
    return folder, len(files), {"codec": "png", "bytes": sum(len(d) for d in files)}


def _write_apng(path: str, frames: torch.Tensor):
    from . import ops
    files = ops.png_bytes(*ops.png_encode(frames))
    path = os.path.splitext(path)[0] + ".png"
    return path, len(files), {"codec": "apng", "bytes": write_apng(path, files, fps=16)}


class GifPreview(NamedTuple):
    """The yaml's `gif_*` keys, checked: keep every `every`-th frame, resize to `size` = (H, W) (None: the video's), `palette` clip |
    frame, `dither` bayer | none (gif.encode's)."""
    every: int
    size: Optional[tuple]
    palette: str
    dither: str


def gif_preview(config) -> Optional[GifPreview]:
    """The yaml's `gif_preview: true` and the keys that shape it (`gif_every`, `gif_size: [H, W]`, `gif_palette`, `gif_dither`): an
    animated `<name>.gif` beside whatever `video_codec` writes.  None without `gif_preview`; the other keys are checked either way."""
    from . import gif
    on = config.get("gif_preview")
    if on is not None and not isinstance(on, bool):
        raise ValueError(f"gif_preview: {on!r} must be true or false")
    every = config.get("gif_every")
    if every is not None and (isinstance(every, bool) or not isinstance(every, int) or every < 1):
        raise ValueError(f"gif_every: {every!r} must be an integer >= 1")
    size = config.get("gif_size")
    if size is not None:
        ok = isinstance(size, (list, tuple)) and len(size) == 2 and all(
            isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= 65535 for v in size)
        if not ok:
            raise ValueError(f"gif_size: {size!r} must be [H, W], two integers 1..65535")
        size = (int(size[0]), int(size[1]))
    palette = _one_of("gif_palette", config.get("gif_palette"), gif.PALETTES, "clip")
    dither = _one_of("gif_dither", config.get("gif_dither"), gif.DITHERS, "bayer")
    return GifPreview(1 if every is None else every, size, palette, dither) if on else None


def _preview_frames(frames: torch.Tensor, codec: Optional[str], width: int, height: int, out_range: str, device) -> torch.Tensor:
    """One sample's frames in the form `video_codec` asked the pipeline for -> uint8 [T', H, W, 3] on the device."""
    from . import ops
    if codec != "y4m":
        return frames.to(device)                                    # absent key: the host's uint8 frames go up again
    y, c = height * width, (height // 2) * (width // 2)             # I420 payloads [T', bytes]
    return ops.yuv_to_frames_u8(frames[:, :y].unflatten(1, (height, width)), frames[:, y:y + c].unflatten(1, (height // 2, width // 2)),
                                frames[:, y + c:].unflatten(1, (height // 2, width // 2)), layout="420jpeg", range=out_range)


def _write_gif_preview(path: str, frames: torch.Tensor, preview: GifPreview) -> Dict:
    """`<name>.gif` beside the video: every `every`-th frame, resized when asked, quantised and coded on the GPU (gif.encode), joined on
    the host (gif.write_gif).  Returns the record's keys."""
    from . import gif, ops
    kept = frames[::preview.every]
    if preview.size is not None and preview.size != tuple(kept.shape[1:3]):
        kept = ops.resize_u8(kept, preview.size, fit="stretch")
    path = os.path.splitext(path)[0] + ".gif"
    size = gif.write_gif(path, gif.files(*gif.encode(kept, preview.palette, preview.dither)), every=preview.every, fps=16)
    return {"gif": path, "gif_bytes": size}


def input_frames(cap) -> Optional[int]:
    """The yaml's `input_frames:` key: at most so many frames of the clip are used (absent = all of them)."""
    if cap is not None and (isinstance(cap, bool) or not isinstance(cap, int) or cap < 1):
        raise ValueError(f"input_frames: {cap!r} must be an integer >= 1")
    return cap


def select_clip_frames(total: int, cap: Optional[int] = None) -> slice:
    """Which frames of a `total`-frame clip are continued: the last 1 + 4k with the largest k that fits the clip and the cap (the
    VAE encoder takes 1 frame, then 4 per latent).  The END of the clip is what gets continued, so frames are dropped at the front."""
    if isinstance(total, bool) or int(total) < 1:
        raise ValueError(f"input_video: the clip holds {total} frames, at least 1 is needed")
    room = int(total) if input_frames(cap) is None else min(int(total), cap)
    used = 1 + 4 * ((room - 1) // 4)
    return slice(int(total) - used, int(total))


def read_input_video(path: str) -> torch.Tensor:
    """uint8 [T, H, W, 3] RGB frames of `path`: an .avi as write_avi_rgb24 or write_avi_mjpeg writes it (chosen by the `strf` chunk's
    biCompression), a .png (a still or an APNG, through PIL), a .gif (through PIL), a .pt holding such a tensor, anything else through
    torchvision.io.read_video when torchvision + PyAV exist."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".avi":
        frames = read_avi_mjpeg(path) if avi_compression(path) == b"MJPG" else read_avi_rgb24(path)
    elif ext == ".png":
        frames = read_png_frames(path)
    elif ext == ".gif":
        from .gif import read_gif_frames
        frames = read_gif_frames(path)
    elif ext == ".pt":
        frames = torch.load(path, map_location="cpu", weights_only=True)      # a bare tensor: nothing is unpickled
    else:
        try:
            from torchvision.io import read_video as tv_read        # noqa: WPS433 (optional dependency)
            import av                                               # noqa: F401  (what torchvision's reader needs)
        except ImportError:
            raise RuntimeError(f"input_video: cannot read {path!r} without torchvision + PyAV; the formats read without them "
                               f"are an uncompressed RGB24 .avi (write_avi_rgb24) and a .pt holding a uint8 [T, H, W, 3] tensor") from None
        frames = tv_read(path, pts_unit="sec", output_format="THWC")[0]
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        what = f"{frames.dtype} {tuple(frames.shape)}" if torch.is_tensor(frames) else type(frames).__name__
        raise ValueError(f"input_video: {path!r} holds {what}, expected uint8 frames [T, H, W, 3]")
    return frames


def load_clip(config, lat_h: int, lat_w: int) -> Optional[torch.Tensor]:
    """The frames the yaml's `input_video` / `input_frames` keys select (host, uint8 [1 + 4k, H, W, 3]); None without the key.  The
    clip must already have the configured pixel size: nothing is resized."""
    path = config.get("input_video")
    if not path:
        return None
    if is_y4m_input(path):
        raise ValueError(f"input_video: {path!r} is a YUV4MPEG2 stream: it is not read on the host but converted on the device "
                         f"(load_clip_y4m, the route run() takes for a .y4m file or a FIFO)")
    frames = read_input_video(str(path))
    if tuple(frames.shape[1:3]) != (8 * lat_h, 8 * lat_w):
        raise ValueError(f"input_video: {path!r} is {frames.shape[2]}x{frames.shape[1]} (W x H), the configured size is "
                         f"{8 * lat_w}x{8 * lat_h}; clips are not resized")
    return frames[select_clip_frames(frames.shape[0], config.get("input_frames"))].contiguous()


def _fitted(frames: torch.Tensor, path: str, lat_h: int, lat_w: int, fit: Optional[str]):
    """Device frames [T, Hs, Ws, 3] at the configured size: (as they are, None) when it is theirs, (ops.resize_u8 of them, [Ws, Hs])
    when `input_fit` says how; refused otherwise."""
    from . import ops
    H, W = 8 * lat_h, 8 * lat_w
    Hs, Ws = int(frames.shape[1]), int(frames.shape[2])
    if (Hs, Ws) == (H, W):
        return frames, None
    if fit is None:
        raise ValueError(f"input_video: {path!r} is {Ws}x{Hs} (W x H), the configured size is {W}x{H}; "
                         f"set input_fit: cover | stretch to resize it")
    return ops.resize_u8(frames, (H, W), fit=fit), [Ws, Hs]


def load_clip_device(config, lat_h: int, lat_w: int, device):
    """load_clip with the yaml's `input_decode` / `input_fit` keys: (uint8 [1 + 4k, H, W, 3] ON THE DEVICE, [W, H] of the source when
    it was resized, else None).  `input_decode: gpu` takes an MJPEG .avi: select_clip_frames runs on the chunk count, so only the
    chosen files are parsed, uploaded and decoded (ops.jpeg_decode).  `input_fit` resizes a clip of another size on the device
    (ops.resize_u8); without it such a clip is refused as before."""
    from . import ops
    path = str(config.get("input_video"))
    decode, fit = input_decode(config.get("input_decode")), input_fit(config.get("input_fit"))
    if decode == "gpu":
        if os.path.splitext(path)[1].lower() != ".avi" or avi_compression(path) != b"MJPG":
            raise ValueError(f"input_decode: gpu reads a Motion-JPEG .avi, {path!r} is not one")
        files = read_avi_mjpeg_files(path)
        frames = ops.jpeg_decode(files[select_clip_frames(len(files), config.get("input_frames"))], device=device,
                                 split=input_split(config.get("input_split")))
    else:
        frames = read_input_video(path)
        frames = frames[select_clip_frames(frames.shape[0], config.get("input_frames"))].contiguous().to(device)
    return _fitted(frames, path, lat_h, lat_w, fit)


def load_clip_y4m(config, lat_h: int, lat_w: int, device):
    """The clip of a YUV4MPEG2 `input_video` (a .y4m file or a FIFO), converted on the device: (uint8 [1 + 4k, H, W, 3] ON THE DEVICE,
    [W, H] of the source when it was resized, else None, [num, den] of the header's rate when `input_rate: match` selected by it, else
    None).  The stream is read once, front to back, and only a ring of the frames the selection can touch is held; the selected
    payloads go up in one copy, their planes through ops.yuv_to_frames_u8 (any of the six layouts, `input_range` when the header
    names no range), then through ops.resize_u8 when `input_fit` is set and the size differs."""
    from . import ops, y4m
    path, cap = str(config.get("input_video")), input_frames(config.get("input_frames"))
    fit, how = input_fit(config.get("input_fit")), input_rate(config.get("input_rate"))
    with y4m.Y4MReader(path, input_range=input_range(config.get("input_range"))) as reader:
        rate = reader.rate() if how == "match" else None          # F0:0 is refused before a frame is read
        keep = None if cap is None else 1 + 4 * ((cap - 1) // 4)
        ring = reader.read_last(keep if rate is None or keep is None else y4m.frames_spanned(keep, rate, 16))
        total = reader.frames_read
        Hs, Ws, layout, rng = reader.height, reader.width, reader.layout, reader.range
    if rate is None:
        picked = list(range(total))[select_clip_frames(total, cap)]
    else:
        picked = y4m.select_frames_at_rate(total, rate, 16, cap)
    first = total - len(ring)
    host = torch.frombuffer(bytearray(b"".join(ring[i - first] for i in picked)), dtype=torch.uint8).view(len(picked), -1)
    buf = host.to(device)                                          # the one copy up
    hc, wc = ops.yuv_chroma_shape(layout, Hs, Ws)
    ybytes, cbytes = Hs * Ws, hc * wc
    y = buf[:, :ybytes].unflatten(1, (Hs, Ws))
    cb = cr = None
    if layout != "mono":
        cb = buf[:, ybytes:ybytes + cbytes].unflatten(1, (hc, wc))
        cr = buf[:, ybytes + cbytes:].unflatten(1, (hc, wc))
    frames = ops.yuv_to_frames_u8(y, cb, cr, layout=layout, range=rng)
    matched = None if rate is None else [rate.numerator, rate.denominator]
    return (*_fitted(frames, path, lat_h, lat_w, fit), matched)


class Clip(NamedTuple):
    """What `input_video` gave, in the terms of the three routes' docstrings (frames: on the host from load_clip, else on the device)."""
    frames: Optional[torch.Tensor]
    input_size: Optional[List[int]] = None
    matched_rate: Optional[List[int]] = None


def input_clip(config, lat_h: int, lat_w: int, device) -> Clip:
    """The clip to continue, by the route the yaml picks: a .y4m file or a FIFO is converted on the device, `input_decode` /
    `input_fit` decode / resize on the device, anything else is read on the host as before."""
    path = config.get("input_video")
    if path and is_y4m_input(path):                              # planes up in one copy, converted on the device
        return Clip(*load_clip_y4m(config, lat_h, lat_w, device))
    if path and (config.get("input_decode") is not None or config.get("input_fit") is not None):
        return Clip(*load_clip_device(config, lat_h, lat_w, device))
    return Clip(load_clip(config, lat_h, lat_w))


# ---- tokenizers --------------------------------------------------------------------------------------------------------
class HashTokenizer:
    """Stand-in for HuggingfaceTokenizer when no tokenizer files exist (synthetic mode): whitespace words -> crc32 ids,
    </s> = 1 appended, <pad> = 0, padded to seq_len.  Same call signature and return types (ids, mask int64)."""

    def __init__(self, vocab_size: int, seq_len: int = 512):
        self.vocab_size, self.seq_len = vocab_size, seq_len

    def __call__(self, texts: Sequence[str], return_mask: bool = True, add_special_tokens: bool = True):
        if isinstance(texts, str):
            texts = [texts]
        ids = torch.zeros(len(texts), self.seq_len, dtype=torch.long)
        mask = torch.zeros_like(ids)
        for b, t in enumerate(texts):
            toks = [2 + zlib.crc32(w.encode("utf-8")) % (self.vocab_size - 2) for w in " ".join(t.split()).split(" ") if w]
            toks = toks[: self.seq_len - 1] + [1]
            ids[b, :len(toks)] = torch.tensor(toks)
            mask[b, :len(toks)] = 1
        return (ids, mask) if return_mask else ids


def hf_tokenizer(path: str, seq_len: int = 512):
    """The reference's HuggingfaceTokenizer(name=path, seq_len=512, clean='whitespace') (wan/modules/tokenizers.py:38-82)
    restated over transformers.AutoTokenizer; ftfy.fix_text is applied when ftfy is installed."""
    import html
    import re
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(path)
    try:
        import ftfy
        fix = ftfy.fix_text
    except ImportError:
        fix = lambda s: s                                            # noqa: E731

    def clean(text):
        text = html.unescape(html.unescape(fix(text))).strip()
        return re.sub(r"\s+", " ", text).strip()

    def call(texts, return_mask=True, add_special_tokens=True):
        if isinstance(texts, str):
            texts = [texts]
        out = tok([clean(t) for t in texts], return_tensors="pt", padding="max_length", truncation=True,
                  max_length=seq_len, add_special_tokens=add_special_tokens)
        return (out.input_ids, out.attention_mask) if return_mask else out.input_ids

    return call


# ---- model construction --------------------------------------------------------------------------------------------------
def wan_config(config, synthetic: bool):
    """The generator's shape: LongLive-1.3B, in synthetic mode shrunk by `synthetic_overrides`."""
    from . import synth
    mk = config.model_kwargs
    ov = config.get("synthetic_overrides", Config()) if synthetic else Config()
    wkw = {k: ov.get(k) for k in ("num_layers", "lat_h", "lat_w") if ov.get(k) is not None}
    return synth.longlive_1_3b(local_attn_size=mk.local_attn_size, sink_size=mk.sink_size, **wkw)


def build_models(config, device, synthetic: bool):
    from . import synth
    from .checkpoint import load_generator
    from .text_encoder import WanTextEncoder
    from .vae import WanVAEWrapper
    from .wan_wrapper import WanDiffusionWrapper
    mk = config.model_kwargs
    ov = config.get("synthetic_overrides", Config()) if synthetic else Config()
    wcfg = wan_config(config, synthetic)
    lora_enabled = False
    if synthetic:
        tcfg = synth.T5Config(vocab_size=4096, num_layers=ov.get("t5_layers", 24))
        gen = WanDiffusionWrapper(timestep_shift=mk.timestep_shift, local_attn_size=mk.local_attn_size, sink_size=mk.sink_size,
                                  cfg=wcfg, device=device, state_dict=synth.synth_state_dict(wcfg, seed=0, device=device))
        vae = WanVAEWrapper(device=device)
        vsd = synth.synth_vae_state_dict(synth.VaeConfig(), seed=5, device=device)
        if config.get("input_video"):               # a clip to continue needs the encoder half too
            vsd.update(synth.synth_vae_encoder_state_dict(synth.VaeConfig(), seed=6, device=device))
        vae.load_state_dict(vsd)
        enc = WanTextEncoder(tcfg, device=device, tokenizer=HashTokenizer(tcfg.vocab_size, tcfg.text_len))
        enc.load_state_dict(synth.synth_t5_state_dict(tcfg, seed=7, device=device))
    else:
        root = config.get("wan_model_dir", "wan_models/Wan2.1-T2V-1.3B")
        gen = WanDiffusionWrapper(timestep_shift=mk.timestep_shift, local_attn_size=mk.local_attn_size, sink_size=mk.sink_size,
                                  cfg=wcfg, device=device)
        lora = config.get("lora_ckpt") if config.get("adapter") is not None else None
        load_generator(gen, config.generator_ckpt, lora_ckpt=lora, adapter=vars(config.adapter) if lora else None,
                       use_ema=config.get("use_ema", False))
        lora_enabled = lora is not None
        vae = WanVAEWrapper(device=device)
        vae.load_state_dict(torch.load(os.path.join(root, "Wan2.1_VAE.pth"), map_location="cpu"), strict=False)
        enc = WanTextEncoder(device=device, tokenizer=hf_tokenizer(os.path.join(root, "google/umt5-xxl/")))
        enc.load_state_dict(torch.load(os.path.join(root, "models_t5_umt5-xxl-enc-bf16.pth"), map_location="cpu"))
    return wcfg, gen, vae, enc, lora_enabled


QUANT_MODES = ("none", "int8", "mxfp8", "fp8_rowwise", "mxfp6", "mxfp4_a6", "mxfp4_a4")


def quant_mode(value) -> Optional[str]:
    """The yaml's `quant:` key (none | int8 | mxfp8 | fp8_rowwise | mxfp6 | mxfp4_a6 | mxfp4_a4, default none) as
    CausalWanModelHIP.set_quant's argument."""
    v = _one_of("quant", value, QUANT_MODES, "none")
    return None if v == "none" else v


ATTN_QUANT_MODES = ("none", "mxfp8")


def attn_quant_mode(value) -> Optional[str]:
    """The yaml's `attn_quant:` key (none | mxfp8, default none) as CausalWanModelHIP.set_attn_quant's argument."""
    v = _one_of("attn_quant", value, ATTN_QUANT_MODES, "none")
    return None if v == "none" else v


def _dist_env():
    if "LOCAL_RANK" in os.environ:
        lr = int(os.environ["LOCAL_RANK"])
        return lr, int(os.environ.get("RANK", str(lr))), int(os.environ.get("WORLD_SIZE", "1"))
    return 0, 0, 1


def run(mode: str, config, synthetic: bool = False, device: Optional[torch.device] = None) -> List[Dict]:
    """The body of inference.py (mode 'inference') / interactive_inference.py (mode 'interactive').  Returns one record per
    written video: {"path", "idx", "frames", "seconds"}, "input_frames" when the yaml's `input_video` gave a clip to continue,
    "input_size" ([W, H] of the clip) when `input_fit` resized it, "input_rate" ([num, den] of a .y4m clip's header) when
    `input_rate: match` selected by it, "codec" and "bytes" when `video_codec` chose one, "range" for `video_codec: y4m`, and "gif"
    (the path) and "gif_bytes" under `gif_preview: true`."""
    from .pipeline import CausalInferencePipeline, InteractiveCausalInferencePipeline
    local_rank, rank, world = _dist_env()
    if device is None:
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    torch.manual_seed(replica_seed(int(config.seed), local_rank))                 # set_seed(config.seed + local_rank)
    synthetic = synthetic or bool(config.get("synthetic", False))
    shape = wan_config(config, synthetic)
    codec = video_codec(config.get("video_codec"))             # names and ranges are refused before any model is built
    quality = jpeg_quality(config.get("jpeg_quality"))
    out_range = yuv_range(config.get("yuv_range"))
    input_range(config.get("input_range")), input_rate(config.get("input_rate"))
    input_decode(config.get("input_decode")), input_fit(config.get("input_fit")), input_split(config.get("input_split"))
    preview = gif_preview(config)
    clip = input_clip(config, shape.lat_h, shape.lat_w, device)    # read (decoded, resized) and checked before any model is built
    write = {None: _write_default, "mjpeg": functools.partial(_write_mjpeg, quality=quality),
             "y4m": functools.partial(_write_y4m, width=8 * shape.lat_w, height=8 * shape.lat_h, out_range=out_range),
             "png": _write_png, "apng": _write_apng}[codec]
    wcfg, gen, vae, enc, lora_enabled = build_models(config, device, synthetic)
    gen.model.set_quant(quant_mode(config.get("quant", "none")))       # block linears: bf16, W8A8, MXFP8, FP8 rowwise, MXFP6, W4A6 or W4A4
    gen.model.set_attn_quant(attn_quant_mode(config.get("attn_quant", "none")))   # self-attention: bf16 or MXFP8
    interactive = mode == "interactive"
    cls = InteractiveCausalInferencePipeline if interactive else CausalInferencePipeline
    pipeline = cls(config, device, generator=gen, text_encoder=enc, vae=vae)
    pipeline.overlap_decode = bool(config.get("overlap_decode", True))     # blocks are decoded while the next ones are generated (same video)
    if interactive:
        switch = parse_switch_frame_indices(config.switch_frame_indices)
        dataset = MultiTextDataset(config.data_path)
        nseg = len(dataset[0]["prompts_list"])
        assert len(switch) == nseg - 1, "The number of switch_frame_indices should be the number of prompt segments minus 1"
    else:
        dataset = TextDataset(prompt_path=config.data_path, extended_prompt_path=config.data_path)
    # every rank creates the folder: the CLI builds no process group, so there is no barrier to order a rank-0-only
    # makedirs before the other ranks' first write (the reference has dist.barrier() there, inference.py:153-156)
    os.makedirs(config.output_folder, exist_ok=True)
    model_type = model_type_of(config, lora_enabled)
    extra, more = {}, {}
    if clip.frames is not None:                     # every prompt continues the same clip: encoded once
        latent = vae.encode_frames_to_latent(clip.frames.unsqueeze(0).to(device))
        more["initial_latent"] = latent.expand(config.num_samples, *latent.shape[1:])
        extra["input_frames"] = int(clip.frames.shape[0])
        if clip.input_size is not None:
            extra["input_size"] = clip.input_size
        if clip.matched_rate is not None:
            extra["input_rate"] = clip.matched_rate
    if codec == "y4m":                              # the decoder's last kernel writes I420: the bytes of the file's payloads
        more["frames"], more["yuv_range"] = "yuv420", out_range
    elif codec is not None:                         # the pipeline hands back uint8 frames: no fp32 planes, no torch conversion
        more["frames"] = "uint8"
    records = []
    for i, idx in enumerate(rank_indices(len(dataset), rank, world)):
        item = dataset[idx]
        noise = torch.randn([config.num_samples, config.num_output_frames, 16, wcfg.lat_h, wcfg.lat_w], device=device,
                            dtype=torch.bfloat16)
        t0 = time.perf_counter()
        if interactive:
            prompts_list = [[p] * config.num_samples for p in item["prompts_list"]]
            video = pipeline.inference(noise=noise, text_prompts_list=prompts_list, switch_frame_indices=switch,
                                       return_latents=False, profile=config.get("profile", False), **more)
            first_prompt = item["prompts_list"][0]
        else:
            prompt = item.get("extended_prompts") or item["prompts"]
            video, _ = pipeline.inference(noise=noise, text_prompts=[prompt] * config.num_samples, return_latents=True,
                                          profile=config.get("profile", False), **more)
            first_prompt = item["prompts"]
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
        if codec is None:
            video = (255.0 * video.permute(0, 1, 3, 4, 2)).to(torch.uint8).cpu()        # b t c h w -> b t h w c
        vae.model.clear_cache()
        for seed_idx in range(config.num_samples):
            name = output_name(rank, idx, seed_idx, model_type, config.save_with_index, first_prompt, interactive)
            path, count, coded = write(os.path.join(config.output_folder, name), video[seed_idx])
            if preview is not None:
                rgb = _preview_frames(video[seed_idx], codec, 8 * shape.lat_w, 8 * shape.lat_h, out_range, device)
                coded = {**coded, **_write_gif_preview(os.path.join(config.output_folder, name), rgb, preview)}
            records.append({"path": path, "idx": idx, "frames": count, "seconds": dt, **coded, **extra})
        if config.inference_iter != -1 and i >= config.inference_iter:
            break
    return records


def main(argv=None):
    ap = argparse.ArgumentParser(prog="longlive_amd.cli")
    ap.add_argument("mode", choices=["inference", "interactive"])
    ap.add_argument("--config_path", type=str, required=True, help="Path to the config file")
    ap.add_argument("--synthetic", action="store_true", help="random-init weights + hash tokenizer (no checkpoints)")
    args = ap.parse_args(argv)
    recs = run(args.mode, load_config(args.config_path), synthetic=args.synthetic)
    for r in recs:
        print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
