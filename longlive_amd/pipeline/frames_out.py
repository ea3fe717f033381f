"""The form frames are delivered in ("Frames out"): one value, built once from the public keywords `frames`,
`jpeg_quality` and `yuv_range` of stream_video / inference, that answers every question the delivery path asks about them.  A new
delivery format is one more mode here (and one more writer in cli.py)."""
from __future__ import annotations

from dataclasses import dataclass

from .. import ops

FRAME_MODES = ("float", "uint8", "jpeg", "yuv420")


def check_jpeg_quality(value) -> int:
    """The 1..100 rule of every `jpeg_quality` (the keyword here, the yaml key in cli.py)."""
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= 100:
        raise ValueError(f"jpeg_quality: {value!r} must be an integer 1..100")
    return int(value)


@dataclass(frozen=True)
class FramesOut:
    """Construction is the validation, refused before any launch: `jpeg_quality` is read by "jpeg" alone, `yuv_range` by "yuv420"
    alone."""
    mode: str = "float"
    jpeg_quality: int = 90
    yuv_range: str = "limited"

    def __post_init__(self):
        if self.mode not in FRAME_MODES:
            raise ValueError(f"frames: {self.mode!r} is not one of {', '.join(FRAME_MODES)}")
        if self.mode == "jpeg":
            check_jpeg_quality(self.jpeg_quality)
        if self.mode == "yuv420" and self.yuv_range not in ops.YUV_RANGES:
            raise ValueError(f"yuv_range: {self.yuv_range!r} is not one of {', '.join(ops.YUV_RANGES)}")

    @property
    def decoder_form(self) -> str:
        """What the VAE decoder writes for this mode: JPEG files are encoded from its uint8 frames."""
        return "uint8" if self.mode == "jpeg" else self.mode

    def decode(self, vae, latents, use_cache: bool):
        """One decode in the decoder form, queued on the current stream: pixels in [0, 1], uint8 frames or I420 frames."""
        form = self.decoder_form
        if form == "float":
            video = vae.decode_to_pixel(latents, use_cache=use_cache)
            return (video * 0.5 + 0.5).clamp(0, 1)
        if form == "yuv420":
            return vae.decode_to_frames(latents, use_cache=use_cache, frames="yuv420", yuv_range=self.yuv_range)
        return vae.decode_to_frames(latents, use_cache=use_cache)

    def encode(self, payload):
        """"jpeg": uint8 [B, T', H, W, 3] -> [(buf, sizes) per batch item] of ops.jpeg_encode, on the current stream; else `payload`."""
        if self.mode != "jpeg":
            return payload
        return [ops.jpeg_encode(v, self.jpeg_quality) for v in payload]

    def deliver(self, payload):
        """What the caller gets: tensors as they are, JPEG pairs as [[bytes per frame] per batch item] (the one host read)."""
        if self.mode != "jpeg":
            return payload
        return [ops.jpeg_bytes(buf, sizes) for buf, sizes in payload]

    def record_stream(self, payload, stream) -> None:
        """An encoded payload, made on another stream, is about to be read on `stream`."""
        for t in ([t for pair in payload for t in pair] if self.mode == "jpeg" else [payload]):
            t.record_stream(stream)
