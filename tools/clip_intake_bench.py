#!/usr/bin/env python3
"""Clip intake on the GPU, measured: decode time per frame of ops.jpeg_decode for a clip of this project's own files (one restart
interval per MCU row: 30 lanes per 480 x 832 frame) and for Pillow-made files of the same frames without restart markers (one lane per
frame), the entropy launch and the two pixel launches separately (device events around ll_jpeg_decode_coefficients and
ll_jpeg_decode_pixels), the resize of 1080p frames to 480p, and Pillow's host decode of the same files on the same machine.  The
entropy stage is also measured as an A/B ("entropy_ab"): the serial route against the split route (subsequences of a segment side by
side) at 128 / 256 / 512 / 1024 bytes and at 64 and 1 lanes per wave, alternating in one loop, with the share of segments per `info`
value and the highest settle round.

    python tools/clip_intake_bench.py [--frames 81] [--reps 5] [--out profiles/clip_intake.json]

Prints one JSON line.  Clock and power over the timed regions come from bench.py's Telemetry (hwmon, side thread).  Nothing here has
a parent value, so nothing gates; profiles/clip_intake.md holds what was measured.  For the share of each kernel inside the pixel
stage run it under `rocprofv3 --kernel-trace --stats -- python tools/clip_intake_bench.py --reps 1`."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import Telemetry                          # noqa: E402
from longlive_amd import _lib, jpeg_files, ops       # noqa: E402


def footage(T: int, H: int, W: int, device) -> torch.Tensor:
    """uint8 [T, H, W, 3]: moving colour gradients plus mild noise, what decoded video looks like to a JPEG coder."""
    g = torch.Generator(device=device).manual_seed(0)
    y = torch.arange(H, dtype=torch.float32, device=device).view(1, H, 1)
    x = torch.arange(W, dtype=torch.float32, device=device).view(1, 1, W)
    t = torch.arange(T, dtype=torch.float32, device=device).view(T, 1, 1)
    base = torch.stack([128 + 100 * torch.sin(x / 37.0 + t / 5.0) + 0 * y, 128 + 100 * torch.cos(y / 29.0 - t / 7.0) + 0 * x,
                        60 + 0.2 * x + 0.25 * y + t], -1)
    return (base + 6.0 * torch.randn(T, H, W, 3, generator=g, device=device)).clamp(0, 255).to(torch.uint8)


def timed(fn, reps: int):
    """Median milliseconds of fn() by device events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def decode_figures(files, reps: int, device) -> dict:
    T = len(files)
    t0 = time.perf_counter()
    pk, d = ops._jpeg_upload(files, device)
    torch.cuda.synchronize()
    host_ms = 1e3 * (time.perf_counter() - t0)
    H, W = pk.height, pk.width
    coef_bytes, scratch_bytes = ops.jpeg_decode_sizes(T, H, W, pk.components, pk.hs, pk.vs)
    coef = torch.empty(coef_bytes // 2, dtype=torch.int16, device=device)
    planes = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
    status = torch.empty(pk.segs.shape[0], dtype=torch.int32, device=device)
    out = torch.empty(T, H, W, 3, dtype=torch.uint8, device=device)
    lib, s = _lib.load(), ops._stream()
    geo = (T, H, W, pk.components, pk.hs, pk.vs)

    def entropy():
        _lib.check(lib.ll_jpeg_decode_coefficients(d["data"].data_ptr(), pk.data.nbytes, d["segs"].data_ptr(), pk.segs.shape[0],
                                                   d["huff"].data_ptr(), d["sel"].data_ptr(), *geo, coef.data_ptr(), status.data_ptr(), s),
                   "ll_jpeg_decode_coefficients")

    def pixels():
        _lib.check(lib.ll_jpeg_decode_pixels(coef.data_ptr(), d["qt"].data_ptr(), *geo, out.data_ptr(), 3 * H * W, planes.data_ptr(),
                                             scratch_bytes, s), "ll_jpeg_decode_pixels")

    e = timed(entropy, reps)
    p = timed(pixels, reps)
    assert int(status.abs().max()) == 0, "a segment failed"
    t0 = time.perf_counter()
    whole = ops.jpeg_decode(files, device=device)
    torch.cuda.synchronize()
    call_ms = 1e3 * (time.perf_counter() - t0)
    assert torch.equal(whole, out)
    return {"frames": T, "bytes_per_frame": sum(len(f) for f in files) // T, "segments": int(pk.segs.shape[0]),
            "entropy_ms_per_frame": e[0] / T, "entropy_ms_min_max": [e[1] / T, e[2] / T],
            "pixels_ms_per_frame": p[0] / T, "pixels_ms_min_max": [p[1] / T, p[2] / T],
            "kernels_ms_per_frame": (e[0] + p[0]) / T, "parse_pack_upload_ms_per_frame": host_ms / T,
            "jpeg_decode_call_ms_per_frame": call_ms / T}, out


SPLIT_SIZES = (128, 256, 512, 1024)
SPLIT_LANES = (64, 1)


def event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def split_figures(files, reps: int, rounds: int, device) -> dict:
    """The entropy stage alone, A/B in one loop on one device: per repetition the serial route (the parent's, one lane per restart
    segment), then the split route at every subsequence size and lane count per wave, each timed by device events; medians over the
    repetitions.  Per size also the share of segments per `info` value and the highest settle round."""
    T = len(files)
    pk, d = ops._jpeg_upload(files, device)
    geo = (T, pk.height, pk.width, pk.components, pk.hs, pk.vs)
    nseg = pk.segs.shape[0]
    coef_bytes = ops.jpeg_decode_sizes(*geo)[0]
    ref = torch.empty(coef_bytes // 2, dtype=torch.int16, device=device)
    coef = torch.empty_like(ref)
    status = torch.empty(nseg, dtype=torch.int32, device=device)
    info = torch.empty(nseg, dtype=torch.int32, device=device)
    lib, s = _lib.load(), ops._stream()
    head = (d["data"].data_ptr(), pk.data.nbytes, d["segs"].data_ptr(), nseg, d["huff"].data_ptr(), d["sel"].data_ptr(), *geo)

    def serial():
        _lib.check(lib.ll_jpeg_decode_coefficients(*head, ref.data_ptr(), status.data_ptr(), s), "ll_jpeg_decode_coefficients")

    tables, empty = {}, []
    for sub in SPLIT_SIZES:
        rows = jpeg_files.split_segments(pk, sub)
        if rows.shape[0] == 0:                             # no segment reaches 4 * sub bytes: the call is the serial route's
            empty.append(sub)
        else:
            work_bytes = ops.jpeg_decode_sizes(*geo, split=(nseg, rows.shape[0]), rounds=rounds)[2]
            tables[sub] = (torch.from_numpy(rows).to(device), rows.shape[0], torch.empty(work_bytes, dtype=torch.uint8, device=device))

    def split(sub, lanes):
        subs, nsub, work = tables[sub]
        _lib.check(lib.ll_set_tuning(b"jpeg_split_lanes", lanes), "ll_set_tuning")
        _lib.check(lib.ll_jpeg_decode_coefficients_split(*head, coef.data_ptr(), status.data_ptr(), subs.data_ptr(), nsub, rounds,
                                                         info.data_ptr(), work.data_ptr(), work.numel(), s),
                   "ll_jpeg_decode_coefficients_split")

    res = {"frames": T, "segments": nseg, "rounds": rounds, "bytes_per_frame": sum(len(f) for f in files) // T,
           "longest_segment_bytes": int(pk.segs[:, 1].max()), "sizes_without_rows": empty, "split": {}}
    serial()
    torch.cuda.synchronize()
    for sub in tables:
        shares = None
        for lanes in SPLIT_LANES:
            coef.fill_(0x7FFF)
            split(sub, lanes)
            torch.cuda.synchronize()
            assert torch.equal(coef, ref) and int(status.abs().max()) == 0, (sub, lanes)
            host = info.cpu()
            shares = {"serial_by_table": float((host == 0).float().mean()), "settled": float((host >= 1).float().mean()),
                      "unsettled": float((host == -1).float().mean()), "flagged": float((host == -2).float().mean()),
                      "highest_settle_round": int(host.max())}
        res["split"][str(sub)] = {"subsequences": tables[sub][1], **shares}
    times = {"serial": []}
    for _ in range(reps):
        times["serial"].append(event_ms(serial))
        for sub in tables:
            for lanes in SPLIT_LANES:
                times.setdefault((sub, lanes), []).append(event_ms(lambda: split(sub, lanes)))
    _lib.check(lib.ll_set_tuning(b"jpeg_split_lanes", 0), "ll_set_tuning")
    res["serial_entropy_ms_per_frame"] = statistics.median(times["serial"]) / T
    for sub in tables:
        for lanes in SPLIT_LANES:
            ms = statistics.median(times[(sub, lanes)]) / T
            res["split"][str(sub)][f"entropy_ms_per_frame_lanes{lanes}"] = ms
            res["split"][str(sub)][f"serial_over_split_lanes{lanes}"] = res["serial_entropy_ms_per_frame"] / ms
    return res


def pil_decode_ms(files) -> float:
    from PIL import Image
    import numpy as np
    t0 = time.perf_counter()
    for f in files:
        np.array(Image.open(io.BytesIO(f)).convert("RGB"), dtype=np.uint8)
    return 1e3 * (time.perf_counter() - t0) / len(files)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--rounds", type=str, default=str(ops.JPEG_SPLIT_ROUNDS), help="rounds of the split route's A/B, comma-separated")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("clip_intake_bench needs a GPU: nothing here is measured on the CPU")
    device = torch.device("cuda", 0)
    T, H, W = args.frames, 480, 832
    res = {"device": torch.cuda.get_device_name(0), "frames": T, "size": [W, H], "quality": args.quality, "reps": args.reps}
    frames = footage(T, H, W, device)
    own = ops.jpeg_bytes(*ops.jpeg_encode(frames, args.quality))
    tel = Telemetry(0)
    tel.start()
    res["own_files"], dec = decode_figures(own, args.reps, device)
    rounds = [int(r) for r in args.rounds.split(",")]
    res["entropy_ab"] = {"own_files": {str(r): split_figures(own, args.reps, r, device) for r in rounds}}
    try:
        from PIL import Image
        import numpy as np
        host = frames.cpu().numpy()
        pil = []
        for t in range(T):
            b = io.BytesIO()
            Image.fromarray(host[t]).save(b, "JPEG", quality=args.quality, subsampling=2)
            pil.append(b.getvalue())
        res["pillow_files"], dec_pil = decode_figures(pil, args.reps, device)
        res["entropy_ab"]["pillow_files"] = {str(r): split_figures(pil, args.reps, r, device) for r in rounds}
        res["pillow_host_decode_ms_per_frame"] = {"own_files": pil_decode_ms(own), "pillow_files": pil_decode_ms(pil)}
        ref = torch.from_numpy(np.stack([np.array(Image.open(io.BytesIO(f)).convert("RGB")) for f in pil[:4]]))
        res["pillow_files"]["max_abs_difference_from_pillows_decoder"] = int((dec_pil[:4].cpu().int() - ref.int()).abs().max())
    except ImportError:
        res["pillow_files"] = res["pillow_host_decode_ms_per_frame"] = None
    del frames
    big = footage(T, 1080, 1920, device)
    out = torch.empty(T, H, W, 3, dtype=torch.uint8, device=device)
    r = timed(lambda: ops.resize_u8(big, (H, W), fit="cover", out=out), args.reps)
    res["resize_1080p_to_480p"] = {"ms_per_frame": r[0] / T, "ms_min_max": [r[1] / T, r[2] / T], "window": list(ops.cover_window(1080, 1920, H, W)),
                                   "taps": [int(ops.resize_taps(1080, H)[1].max()), int(ops.resize_taps(1872, W)[1].max())]}
    res["telemetry"] = tel.stop(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
