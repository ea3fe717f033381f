"""MEASUREMENT ONLY.  Lossless frames out ("Lossless frames: PNG") at 480x832 on one device, synthetic weights.
usage: python tools/png_bench.py [--out profiles/png_frames.json] [--reps 5] [--skip-stream]
Prints one JSON line (also written to --out) with
  png             us per frame of ll_png_encode_u8 on T = 12 (one block's frames) and T = 81 decoded synthetic frames and on 12 frames of
                  uniform noise (the stored fallback), of its filter stage alone (ll_png_filter_u8) and of the compressor alone
                  (ll_zlib_compress_u8 over the filtered rows), with ll_jpeg_encode_u8 at quality 90 on the same frames ALTERNATED
                  inside every repetition; each figure is the median over the repetitions; mean file sizes
  kernels         us per launch of every png / zlib kernel from a kernel trace (torch.profiler) of three T = 12 encodes
  pillow          ms per frame of Pillow's PNG writer on this host at its default level and at compress_level=1 on 3 of the same
                  frames, its default file size, and our size against it
  stream_video    pixel frames/s of CausalInferencePipeline.stream_video at bench.py's e2e_live configuration with frames = uint8, jpeg,
                  and uint8 with every yielded block encoded by ops.png_encode and read to the host (what the CLI's writers do with a
                  whole video), overlap_decode, one pass each, ALTERNATED."""
import argparse
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="launches per timed window")
    ap.add_argument("--skip-stream", action="store_true")
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    import bench
    from longlive_amd import ops, synth
    from longlive_amd.vae import WanVAEWrapper

    dev = torch.device("cuda", 0)
    H, W = 480, 832
    vcfg = synth.VaeConfig()
    vae = WanVAEWrapper(vcfg, device=dev, chunk=3)
    vae.load_state_dict(synth.synth_vae_state_dict(vcfg, seed=5, device=dev))
    lat = synth.hash_normal(55, "frames_out.latent", (1, 21, 16, H // 8, W // 8)).to(torch.bfloat16).to(dev)
    decoded81 = vae.decode_to_frames(lat, use_cache=False)[0].contiguous()                  # 81 frames
    noise12 = torch.randint(0, 256, (12, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(3))
    torch.cuda.synchronize()
    rec = {"device": torch.cuda.get_device_name(0), "frame": f"{H}x{W}", "reps": args.reps, "launches_per_window": args.inner}
    lib, st = ops._lib.load(), ops._stream()

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / args.inner                                        # us per call

    def alternate(fns):
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        got = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                got[k].append(window(fn))
        return {k: statistics.median(v) for k, v in got.items()}, {k: [min(v), max(v)] for k, v in got.items()}

    rec["png"] = {}
    for name, frames in (("decoded_T12", decoded81[1:13].contiguous()), ("decoded_T81", decoded81), ("noise_T12", noise12)):
        T = int(frames.shape[0])
        stride_t, n = 3 * H * W, H * (1 + 3 * W)
        out_stride, scratch_bytes = ops.png_sizes(T, H, W)
        buf = torch.empty(T, out_stride, dtype=torch.uint8, device=dev)
        sizes = torch.empty(T, dtype=torch.int32, device=dev)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        filtered = ops.png_filter(frames).view(T, n)
        z_stride, z_scratch = ops.zlib_sizes(T, n)
        zbuf = torch.empty(T, z_stride, dtype=torch.uint8, device=dev)
        zscr = torch.empty(z_scratch, dtype=torch.uint8, device=dev)
        j_stride, j_scratch = ops.jpeg_sizes(T, H, W)
        jbuf = torch.empty(T, j_stride, dtype=torch.uint8, device=dev)
        jsizes = torch.empty(T, dtype=torch.int32, device=dev)
        jscr = torch.empty(j_scratch, dtype=torch.uint8, device=dev)
        fout = torch.empty(T, n, dtype=torch.uint8, device=dev)
        med, span = alternate({
            "png_encode": lambda: lib.ll_png_encode_u8(frames.data_ptr(), stride_t, T, H, W, buf.data_ptr(), out_stride, sizes.data_ptr(),
                                                       scratch.data_ptr(), scratch_bytes, st),
            "filter": lambda: lib.ll_png_filter_u8(frames.data_ptr(), stride_t, T, H, W, fout.data_ptr(), st),
            "compress": lambda: lib.ll_zlib_compress_u8(filtered.data_ptr(), n, T, n, zbuf.data_ptr(), z_stride, sizes.data_ptr(),
                                                        zscr.data_ptr(), z_scratch, st),
            "jpeg_encode_q90": lambda: lib.ll_jpeg_encode_u8(frames.data_ptr(), stride_t, T, H, W, 90, jbuf.data_ptr(), j_stride,
                                                             jsizes.data_ptr(), jscr.data_ptr(), j_scratch, st)})
        lib.ll_png_encode_u8(frames.data_ptr(), stride_t, T, H, W, buf.data_ptr(), out_stride, sizes.data_ptr(), scratch.data_ptr(),
                             scratch_bytes, st)
        torch.cuda.synchronize()
        rec["png"][name] = {"frames": T, "us_per_frame": {k: v / T for k, v in med.items()},
                            "min_max_us_per_frame": {k: [a / T, b / T] for k, (a, b) in span.items()},
                            "mean_png_bytes": float(sizes.float().mean()), "mean_jpeg_bytes": float(jsizes.float().mean()),
                            "raw_frame_bytes": stride_t, "scratch_mib": scratch_bytes / 2 ** 20, "out_stride": out_stride}

    try:
        from torch.profiler import ProfilerActivity, profile
        frames = decoded81[1:13].contiguous()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                ops.png_encode(frames)
            torch.cuda.synchronize()
        rec["kernels"] = {e.key: {"launches": e.count, "us_per_launch": getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)) / e.count}
                          for e in prof.key_averages() if "png" in e.key or "zlib" in e.key}
    except Exception as exc:                                      # the trace is a convenience: the figures above stand without it
        rec["kernels"] = {"error": repr(exc)}

    from PIL import Image
    host = decoded81[1:4].cpu().numpy()
    ours = ops.png_bytes(*ops.png_encode(decoded81[1:4].contiguous()))
    pil = {"default": [], "compress_level_1": []}
    pil_bytes = []
    for t in range(3):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(ours[t])).convert("RGB")), host[t])
        for key, kw in (("default", {}), ("compress_level_1", {"compress_level": 1})):
            b = io.BytesIO()
            t0 = time.perf_counter()
            Image.fromarray(host[t]).save(b, "PNG", **kw)
            pil[key].append(1e3 * (time.perf_counter() - t0))
            if key == "default":
                pil_bytes.append(len(b.getvalue()))
    rec["pillow"] = {"ms_per_frame": pil, "default_bytes": pil_bytes, "our_bytes": [len(f) for f in ours],
                     "ours_over_default": [len(f) / p for f, p in zip(ours, pil_bytes)]}

    if not args.skip_stream:
        from longlive_amd.pipeline import CausalInferencePipeline
        from longlive_amd.wan_wrapper import WanDiffusionWrapper
        cfg = synth.longlive_1_3b(local_attn_size=12, sink_size=3)
        gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=12, sink_size=3, cfg=cfg, device=dev,
                                  state_dict=synth.synth_state_dict(cfg, seed=0, device=dev))
        prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=dev)}
        P = CausalInferencePipeline(bench._pipe_args(), dev, generator=gen, text_encoder=lambda text_prompts: prompt, vae=vae)
        nb = 11
        noise = synth.synth_noise(cfg, 3 * nb, seed=0, device=dev)

        def run(frames):
            times = []
            for _, px in P.stream_video(noise, ["p0"], overlap_decode=True, frames="uint8" if frames == "uint8+png" else frames):
                if frames == "uint8":
                    px.view(-1)[-1].item()                       # wait for THIS block's frames only; jpeg files are on the host already
                elif frames == "uint8+png":
                    ops.png_bytes(*ops.png_encode(px[0]))        # encoded on the caller's stream, one host read
                times.append(time.perf_counter())
            torch.cuda.synchronize()
            steady = [(b - a) * 1e3 for a, b in zip(times[5:-1], times[6:])]
            return 12e3 * len(steady) / sum(steady)

        run("uint8")                                             # warm-up
        rec["stream_video"] = {f: run(f) for f in ("uint8", "jpeg", "uint8+png")}
        rec["stream_video"]["what"] = "pixel frames/s over the last 5 block intervals of 11, overlap_decode, one pass each after a warm-up pass"

    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
