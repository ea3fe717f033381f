"""MEASUREMENT ONLY.  Animated previews ("Animated previews: GIF") on one device, synthetic weights.
usage: python tools/gif_bench.py [--out profiles/gif_frames.json] [--reps 5] [--skip-stream]
Prints one JSON line (also written to --out) with
  gif             us per frame of ll_gif_encode_u8 (palette clip, dither bayer) on T = 12 (one block's frames) and T = 81 decoded synthetic
                  frames at 480x832 and at 240x416 (the same frames through ops.resize_u8), of its quantiser alone (ll_gif_quantize_u8)
                  and of its coder alone (ll_gif_lzw_u8 over the quantiser's indices), with ll_png_encode_u8 on the same frames, all
                  ALTERNATED inside every repetition; each figure is the median over the repetitions, a repetition being a window of
                  --window-ms (300) of launches between two device events; mean file sizes
  kernels         us per launch of every gif kernel from a kernel trace (torch.profiler) of three T = 12 encodes at 480x832
  pillow          ms per frame of Pillow on this host for 3 of the same 480x832 frames: `save` of our indices under our palette, and
                  quantize(256, MEDIANCUT) + `save`; its file sizes and ours; PSNR of both against the frames
  stream_video    pixel frames/s of CausalInferencePipeline.stream_video at bench.py's e2e_live configuration with frames = uint8, and
                  with every yielded block encoded by gif.encode and read to the host, overlap_decode, one pass each, ALTERNATED; the
                  difference per block of 12 frames."""
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
    ap.add_argument("--inner", type=int, default=5, help="launches per timed window at least")
    ap.add_argument("--window-ms", type=float, default=300.0, help="a timed window is filled to this length")
    ap.add_argument("--skip-stream", action="store_true")
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    import bench
    from longlive_amd import gif, ops, synth
    from longlive_amd.vae import WanVAEWrapper

    dev = torch.device("cuda", 0)
    H, W = 480, 832
    vcfg = synth.VaeConfig()
    vae = WanVAEWrapper(vcfg, device=dev, chunk=3)
    vae.load_state_dict(synth.synth_vae_state_dict(vcfg, seed=5, device=dev))
    lat = synth.hash_normal(55, "frames_out.latent", (1, 21, 16, H // 8, W // 8)).to(torch.bfloat16).to(dev)
    decoded81 = vae.decode_to_frames(lat, use_cache=False)[0].contiguous()                  # 81 frames
    half81 = ops.resize_u8(decoded81, (H // 2, W // 2), fit="stretch")
    torch.cuda.synchronize()
    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "launches_per_window_min": args.inner, "window_ms": args.window_ms, "palette": "clip",
           "dither": "bayer"}
    lib, st = gif.bind(), ops._stream()

    def window(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / inner                                             # us per call

    def alternate(fns):
        """Medians and spans over --reps windows per candidate, the candidates alternated.  A window holds as many launches as fill
        --window-ms (at least --inner), sized from a first window after the warm-up: a short candidate is not timed over a few ms."""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        inner = {k: max(args.inner, int(1e3 * args.window_ms / max(window(fn, args.inner), 1.0)) + 1) for k, fn in fns.items()}
        got = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                got[k].append(window(fn, inner[k]))
        return {k: statistics.median(v) for k, v in got.items()}, {k: [min(v), max(v)] for k, v in got.items()}, inner

    rec["gif"] = {}
    for name, frames in (("480x832_T12", decoded81[1:13].contiguous()), ("480x832_T81", decoded81),
                         ("240x416_T12", half81[1:13].contiguous()), ("240x416_T81", half81)):
        T, h, w, _ = (int(v) for v in frames.shape)
        stride_t, n = 3 * h * w, h * w
        out_stride, scratch_bytes = gif.sizes(T, h, w, "clip")
        buf = torch.empty(T, out_stride, dtype=torch.uint8, device=dev)
        sizes = torch.empty(T, dtype=torch.int32, device=dev)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        idx, pal, used = gif.quantize(frames, "clip", "bayer")
        qidx, qpal, qused = torch.empty_like(idx), torch.empty_like(pal), torch.empty_like(used)
        z_stride, z_scratch = gif.lzw_sizes(T, n)
        zbuf = torch.empty(T, z_stride, dtype=torch.uint8, device=dev)
        zsizes = torch.empty(T, dtype=torch.int32, device=dev)
        zscr = torch.empty(z_scratch, dtype=torch.uint8, device=dev)
        p_stride, p_scratch = ops.png_sizes(T, h, w)
        pbuf = torch.empty(T, p_stride, dtype=torch.uint8, device=dev)
        psizes = torch.empty(T, dtype=torch.int32, device=dev)
        pscr = torch.empty(p_scratch, dtype=torch.uint8, device=dev)
        med, span, inner = alternate({
            "gif_encode": lambda: lib.ll_gif_encode_u8(frames.data_ptr(), stride_t, T, h, w, 0, 1, buf.data_ptr(), out_stride,
                                                       sizes.data_ptr(), scratch.data_ptr(), scratch_bytes, st),
            "quantize": lambda: lib.ll_gif_quantize_u8(frames.data_ptr(), stride_t, T, h, w, 0, 1, qidx.data_ptr(), qpal.data_ptr(),
                                                       qused.data_ptr(), scratch.data_ptr(), scratch_bytes, st),
            "lzw": lambda: lib.ll_gif_lzw_u8(idx.data_ptr(), n, T, n, zbuf.data_ptr(), z_stride, zsizes.data_ptr(), zscr.data_ptr(),
                                             z_scratch, st),
            "png_encode": lambda: lib.ll_png_encode_u8(frames.data_ptr(), stride_t, T, h, w, pbuf.data_ptr(), p_stride, psizes.data_ptr(),
                                                       pscr.data_ptr(), p_scratch, st)})
        torch.cuda.synchronize()
        rec["gif"][name] = {"frames": T, "us_per_frame": {k: v / T for k, v in med.items()},
                            "min_max_us_per_frame": {k: [a / T, b / T] for k, (a, b) in span.items()}, "launches_per_window": inner,
                            "mean_gif_bytes": float(sizes.float().mean()), "mean_png_bytes": float(psizes.float().mean()),
                            "used_entries": int(used[0]), "raw_frame_bytes": stride_t, "scratch_mib": scratch_bytes / 2 ** 20,
                            "out_stride": out_stride}

    try:
        from torch.profiler import ProfilerActivity, profile
        frames = decoded81[1:13].contiguous()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                gif.encode(frames)
            torch.cuda.synchronize()
        rec["kernels"] = {e.key: {"launches": e.count, "us_per_launch": getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)) / e.count}
                          for e in prof.key_averages() if "gif" in e.key}
    except Exception as exc:                                      # the trace is a convenience: the figures above stand without it
        rec["kernels"] = {"error": repr(exc)}

    from PIL import Image

    def psnr(a, b):
        mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
        return float("inf") if mse == 0 else 10 * float(np.log10(255.0 ** 2 / mse))

    three = decoded81[1:4].contiguous()
    host = three.cpu().numpy()
    ours = gif.files(*gif.encode(three))
    idx, pal, _ = (t.cpu().numpy() for t in gif.quantize(three, "clip", "bayer"))
    idx0, pal0, _ = (t.cpu().numpy() for t in gif.quantize(three, "clip", "none"))
    pil = {"save_our_indices": [], "quantize_mediancut_and_save": []}
    pil_bytes, pil_psnr = {"save_our_indices": [], "quantize_mediancut_and_save": []}, []
    for t in range(3):
        with Image.open(io.BytesIO(ours[t])) as im:
            assert np.array_equal(np.asarray(im.convert("RGB")), pal[0][idx[t]])
        b = io.BytesIO()
        t0 = time.perf_counter()
        im = Image.fromarray(idx[t], "P")
        im.putpalette(pal[0].tobytes())
        im.save(b, "GIF", optimize=False)
        pil["save_our_indices"].append(1e3 * (time.perf_counter() - t0))
        pil_bytes["save_our_indices"].append(len(b.getvalue()))
        b = io.BytesIO()
        t0 = time.perf_counter()
        q = Image.fromarray(host[t]).quantize(256, method=Image.Quantize.MEDIANCUT)
        q.save(b, "GIF")
        pil["quantize_mediancut_and_save"].append(1e3 * (time.perf_counter() - t0))
        pil_bytes["quantize_mediancut_and_save"].append(len(b.getvalue()))
        q0 = Image.fromarray(host[t]).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE)
        pil_psnr.append(psnr(np.asarray(q0.convert("RGB")), host[t]))
    rec["pillow"] = {"ms_per_frame": pil, "bytes": pil_bytes, "our_bytes": [len(f) for f in ours],
                     "ours_over_save_our_indices": [len(f) / p for f, p in zip(ours, pil_bytes["save_our_indices"])],
                     "psnr_undithered_db": {"ours_clip_palette_of_3": [psnr(pal0[0][idx0[t]], host[t]) for t in range(3)],
                                            "pillow_mediancut_per_frame": pil_psnr}}

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

        def run(mode):
            times = []
            for _, px in P.stream_video(noise, ["p0"], overlap_decode=True, frames="uint8"):
                if mode == "uint8":
                    px.view(-1)[-1].item()                       # wait for THIS block's frames only
                else:
                    gif.files(*gif.encode(px[0]))                # encoded on the caller's stream, one host read
                times.append(time.perf_counter())
            torch.cuda.synchronize()
            steady = [(b - a) * 1e3 for a, b in zip(times[5:-1], times[6:])]
            return 12e3 * len(steady) / sum(steady), sum(steady) / len(steady)

        run("uint8")                                             # warm-up
        res = {m: run(m) for m in ("uint8", "uint8+gif")}
        rec["stream_video"] = {m: fps for m, (fps, _) in res.items()}
        rec["stream_video"]["ms_per_block"] = {m: ms for m, (_, ms) in res.items()}
        rec["stream_video"]["gif_ms_per_block_added"] = res["uint8+gif"][1] - res["uint8"][1]
        rec["stream_video"]["what"] = "pixel frames/s over the last 5 block intervals of 11, overlap_decode, one pass each after a warm-up pass"

    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
