"""MEASUREMENT ONLY.  Frames out ("Frames out") at 480x832 on one device, synthetic weights.
usage: python tools/frames_out_bench.py [--out profiles/frames_out.json] [--reps 7] [--skip-stream]
Prints one JSON line (also written to --out) with
  to_u8           us per frame of ll_cl_to_frames_u8 against ll_cl_to_tchw_clamp + the torch chain it replaces
                  (`(v * 0.5 + 0.5).clamp(0, 1)`, `(255.0 * v.permute(...)).to(uint8)`) on one decoder chunk of 12 frames; the two are
                  ALTERNATED inside every repetition and each figure is the median over the repetitions
  jpeg            us per frame of ll_jpeg_encode_u8 at quality 90 on 12 decoded synthetic frames and on 12 frames of uniform noise, the
                  share of its first stage (ll_jpeg_coefficients_u8 alone; the three entropy launches are the rest), mean file size.
                  Per-kernel times come from a kernel trace of this script run with --only-jpeg (profiles/frames_out.md)
  stream_video    pixel frames/s of CausalInferencePipeline.stream_video at bench.py's e2e_live configuration (LongLive-1.3B, VAE chunk 3,
                  11 blocks, the last 5 intervals timed) with frames = float / uint8 / jpeg, serial and overlap_decode, the three ALTERNATED
and the card's average clock and power over the run (bench.Telemetry)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed window")
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--only-jpeg", action="store_true", help="a few encodes and nothing else (for a kernel trace)")
    args = ap.parse_args(argv)

    import torch
    import bench
    from longlive_amd import ops, synth
    from longlive_amd.vae import WanVAEWrapper

    dev = torch.device("cuda", 0)
    H, W, N = 480, 832, 12
    vcfg = synth.VaeConfig()
    vae = WanVAEWrapper(vcfg, device=dev, chunk=3)
    vae.load_state_dict(synth.synth_vae_state_dict(vcfg, seed=5, device=dev))
    lat = synth.hash_normal(55, "frames_out.latent", (1, 4, 16, H // 8, W // 8)).to(torch.bfloat16).to(dev)
    decoded = vae.decode_to_frames(lat, use_cache=False)[0, 1:1 + N].contiguous()           # 12 of the 13 frames
    noise_frames = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(3))
    torch.cuda.synchronize()

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / args.inner                                        # us per call

    def alternate(fns):
        """{name: median us per call}: every repetition times each candidate once, in turn."""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        got = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                got[k].append(window(fn))
        return {k: statistics.median(v) for k, v in got.items()}, {k: [min(v), max(v)] for k, v in got.items()}

    if args.only_jpeg:
        for _ in range(5):
            ops.jpeg_encode(decoded, 90)
            ops.jpeg_encode(noise_frames, 90)
        torch.cuda.synchronize()
        return

    tel = bench.Telemetry(0)
    tel.start()
    rec = {"device": torch.cuda.get_device_name(0), "frames": f"{N} x {H}x{W}", "reps": args.reps, "launches_per_window": args.inner}

    x = (torch.randn(N, H, W, 8, device=dev, generator=torch.Generator(dev).manual_seed(1)) * 0.7).to(torch.bfloat16)   # a head output
    out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)

    def torch_chain():
        v = ops.cl_to_tchw_clamp(x)
        v = (v * 0.5 + 0.5).clamp(0, 1)
        return (255.0 * v[None].permute(0, 1, 3, 4, 2)).to(torch.uint8)

    assert torch.equal(torch_chain()[0], ops.cl_to_frames_u8(x, out=out))
    med, span = alternate({"kernel": lambda: ops.cl_to_frames_u8(x, out=out), "tchw_clamp_plus_torch": torch_chain,
                           "tchw_clamp_alone": lambda: ops.cl_to_tchw_clamp(x)})
    rec["to_u8"] = {"us_per_frame": {k: v / N for k, v in med.items()}, "min_max_us_per_frame": {k: [a / N, b / N] for k, (a, b) in span.items()},
                    "gbps_kernel": (x.numel() * 2 + out.numel()) / med["kernel"] / 1e3}

    rec["jpeg"] = {}
    for name, frames in (("decoded", decoded), ("noise", noise_frames)):
        stride_t = 3 * H * W
        out_stride, scratch_bytes = ops.jpeg_sizes(N, H, W)
        buf = torch.empty(N, out_stride, dtype=torch.uint8, device=dev)
        sizes = torch.empty(N, dtype=torch.int32, device=dev)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        coef = torch.empty(N, 30, 52, 6, 64, dtype=torch.int16, device=dev)
        lib, st = ops._lib.load(), ops._stream()
        med, span = alternate({
            "encode": lambda: lib.ll_jpeg_encode_u8(frames.data_ptr(), stride_t, N, H, W, 90, buf.data_ptr(), out_stride, sizes.data_ptr(),
                                                    scratch.data_ptr(), scratch_bytes, st),
            "coefficients": lambda: lib.ll_jpeg_coefficients_u8(frames.data_ptr(), stride_t, N, H, W, 90, coef.data_ptr(), st)})
        rec["jpeg"][name] = {"quality": 90, "us_per_frame": {k: v / N for k, v in med.items()},
                             "min_max_us_per_frame": {k: [a / N, b / N] for k, (a, b) in span.items()},
                             "entropy_us_per_frame": (med["encode"] - med["coefficients"]) / N,
                             "mean_file_bytes": float(sizes.float().mean()), "raw_frame_bytes": stride_t,
                             "scratch_mib": scratch_bytes / 2 ** 20, "out_stride": out_stride}

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

        def run(frames, overlap):
            times = []
            for _, px in P.stream_video(noise, ["p0"], overlap_decode=overlap, frames=frames):
                if frames == "jpeg":
                    pass                                         # the files are on the host: this block is done
                elif overlap:
                    px.view(-1)[-1].item()                       # wait for THIS block's frames only
                else:
                    torch.cuda.synchronize()
                times.append(time.perf_counter())
            torch.cuda.synchronize()
            steady = [(b - a) * 1e3 for a, b in zip(times[5:-1], times[6:])]
            return 12e3 * len(steady) / sum(steady)

        res = {}
        for overlap in (False, True):
            key = "overlap_decode" if overlap else "serial"
            fps = {f: [] for f in ("float", "uint8", "jpeg")}
            for _ in range(2):
                for f in fps:
                    fps[f].append(run(f, overlap))
            res[key] = {f: {"fps": max(v), "passes": v} for f, v in fps.items()}
        rec["stream_video"] = dict(res, what="pixel frames/s over the last 5 block intervals of 11; best of 2 alternated passes, both listed")

    t = tel.stop(0)
    rec["telemetry"] = {k: t.get(k) for k in ("sclk_mhz_avg", "sclk_mhz_min", "power_w_avg", "power_w_max", "power_cap_w", "samples", "source")}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
