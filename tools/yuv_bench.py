"""MEASUREMENT ONLY.  Planar YUV ("Planar YUV and Y4M") at 480x832 on one device, synthetic weights.
usage: python tools/yuv_bench.py [--out profiles/yuv_frames.json] [--reps 7] [--skip-stream]
Prints one JSON line (also written to --out) with
  cl_to_yuv420    us per frame of ll_cl_to_yuv420 on one decoder chunk of 12 frames against the only other route to the same bytes:
                  ll_cl_to_frames_u8 followed by a torch-op chain that restates the integer arithmetic on the device (checked equal
                  first); the candidates are ALTERNATED inside every repetition and each figure is the median over the repetitions
  frames_u8_to_yuv420, yuv_to_frames_u8 (420jpeg and 420mpeg2)    us per frame, likewise
  tbps            each kernel's achieved bytes/s over the bytes its algorithm must move (input read once + output written once),
                  beside ll_cl_to_frames_u8's measured in the same run
  stream_video    pixel frames/s of CausalInferencePipeline.stream_video with overlap_decode at bench.py's e2e_live configuration for
                  frames = uint8 and yuv420, ALTERNATED
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
    args = ap.parse_args(argv)

    import torch
    import bench
    from longlive_amd import ops, synth

    dev = torch.device("cuda", 0)
    H, W, N = 480, 832, 12

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

    tel = bench.Telemetry(0)
    tel.start()
    rec = {"device": torch.cuda.get_device_name(0), "frames": f"{N} x {H}x{W}", "reps": args.reps, "launches_per_window": args.inner}

    x = (torch.randn(N, H, W, 8, device=dev, generator=torch.Generator(dev).manual_seed(1)) * 0.7).to(torch.bfloat16)   # a head output
    u8 = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    nbytes = ops.yuv420_bytes(H, W)
    i420 = torch.empty(N, nbytes, dtype=torch.uint8, device=dev)
    back = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)

    def torch_chain():
        """ll_cl_to_frames_u8, then limited-range I420 in int32 torch ops (the rules of csrc/yuv.h; H and W are even here)."""
        v = ops.cl_to_frames_u8(x, out=u8).to(torch.int32)
        y = 16 + ((16829 * v[..., 0] + 33039 * v[..., 1] + 6416 * v[..., 2] + 32768) >> 16)
        s = v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]
        cb = (128 + ((-9714 * s[..., 0] - 19071 * s[..., 1] + 28785 * s[..., 2] + 131072) >> 18)).clamp(16, 240)
        cr = (128 + ((28784 * s[..., 0] - 24103 * s[..., 1] - 4681 * s[..., 2] + 131072) >> 18)).clamp(16, 240)
        return torch.cat([y.clamp(16, 235).reshape(N, -1), cb.reshape(N, -1), cr.reshape(N, -1)], 1).to(torch.uint8)

    assert torch.equal(torch_chain(), ops.cl_to_yuv420(x, out=i420))
    assert torch.equal(ops.frames_u8_to_yuv420(u8), i420)
    y, cb, cr = ops.yuv420_planes(i420, H, W)
    med, span = alternate({
        "cl_to_yuv420": lambda: ops.cl_to_yuv420(x, out=i420),
        "cl_to_frames_u8_plus_torch": torch_chain,
        "cl_to_frames_u8": lambda: ops.cl_to_frames_u8(x, out=u8),
        "frames_u8_to_yuv420": lambda: ops.frames_u8_to_yuv420(u8, out=i420),
        "yuv_to_frames_u8_420jpeg": lambda: ops.yuv_to_frames_u8(y, cb, cr, "420jpeg", out=back),
        "yuv_to_frames_u8_420mpeg2": lambda: ops.yuv_to_frames_u8(y, cb, cr, "420mpeg2", out=back)})
    moved = {"cl_to_yuv420": x.numel() * 2 + i420.numel(), "cl_to_frames_u8": x.numel() * 2 + u8.numel(),
             "frames_u8_to_yuv420": u8.numel() + i420.numel(), "yuv_to_frames_u8_420jpeg": i420.numel() + back.numel(),
             "yuv_to_frames_u8_420mpeg2": i420.numel() + back.numel()}
    rec["kernels"] = {"us_per_frame": {k: v / N for k, v in med.items()},
                      "min_max_us_per_frame": {k: [a / N, b / N] for k, (a, b) in span.items()},
                      "bytes_moved": moved, "tbps": {k: moved[k] / med[k] / 1e6 for k in moved}}

    if not args.skip_stream:
        from longlive_amd.pipeline import CausalInferencePipeline
        from longlive_amd.vae import WanVAEWrapper
        from longlive_amd.wan_wrapper import WanDiffusionWrapper
        vcfg = synth.VaeConfig()
        vae = WanVAEWrapper(vcfg, device=dev, chunk=3)
        vae.load_state_dict(synth.synth_vae_state_dict(vcfg, seed=5, device=dev))
        cfg = synth.longlive_1_3b(local_attn_size=12, sink_size=3)
        gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=12, sink_size=3, cfg=cfg, device=dev,
                                  state_dict=synth.synth_state_dict(cfg, seed=0, device=dev))
        prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=dev)}
        P = CausalInferencePipeline(bench._pipe_args(), dev, generator=gen, text_encoder=lambda text_prompts: prompt, vae=vae)
        nb = 11
        noise = synth.synth_noise(cfg, 3 * nb, seed=0, device=dev)

        def run(frames):
            times = []
            for _, px in P.stream_video(noise, ["p0"], overlap_decode=True, frames=frames):
                px.view(-1)[-1].item()                           # wait for THIS block's frames only
                times.append(time.perf_counter())
            torch.cuda.synchronize()
            steady = [(b - a) * 1e3 for a, b in zip(times[5:-1], times[6:])]
            return 12e3 * len(steady) / sum(steady)

        fps = {f: [] for f in ("uint8", "yuv420")}
        for _ in range(2):
            for f in fps:
                fps[f].append(run(f))
        rec["stream_video"] = dict({f: {"fps": max(v), "passes": v} for f, v in fps.items()},
                                   what="overlap_decode; pixel frames/s over the last 5 block intervals of 11; best of 2 alternated passes")

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
