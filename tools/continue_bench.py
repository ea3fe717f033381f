"""MEASUREMENT ONLY.  Continuing an 81-frame 480x832 clip ("Continuing a clip"): synthetic LongLive-1.3B weights
and a synthetic VAE, one device.   usage: python tools/continue_bench.py [--out profiles/continue_bench.json] [--reps 3]
Prints one JSON line (also written to --out) with
  intake          ll_pixels_u8_to_cl on the encoder's 4-frame step (Cpad 32): us per launch, us per frame, GB/s read + written
  encode_ms       encode_frames_to_latent of the 81 frames (1 + 20 steps of 4) -> 21 latent frames
  prefill_ms      the 7 kv_only forwards over those 21 latents (last_profile's "prefill" phase)
  first_block_ms  host time from the call of `stream(..., initial_latent=)` until the device has finished the first GENERATED block (its
                  own context pass, queued right behind it, included), from latents and, with the encode in front, from frames
and the card's average clock and power over the run (bench.Telemetry), as the other records of profiles/ state them."""
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
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)

    import torch
    import bench
    from longlive_amd import ops, synth
    from longlive_amd.pipeline import CausalInferencePipeline
    from longlive_amd.vae import WanVAEWrapper
    from longlive_amd.wan_wrapper import WanDiffusionWrapper

    dev = torch.device("cuda", 0)
    T, H, W, NEW = 81, 480, 832, 3
    cfg = synth.longlive_1_3b(local_attn_size=12, sink_size=3)
    gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=12, sink_size=3, cfg=cfg, device=dev,
                              state_dict=synth.synth_state_dict(cfg, seed=0, device=dev))
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=dev)}
    vcfg = synth.VaeConfig()
    vae = WanVAEWrapper(vcfg, device=dev)
    sd = dict(synth.synth_vae_state_dict(vcfg, seed=5, device=dev))
    sd.update(synth.synth_vae_encoder_state_dict(vcfg, seed=6, device=dev))
    vae.load_state_dict(sd)
    clip = torch.randint(0, 256, (1, T, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(3))
    noise = synth.synth_noise(cfg, NEW, seed=0, device=dev)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def median(fn):
        fn()                                                 # warm-up: packing, code objects, memos
        torch.cuda.synchronize()
        return statistics.median(events(fn)[0] for _ in range(args.reps))

    tel = bench.Telemetry(0)
    tel.start()
    rec = {"device": torch.cuda.get_device_name(0), "clip": f"{T} frames {H}x{W} uint8", "latent_frames": 1 + (T - 1) // 4, "reps": args.reps}

    cpad = vae._get_encoder().cpad
    dst = torch.empty(4, H, W, cpad, dtype=torch.bfloat16, device=dev)
    us = 1e3 * median(lambda: ops.pixels_u8_to_cl(clip[0, 1:5], cpad, out=dst))
    rec["intake"] = dict(cpad=cpad, us_per_4_frames=us, us_per_frame=us / 4,
                         gbps=(4 * H * W * 3 + dst.numel() * 2) / us / 1e3)
    rec["encode_ms"] = median(lambda: vae.encode_frames_to_latent(clip))
    latent = vae.encode_frames_to_latent(clip)

    pipe = CausalInferencePipeline(bench._pipe_args(), dev, generator=gen)

    def prefill():
        pipe.inference(noise, prompt, initial_latent=latent, profile=True)
        return pipe.last_profile["times_ms"]["prefill"]

    prefill()
    rec["prefill_ms"] = statistics.median(prefill() for _ in range(args.reps))
    rec["prefill_forwards"] = len(pipe._prefix_blocks(latent.shape[1]))

    def first_block(from_frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat = vae.encode_frames_to_latent(clip) if from_frames else latent
        for start, _ in pipe.stream(noise, prompt, initial_latent=lat):
            if start >= lat.shape[1]:
                break
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    rec["first_block_ms"] = {"from_latents": statistics.median(first_block(False) for _ in range(args.reps)),
                             "from_frames": statistics.median(first_block(True) for _ in range(args.reps))}
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
