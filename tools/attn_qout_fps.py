"""What the attention kernels' quantised output (model.fuse_attn_quant) is worth in the block-scaled modes: frames/s with the fusion on
and off, alternated in one process on one device (tools/quant_fps.py's method: bench.py's steady-state workload, 4 warm-up blocks,
then timed blocks through pipe.stream), medians over --rounds rounds with the device's clock and board power beside each figure; and
from one timed-launch block of each, the median launch time of the fused self- and cross-attention against the bf16 attention launch
plus its quantiser launch.

    python tools/attn_qout_fps.py --rounds 3 --blocks 3 --out profiles/attn_qout_fps.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("mxfp8", "mxfp6", "mxfp4_a6", "mxfp4_a4", "mxfp4_a4+attn")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", default=",".join(MODES[:4]), help="comma-separated subset of " + ", ".join(MODES))
    args = ap.parse_args(argv)

    import torch
    import bench
    from longlive_amd import _lib, model, ops, synth
    from longlive_amd.pipeline import CausalInferencePipeline
    from longlive_amd.wan_wrapper import WanDiffusionWrapper

    _lib.load()
    dev = torch.device("cuda", 0)
    cfg = synth.longlive_1_3b(local_attn_size=12, sink_size=3)
    gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=12, sink_size=3, cfg=cfg, device=dev,
                              state_dict=synth.synth_state_dict(cfg, seed=0, device=dev))
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=dev)}
    modes = [m.strip() for m in args.modes.split(",") if m.strip()]
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode {m!r}: one of {', '.join(MODES)}")
    default_on = gen.model.fuse_attn_quant

    def run(mode, fuse, blocks, timer=None):
        lin, _, attn = mode.partition("+")
        gen.model.set_quant(lin)
        gen.model.set_attn_quant("mxfp8" if attn == "attn" else None)
        gen.model.fuse_attn_quant = fuse
        pipe = CausalInferencePipeline(bench._pipe_args(), dev, generator=gen)
        st = pipe.stream(synth.synth_noise(cfg, 3 * (4 + blocks), seed=0, device=dev), prompt)
        for _ in range(4):
            next(st)
        torch.cuda.synchronize()
        tel = bench.Telemetry(0)
        tel.start()
        ops.timer = timer
        t0 = time.perf_counter()
        for _ in range(blocks):
            next(st)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ops.timer = None
        t = tel.stop(0)
        return dict(fps=12 * blocks / dt, ms_per_block=1e3 * dt / blocks, sclk_mhz=t.get("sclk_mhz_avg"), power_w=t.get("power_w_avg"))

    keys = [(m, f) for m in modes for f in (True, False)]
    rows = {k: [] for k in keys}
    for r in range(args.rounds):
        for k in keys:
            rows[k].append(run(*k, args.blocks))
            x = rows[k][-1]
            print(f"round {r} {k[0]:14s} {'fused  ' if k[1] else 'unfused'}: {x['fps']:.2f} frames/s, {x['ms_per_block']:.1f} ms/block, "
                  f"sclk {x['sclk_mhz']}, {x['power_w']} W", flush=True)

    def med(xs):
        xs = [x for x in xs if x is not None]
        return statistics.median(xs) if xs else None

    name = lambda k: f"{k[0]}/{'fused' if k[1] else 'unfused'}"      # noqa: E731
    median = {name(k): {f: med([x[f] for x in rows[k]]) for f in ("fps", "ms_per_block", "sclk_mhz", "power_w")} for k in keys}

    def launches(mode, fuse):
        """tag -> (launches, median us) of one timed-launch block"""
        timer = ops.KernelTimer()
        run(mode, fuse, 1, timer)
        torch.cuda.synchronize()
        return {t: (len(recs), 1e3 * statistics.median(a.elapsed_time(b) for a, b, _ in recs)) for t, recs in timer.records.items()}

    per_launch = {}
    for m in modes:
        on, off = launches(m, True), launches(m, False)
        qtag = [t for t in off if t.startswith("quantize")]
        assert not [t for t in on if t.startswith("quantize")], on.keys()
        rec = {"quantiser": {t: dict(launches=off[t][0], median_us=off[t][1]) for t in qtag}}
        q_us = off[qtag[0]][1] if qtag else None
        for t in sorted(t for t in on if t.startswith("flash_attn") and t in off):
            rec[t] = dict(launches=on[t][0], fused_us=on[t][1], bf16_us=off[t][1], bf16_plus_quantiser_us=None if q_us is None else off[t][1] + q_us)
        per_launch[m] = rec
    gen.model.set_quant(None)
    gen.model.set_attn_quant(None)
    gen.model.fuse_attn_quant = default_on
    M, S, sink = 3 * cfg.frame_seqlen, cfg.local_attn_size * cfg.frame_seqlen, cfg.sink_size * cfg.frame_seqlen
    plans = {m: dict(self_attention=ops.flash_attn_q_plan(model._QUANT_MODES[m.partition("+")[0]].afmt, M, cfg.num_heads, 1, [(0, sink), (sink, S)]),
                     cross_attention=ops.flash_attn_q_plan(model._QUANT_MODES[m.partition("+")[0]].afmt, M, cfg.num_heads, 1, [(0, cfg.text_len)]))
             for m in modes}
    verdict = {m: median[name((m, True))]["ms_per_block"] <= median[name((m, False))]["ms_per_block"] for m in modes}
    rec = dict(tool="tools/attn_qout_fps.py", device=torch.cuda.get_device_name(0), rounds=args.rounds, blocks=args.blocks,
               workload="bench.py fps_of: LongLive-1.3B random-init, config 2 steady state, 4 warm-up blocks, timed blocks via pipe.stream; "
                        "fuse_attn_quant on / off alternated in one process",
               median=median, fused_no_slower=verdict, per_launch_one_block=per_launch, plans=plans,
               runs={name(k): v for k, v in rows.items()})
    print(json.dumps(dict(median=median, fused_no_slower=verdict, per_launch=per_launch), indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
