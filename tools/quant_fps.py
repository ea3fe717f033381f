"""Frames/s of the block-linear precisions (none = bf16, int8 = W8A8, mxfp8 = MXFP8, fp8_rowwise = e4m3 with per-token / per-channel
scales, mxfp6 = MXFP6 E2M3, mxfp4_a6 = E2M1 weights over MXFP6 activations,
mxfp4_a4 = E2M1 weights and activations), each with bf16 self-attention or with MXFP8
self-attention over the shadow of the KV cache ("+attn": set_attn_quant("mxfp8")), alternated in one process.

Workload = bench.py's fps_of: the LongLive-1.3B random-init generator, config 2's steady state (4 warm-up blocks, then timed blocks
through pipe.stream).  The modes run in turn for --rounds rounds, so a clock drift of the device lands on all of them alike; the
record holds the median frames/s, ms per block and average GPU clock per mode, and per-kernel tables of one extra (timed-launch)
block of mxfp8, fp8_rowwise, mxfp6, mxfp4_a6, mxfp4_a4 and none+attn (those among --modes), with the MX / FP8 / MXFP6 / W4A6 /
W4A4 GEMM and MX attention plan strings.  With both mxfp6 and mxfp4_a6 among --modes, the record also compares each GEMM shape's
launch in the two (median over --rounds timed blocks of each, alternated); likewise mxfp4_a4 against mxfp4_a6.

    python tools/quant_fps.py --rounds 3 --blocks 4 --out profiles/quant_fps.json
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

MODES = ("none", "int8", "mxfp8", "fp8_rowwise", "mxfp6", "mxfp4_a6", "mxfp4_a4", "none+attn", "int8+attn", "mxfp8+attn", "fp8_rowwise+attn",
         "mxfp6+attn", "mxfp4_a6+attn", "mxfp4_a4+attn")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset of " + ", ".join(MODES))
    args = ap.parse_args(argv)

    import torch
    import bench
    from longlive_amd import _lib, ops, synth
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

    def run(mode, blocks, timer=None):
        lin, _, attn = mode.partition("+")
        gen.model.set_quant(None if lin == "none" else lin)
        gen.model.set_attn_quant("mxfp8" if attn == "attn" else None)
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
        clk = tel.stop(0).get("sclk_mhz_avg")
        return dict(fps=12 * blocks / dt, ms_per_block=1e3 * dt / blocks, sclk_mhz=clk)

    rows = {m: [] for m in modes}
    for r in range(args.rounds):
        for m in modes:
            rows[m].append(run(m, args.blocks))
            print(f"round {r} {m:10s}: {rows[m][-1]['fps']:.2f} frames/s, {rows[m][-1]['ms_per_block']:.1f} ms/block, "
                  f"sclk {rows[m][-1]['sclk_mhz']}", flush=True)
    med = {}
    for m in modes:
        clks = [x["sclk_mhz"] for x in rows[m] if x["sclk_mhz"] is not None]
        med[m] = dict(fps=statistics.median(x["fps"] for x in rows[m]), ms_per_block=statistics.median(x["ms_per_block"] for x in rows[m]),
                      sclk_mhz=statistics.median(clks) if clks else None)

    def kernel_table(mode):
        timer = ops.KernelTimer()
        run(mode, 1, timer)
        torch.cuda.synchronize()
        summ = timer.summary()
        return {t: dict(launches=v["launches"], avg_us=1e3 * v["avg_ms"], total_ms=v["total_ms"])
                for t, v in sorted(summ.items(), key=lambda kv: -kv[1]["total_ms"])}

    tables = {m: kernel_table(m) for m in ("mxfp8", "fp8_rowwise", "mxfp6", "mxfp4_a6", "mxfp4_a4", "none+attn") if m in modes}

    def gemm_launch_vs(new, old):
        """Each GEMM shape's launch time in `new` against `old` (median over --rounds timed blocks of each, alternated)."""
        per = {new: [], old: []}
        for _ in range(args.rounds):
            for m in per:
                per[m].append(kernel_table(m))
        vs = {}
        for t in ("gemm_f1", "gemm_f2", "gemm_qkv", "gemm_o", "gemm_co", "gemm_cq"):
            if not all(t in tb for m in per for tb in per[m]):
                continue
            us = {m: statistics.median(tb[t]["avg_us"] for tb in per[m]) for m in per}
            vs[t] = {f"{new}_us": us[new], f"{old}_us": us[old], "ratio": us[new] / us[old]}
        return vs

    gemm_vs = gemm_launch_vs("mxfp4_a6", "mxfp6") if "mxfp6" in modes and "mxfp4_a6" in modes else None
    gemm_vs4 = gemm_launch_vs("mxfp4_a4", "mxfp4_a6") if "mxfp4_a6" in modes and "mxfp4_a4" in modes else None
    M = 3 * cfg.frame_seqlen
    S = cfg.local_attn_size * cfg.frame_seqlen
    shapes = (("gemm_qkv", 3 * cfg.dim, cfg.dim), ("gemm_o / gemm_cq / gemm_co", cfg.dim, cfg.dim), ("gemm_f1", cfg.ffn_dim, cfg.dim),
              ("gemm_f2", cfg.dim, cfg.ffn_dim))
    plans = {name: ops.gemm_plan_mx(M, n, k) for name, n, k in shapes}
    plans_f8 = {name: ops.gemm_plan_f8(M, n, k) for name, n, k in shapes}
    plans_mx6 = {name: ops.gemm_plan_mx6(M, n, k) for name, n, k in shapes}
    plans_mx4 = {name: ops.gemm_plan_mx4w6(M, n, k) for name, n, k in shapes}
    plans_mx4a4 = {name: ops.gemm_plan_mx4(M, n, k) for name, n, k in shapes}
    sink = cfg.sink_size * cfg.frame_seqlen
    attn_plan = ops.flash_attn_mx_plan(M, cfg.num_heads, 1, [(0, sink), (sink, S)])
    gen.model.set_quant(None)
    gen.model.set_attn_quant(None)
    rec = dict(tool="tools/quant_fps.py", device=torch.cuda.get_device_name(0), rounds=args.rounds, blocks=args.blocks,
               workload="bench.py fps_of: LongLive-1.3B random-init, config 2 steady state, 4 warm-up blocks, timed blocks via pipe.stream",
               median=med, runs=rows, mxfp8_gemm_plans=plans, fp8_rowwise_gemm_plans=plans_f8, mxfp6_gemm_plans=plans_mx6,
               mxfp4_a6_gemm_plans=plans_mx4, mxfp4_a4_gemm_plans=plans_mx4a4, flash_attn_mx_plan=attn_plan)
    if gemm_vs is not None:
        rec["mxfp4_a6_vs_mxfp6_gemm_launch_us"] = gemm_vs
    if gemm_vs4 is not None:
        rec["mxfp4_a4_vs_mxfp4_a6_gemm_launch_us"] = gemm_vs4
    for m, kern in tables.items():
        rec[m.replace("+", "_") + "_kernels_one_block"] = kern
    print(json.dumps(dict(median=med)), flush=True)
    for m, kern in tables.items():
        print(f"per-kernel, one timed block of {m}:")
        for t, v in kern.items():
            print(f"  {t:28s} {v['launches']:5d} launches  {v['avg_us']:9.1f} us avg  {v['total_ms']:8.2f} ms")
    if "fp8_rowwise" in tables:
        for name, p in plans_f8.items():
            print(f"fp8_rowwise {name}: {p}")
    if "mxfp6" in tables:
        for name, p in plans_mx6.items():
            print(f"mxfp6 {name}: {p}")
    if "mxfp4_a6" in tables:
        for name, p in plans_mx4.items():
            print(f"mxfp4_a6 {name}: {p}")
    if gemm_vs is not None:
        for t, v in gemm_vs.items():
            print(f"  {t:9s} mxfp4_a6 {v['mxfp4_a6_us']:7.1f} us vs mxfp6 {v['mxfp6_us']:7.1f} us ({v['ratio']:.3f})")
    if "mxfp4_a4" in tables:
        for name, p in plans_mx4a4.items():
            print(f"mxfp4_a4 {name}: {p}")
    if gemm_vs4 is not None:
        for t, v in gemm_vs4.items():
            print(f"  {t:9s} mxfp4_a4 {v['mxfp4_a4_us']:7.1f} us vs mxfp4_a6 {v['mxfp4_a6_us']:7.1f} us ({v['ratio']:.3f})")
    if "none+attn" in tables:
        print(f"flash_attn_mx: {attn_plan}")
        for t in ("flash_attn_self_mx", "kv_shadow_mx"):
            v = tables["none+attn"].get(t)
            if v:
                print(f"  {t}: {v['launches']} launches, {v['avg_us']:.1f} us avg, {v['total_ms']:.2f} ms per block (lone-stream launches)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
