"""Launch-count driver for MXFP8 self-attention, meant to run under a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/mx_attn_trace.py

Two steady-state forwards of the 30-layer LongLive-1.3B (random init, cache full: every forward rolls the window and inserts 3 frames)
in none+attn mode (bf16 linears, set_attn_quant("mxfp8")).  The first forward allocates each layer's shadow and re-derives all of it
(one kv_shadow_mx_kernel launch per layer, covering the roll and the insert); the second refreshes the rolled window and the inserted
tokens as one merged range per layer.  Expected: 60 flash_attn_mx_kernel, 60 kv_shadow_mx_kernel, no flash_attn_asm_kernel (the
self-attention kernel of bf16 mode; cross-attention keeps flash_attn_asm_qn_kernel).

--quant / --attn-quant pick other modes for the same two forwards, e.g. the FP8 rowwise trace:

    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/mx_attn_trace.py --quant fp8_rowwise --attn-quant none

and the MXFP6 trace: --quant mxfp6 --attn-quant none; the W4A6 trace: --quant mxfp4_a6
--attn-quant none; the W4A4 trace: --quant mxfp4_a4 --attn-quant none."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quant", default="none", help="block linears: none | int8 | mxfp8 | fp8_rowwise | mxfp6 | mxfp4_a6 | mxfp4_a4")
    ap.add_argument("--attn-quant", default="mxfp8", help="self-attention: none | mxfp8")
    args = ap.parse_args(argv)
    import torch
    from longlive_amd import synth
    from longlive_amd.wan_wrapper import WanDiffusionWrapper
    dev = torch.device("cuda", 0)
    cfg = synth.longlive_1_3b()
    gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=12, sink_size=3, cfg=cfg, device=dev,
                              state_dict=synth.synth_state_dict(cfg, seed=0, device=dev))
    fs, S = cfg.frame_seqlen, 12 * cfg.frame_seqlen
    for mod in gen.model.modules():
        if hasattr(mod, "max_attention_size"):
            mod.max_attention_size = S
    gen.model.set_quant(None if args.quant == "none" else args.quant)
    gen.model.set_attn_quant(None if args.attn_quant == "none" else args.attn_quant)
    bf = torch.bfloat16
    kv = []
    for i in range(cfg.num_layers):
        k = synth.hash_normal(61, f"kv.{i}.k", (1, S, cfg.num_heads, cfg.head_dim), device=dev).to(bf)
        v = (0.5 * synth.hash_normal(61, f"kv.{i}.v", (1, S, cfg.num_heads, cfg.head_dim), device=dev)).to(bf)
        kv.append(dict(k=k, v=v, global_end_index=S, local_end_index=S))
    ca = [dict(k=torch.zeros(1, cfg.text_len, cfg.num_heads, 128, dtype=bf, device=dev),
               v=torch.zeros(1, cfg.text_len, cfg.num_heads, 128, dtype=bf, device=dev), is_init=False) for _ in range(cfg.num_layers)]
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=dev)}
    noise = synth.synth_noise(cfg, 6, seed=0, device=dev)
    for f in range(2):
        gen(noise[:, 3 * f: 3 * f + 3], prompt, torch.full((1, 3), 625.0, device=dev), kv_cache=kv, crossattn_cache=ca,
            current_start=S + 3 * f * fs)
    torch.cuda.synchronize()
    print(f"mx_attn_trace: 2 forwards done (quant {args.quant}, attn_quant {args.attn_quant})")


if __name__ == "__main__":
    main()
