"""Writes tests/golden/vae_encode.pt: the reference's WanVAEWrapper.encode_to_latent -> WanVAE_.encode (utils/wan_wrapper.py:80-94,
wan/modules/vae.py:517-543) on CPU in bf16 with the synthetic encoder weights, for the cases of tests/vae_enc_ref.py.  Run by hand
where the reference tree is present (LONGLIVE_REFERENCE, through oracle/ref_import.py's shims); no test imports the reference.
Only outputs and seeds are stored: inputs and weights are regenerated from the seeds."""
import importlib
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from longlive_amd import synth  # noqa: E402
from oracle import ref_import, ref_vae  # noqa: E402
import vae_enc_ref as ER  # noqa: E402


def main():
    torch.manual_seed(0)
    ns = ref_import.load_pipelines()
    vae = importlib.import_module("wan.modules.vae")
    cfg = synth.VaeConfig()
    sd = dict(synth.synth_vae_state_dict(cfg, seed=5))
    sd.update(synth.synth_vae_encoder_state_dict(cfg, seed=ER.ENC_SEED))
    model = vae.WanVAE_(dim=96, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=2, attn_scales=[], temperal_downsample=[False, True, True],
                        dropout=0.0)
    model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)      # every name of both halves is the reference's
    model = model.to(torch.bfloat16).eval().requires_grad_(False)
    W = ns.wan_wrapper.WanVAEWrapper
    wr = W.__new__(W)
    nn.Module.__init__(wr)
    wr.mean = torch.tensor(ref_vae.VAE_MEAN, dtype=torch.float32)
    wr.std = torch.tensor(ref_vae.VAE_STD, dtype=torch.float32)
    wr.model = model
    rec = {"enc_seed": ER.ENC_SEED, "cases": {k: dict(seed=s, shape=list(sh)) for k, (s, sh) in ER.CASES.items()}}
    with torch.no_grad():
        for tag in ER.CASES:
            px = ER.case_pixels(tag)
            t0 = time.time()
            out = wr.encode_to_latent(px)
            print(f"{tag}: {tuple(px.shape)} -> {tuple(out.shape)} in {time.time() - t0:.1f}s, std {float(out.std()):.3f}")
            assert out.dtype == torch.float32 and torch.equal(out.to(torch.bfloat16).float(), out)      # bf16 values: stored losslessly
            rec[tag] = out.to(torch.bfloat16)
        px6 = ER.case_pixels("t6")
        assert torch.equal(wr.encode_to_latent(px6[:, :, :5]), rec["t6"].float()), "frames beyond 1 + 4k must be dropped"
    path = os.path.join(ROOT, "tests", "golden", "vae_encode.pt")
    torch.save(rec, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
