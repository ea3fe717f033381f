"""Times the HIP VAE encoder at the real geometry (480x832 pixels -> 60x104 latents), synthetic weights, beside the decoder on the
same device.   usage: python tools/vae_encode_bench.py [out.json]   (prints one JSON line; also written to out.json)
Records: the T = 5 call (1 + 4 frames, HIP events), the steady 4-frame step, a per-launch table of the two strided kernels
(ll_conv_cl_down, ll_conv_cl_tdown) at their shipped shapes and of encoder.conv1 at both input paddings (Cpad 8: generic decode +
RMS_norm launch; Cpad 32: halo-tile kernel with the fused RMS_norm), and the decoder's pixel-frame rate."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longlive_amd import ops, synth  # noqa: E402
from longlive_amd.vae import WanVAEWrapper, _Conv  # noqa: E402

bf = torch.bfloat16


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def main():
    dev = "cuda"
    cfg = synth.VaeConfig()
    vae = WanVAEWrapper(cfg, device=dev, chunk=2)
    sd = dict(synth.synth_vae_state_dict(cfg, seed=5, device=dev))
    sd.update(synth.synth_vae_encoder_state_dict(cfg, seed=6, device=dev))
    vae.load_state_dict(sd)
    px = (synth.hash_uniform(71, "vae.pixels.real", (1, 3, 9, 480, 832), dev) * 2.0 - 1.0).to(bf)
    rec = {"device": torch.cuda.get_device_name(0), "geometry": "480x832"}
    rec["encode_T5_ms"] = timed(lambda: vae.encode_to_latent(px[:, :, :5]), 3)
    vae.encoder.clear_cache()
    vae.encode_to_latent(px[:, :, :1], keep_cache=True)
    rec["encode_step4_ms"] = timed(lambda: vae.encode_to_latent(px[:, :, 1:5], keep_cache=True), 3)
    rec["encode_pixel_frames_per_s"] = 4000.0 / rec["encode_step4_ms"]
    vae.encoder.chunk = 8
    rec["encode_step8_ms"] = timed(lambda: vae.encode_to_latent(px[:, :, 1:9], keep_cache=True), 3)
    vae.encoder.chunk = 4
    vae.encoder.clear_cache()
    # decoder beside it: steady state, 2 latent frames = 8 pixel frames per step
    lat = synth.hash_normal(9, "lat", (1, 5, 16, 60, 104), dev).to(bf)
    vae.model.clear_cache()
    vae.decode_to_pixel(lat[:, :1], use_cache=True)
    dms = timed(lambda: vae.decode_to_pixel(lat[:, 1:3], use_cache=True), 3)
    vae.model.clear_cache()
    rec["decode_step2_ms"], rec["decode_pixel_frames_per_s"] = dms, 8000.0 / dms
    # per-launch table
    table = {}
    enc = vae.encoder
    for name, kind, T, H, W in (("encoder.downsamples.2.resample.1", 0, 4, 480, 832), ("encoder.downsamples.5.resample.1", 0, 4, 240, 416),
                                ("encoder.downsamples.8.resample.1", 0, 2, 120, 208), ("encoder.downsamples.5.time_conv", 1, 4, 120, 208),
                                ("encoder.downsamples.8.time_conv", 1, 2, 60, 104)):
        c = enc._convs[name]
        cin, cout = c.geo[0], c.geo[1]
        x = torch.randn(T + kind, H, W, cin, device=dev).to(bf)
        fn = (lambda: ops.conv_cl_tdown(x, c.w, c.b, c.geo)) if kind else (lambda: ops.conv_cl_down(x, c.w, c.b, c.geo))
        ms = timed(fn)
        To, Ho, Wo = (T // 2, H, W) if kind else (T, H // 2, W // 2)
        fl = 2.0 * To * Ho * Wo * cout * (3 if kind else 9) * cin
        table[name] = dict(plan=ops.conv_down_plan(kind, T, H, W, cin, cout), ms=ms, tflops=fl / ms / 1e9,
                           in_gbps=x.numel() * 2 / ms / 1e6)
    w, b = enc._p("encoder.conv1.weight"), enc._p("encoder.conv1.bias")
    gamma = enc._gamma["encoder.downsamples.0.residual.0.gamma"]
    for cpad in (8, 32):
        wp = torch.zeros(96, cpad, 3, 3, 3, dtype=bf, device=dev)
        wp[:, :3] = w
        c = _Conv(wp, b)
        src = px[0, :, 1:5]

        def conv1():
            x = ops.pixels_to_cl(src, 0, cpad, out=c.input(4, 480, 832, dev))
            c(x, rms=(gamma, torch.empty(4, 480, 832, 96, dtype=bf, device=dev)), want_raw=True)

        table[f"encoder.conv1 cpad={cpad} (pixels_to_cl + conv + rms_silu)"] = dict(
            plan=ops.conv_plan(4, 480, 832, c.geo, rms=ops.conv_cl_rms_ok(c.geo, 480, 832)), ms=timed(conv1))
    rec["launches"] = table
    line = json.dumps(rec)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
