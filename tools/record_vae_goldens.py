#!/usr/bin/env python3
"""Records what longlive_amd/vae.py launches (tests/golden/vae_launch_trace.json, for tests/test_vae_trace_host.py) and what the
assembled VAE writes (tests/golden/vae_pin_hashes.json, for tests/test_vae_pin_gpu.py).  Run by hand against the vae.py the later ones
are to equal, never against the one under test: `--vae FILE` loads a saved copy of that commit's vae.py as longlive_amd.vae, against
the tree's ops and library; COMMIT is written into the file's header.

  python tools/record_vae_goldens.py trace COMMIT [--vae FILE]               # host only, no device and no library needed
  python tools/record_vae_goldens.py pins COMMIT [--vae FILE] [--out OUT]    # on an MI355X; OUT instead of the golden file

Record `pins` twice (two OUT files) and compare: an output whose bytes differ between two runs of one vae.py cannot be held to a hash
and is left out of the golden file.  The cases live in tests/vae_trace.py and tests/test_vae_pin_gpu.py; this tool only runs them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _opt(argv, flag, default=None):
    return argv[argv.index(flag) + 1] if flag in argv else default


def main(argv):
    mode, commit = argv[0], argv[1]
    import vae_trace
    if "--vae" in argv:
        vae_trace.use_vae_source(_opt(argv, "--vae"))
    if mode == "trace":
        out = _opt(argv, "--out", os.path.join(ROOT, "tests", "golden", "vae_launch_trace.json"))
        doc = {"recorded_from": commit, "what": "tests/vae_trace.py: per scenario and setting, the per-op counts and the SHA-256 of the "
               "canonical JSON trace (python tests/vae_trace.py --dump FILE writes the rows themselves)", "scenarios": vae_trace.all_summaries()}
    else:
        import test_vae_pin_gpu as T
        from longlive_amd import ops
        out = _opt(argv, "--out", T.GOLDEN)
        vae = T.make_vae()
        doc = {"recorded_from": commit, "what": "tests/test_vae_pin_gpu.py: SHA-256 of each output's bytes on an MI355X",
               "outputs": {name: T.run_case(vae, name) for name in T.CASES}}
        for side, m, block, sizes in (("decoder", vae.model, "decoder.upsamples.%d.residual.2", ((0, 8, 12), (4, 16, 24), (8, 32, 48), (12, 64, 96))),
                                      ("encoder", vae.encoder, "encoder.downsamples.%d.residual.2", ((0, 64, 96), (3, 32, 48), (6, 16, 24), (9, 8, 12)))):
            for idx, H, W in sizes:                  # which kernel each stage's 3x3x3 convolutions run at this size
                geo = m._convs[block % idx].geo
                print(f"{side} {H}x{W}: {ops.conv_plan(2, H, W, geo, rms=ops.conv_cl_rms_ok(geo, H, W))}")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{out}: recorded from {commit}")


if __name__ == "__main__":
    main(sys.argv[1:])
