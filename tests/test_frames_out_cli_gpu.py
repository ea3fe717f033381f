"""The CLI's `video_codec: mjpeg` key on the GPU in synthetic mode, shrunk like tests/test_cli_gpu.py: the run's frames leave the
pipeline as uint8, are encoded by the GPU JPEG encoder, land in an MJPEG .avi, and that file is continued as `input_video`."""
import io

import numpy as np
import pytest
import torch

import jpeg_ref as J
from longlive_amd import cli

pytestmark = pytest.mark.gpu


def _config(tmp_path, **kw):
    base = dict(profile=False, denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3), output_folder=str(tmp_path / "out"),
                inference_iter=-1, num_output_frames=3, use_ema=False, seed=0, num_samples=1, save_with_index=True,
                global_sink=True, context_noise=0, synthetic=True,
                synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12))
    base.update(kw)
    return cli.Config(**base)


def test_cli_writes_mjpeg_and_continues_it(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    dev = torch.device("cuda", 0)
    plain = cli.run("inference", _config(tmp_path, data_path=str(p), output_folder=str(tmp_path / "plain")), device=dev)
    recs = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="mjpeg", jpeg_quality=90), device=dev)
    assert len(recs) == 1 and recs[0]["codec"] == "mjpeg" and recs[0]["frames"] == 9 and recs[0]["path"].endswith(".avi")
    raw = open(recs[0]["path"], "rb").read()
    assert recs[0]["bytes"] == len(raw) < 9 * 64 * 96 * 3 and cli.avi_compression(recs[0]["path"]) == b"MJPG"
    got = cli.read_input_video(recs[0]["path"])
    assert got.shape == (9, 64, 96, 3) and got.dtype == torch.uint8
    if plain[0]["path"].endswith(".avi"):                       # the same run written uncompressed (no torchvision + PyAV here)
        want = cli.read_avi_rgb24(plain[0]["path"]).numpy()
        assert want.std() > 1.0
        for t in range(9):                                      # the rule of tests/test_frames_out_gpu.py: PIL's encoder - 0.1 dB
            b = io.BytesIO()
            Image.fromarray(want[t]).save(b, "JPEG", quality=90, subsampling=2)
            ours, pil = J.psnr(got[t].numpy(), want[t]), J.psnr(np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB")), want[t])
            print(f"frame {t}: ours {ours:.3f} dB, PIL {pil:.3f} dB")
            assert ours >= pil - 0.1, (t, ours, pil)
    cont = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="mjpeg", input_video=recs[0]["path"],
                                        output_folder=str(tmp_path / "cont")), device=dev)
    assert cont[0]["input_frames"] == 9 and cont[0]["frames"] == 1 + 4 * (3 + 3 - 1) and cont[0]["codec"] == "mjpeg"
    assert cli.read_avi_mjpeg(cont[0]["path"]).shape == (21, 64, 96, 3)


def test_cli_interactive_writes_mjpeg(tmp_path):
    import json
    j = tmp_path / "m.jsonl"
    j.write_text(json.dumps({"prompts": ["scene part 0", "scene part 1"]}) + "\n")
    cfg = _config(tmp_path, data_path=str(j), switch_frame_indices="3", global_sink=False, num_output_frames=6, video_codec="mjpeg",
                  jpeg_quality=50, num_samples=2)
    recs = cli.run("interactive", cfg, device=torch.device("cuda", 0))
    assert len(recs) == 2 and all(r["codec"] == "mjpeg" and r["frames"] == 21 for r in recs)
    assert recs[0]["path"] != recs[1]["path"] and all(cli.avi_compression(r["path"]) == b"MJPG" for r in recs)
