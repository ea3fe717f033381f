"""The CLI's `input_video` key on the GPU in synthetic mode, shrunk like tests/test_cli_gpu.py: a 9-frame clip on disk -> VAE encoder
(3 latents) -> continued by both entry points -> video file of the whole timeline."""
import json

import pytest
import torch

from longlive_amd import cli

pytestmark = pytest.mark.gpu


def _config(tmp_path, **kw):
    base = dict(profile=False, denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3), output_folder=str(tmp_path / "out"),
                inference_iter=-1, num_output_frames=6, use_ema=False, seed=0, num_samples=1, save_with_index=True,
                global_sink=True, context_noise=0, synthetic=True,
                synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12))
    base.update(kw)
    return cli.Config(**base)


def _clip(path, T, H, W, seed=3):
    frames = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    cli.write_avi_rgb24(str(path), frames)
    return frames


def test_cli_inference_continues_a_clip(tmp_path):
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    _clip(tmp_path / "clip.avi", 9, 64, 96)
    T = 6
    cfg = _config(tmp_path, data_path=str(p), input_video=str(tmp_path / "clip.avi"), num_output_frames=T)
    recs = cli.run("inference", cfg, device=torch.device("cuda", 0))
    assert len(recs) == 1 and recs[0]["frames"] == 1 + 4 * (3 + T - 1) and recs[0]["input_frames"] == 9
    if recs[0]["path"].endswith(".avi"):
        v = cli.read_avi_rgb24(recs[0]["path"])
        assert v.shape == (33, 64, 96, 3) and v.float().std() > 1.0
    cfg.input_frames = 7                                     # the cap: the last 5 frames, 2 latents
    recs = cli.run("inference", cfg, device=torch.device("cuda", 0))
    assert recs[0]["frames"] == 1 + 4 * (2 + T - 1) and recs[0]["input_frames"] == 5


def test_cli_interactive_continues_a_clip(tmp_path):
    j = tmp_path / "m.jsonl"
    j.write_text(json.dumps({"prompts": ["scene part 0", "scene part 1"]}) + "\n")
    _clip(tmp_path / "clip.avi", 9, 64, 96)
    cfg = _config(tmp_path, data_path=str(j), switch_frame_indices="6", global_sink=False, num_output_frames=6,
                  input_video=str(tmp_path / "clip.avi"))
    recs = cli.run("interactive", cfg, device=torch.device("cuda", 0))
    assert len(recs) == 1 and recs[0]["frames"] == 33 and recs[0]["input_frames"] == 9


def test_cli_refuses_a_clip_of_the_wrong_size(tmp_path):
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    _clip(tmp_path / "small.avi", 5, 32, 96)
    cfg = _config(tmp_path, data_path=str(p), input_video=str(tmp_path / "small.avi"))
    with pytest.raises(ValueError, match="96x32.*96x64.*not resized"):
        cli.run("inference", cfg, device=torch.device("cuda", 0))
