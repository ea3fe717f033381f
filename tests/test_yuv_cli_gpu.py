"""The CLI's `video_codec: y4m` and `.y4m` `input_video` on the GPU in synthetic mode, shrunk like tests/test_cli_gpu.py: the run's
frames leave the pipeline as I420 and land in a YUV4MPEG2 file; that file is continued with `input_rate: match` at a header rate of
32:1 (every second frame), and a file of twice the size is continued with `input_fit: cover`."""
import numpy as np
import pytest
import torch

import yuv_ref as R
from longlive_amd import cli, y4m

pytestmark = pytest.mark.gpu


def _config(tmp_path, **kw):
    base = dict(profile=False, denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3), output_folder=str(tmp_path / "out"),
                inference_iter=-1, num_output_frames=3, use_ema=False, seed=0, num_samples=1, save_with_index=True,
                global_sink=True, context_noise=0, synthetic=True,
                synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12))
    base.update(kw)
    return cli.Config(**base)


def test_cli_writes_y4m_and_continues_it_at_a_matched_rate(tmp_path, monkeypatch):
    from longlive_amd.pipeline import CausalInferencePipeline
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    dev = torch.device("cuda", 0)
    seen = []
    inference = CausalInferencePipeline.inference

    def spy(self, *a, **k):
        out = inference(self, *a, **k)
        seen.append((k.get("frames"), k.get("yuv_range"), out[0].cpu()))
        return out

    monkeypatch.setattr(CausalInferencePipeline, "inference", spy)
    recs = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="y4m", yuv_range="full"), device=dev)
    assert len(recs) == 1 and recs[0]["codec"] == "y4m" and recs[0]["range"] == "full" and recs[0]["frames"] == 9
    assert recs[0]["path"].endswith(".y4m")
    raw = open(recs[0]["path"], "rb").read()
    n = R.yuv420_bytes(64, 96)
    assert recs[0]["bytes"] == len(raw) == len(b"YUV4MPEG2 W96 H64 F16:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n") + 9 * (6 + n)
    with y4m.Y4MReader(recs[0]["path"]) as r:
        payloads = list(r)
        assert (r.width, r.height, r.fps, r.layout, r.range) == (96, 64, 16, "420jpeg", "full")
    assert seen[0][:2] == ("yuv420", "full") and seen[0][2].shape == (1, 9, n)
    assert payloads == [bytes(row) for row in seen[0][2][0].numpy()]            # the file's payloads are the pipeline's bytes
    assert np.frombuffer(payloads[0], np.uint8)[:64 * 96].std() > 1.0
    # continue it as if it had been shot at 32 frames/s: every second frame, counted back from the last
    fast = tmp_path / "fast.y4m"
    fast.write_bytes(raw.replace(b" F16:1 ", b" F32:1 ", 1))
    clips = []
    load = cli.load_clip_y4m

    def spy_load(*a, **k):
        out = load(*a, **k)
        clips.append(out[0].cpu())
        return out

    monkeypatch.setattr(cli, "load_clip_y4m", spy_load)
    cont = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="y4m", input_video=str(fast), input_rate="match",
                                        output_folder=str(tmp_path / "cont")), device=dev)
    assert cont[0]["input_rate"] == [32, 1] and cont[0]["input_frames"] == 5 and "input_size" not in cont[0]
    assert cont[0]["frames"] == 1 + 4 * (2 + 3 - 1) and cont[0]["codec"] == "y4m" and cont[0]["range"] == "limited"
    picked = np.stack([np.frombuffer(payloads[i], np.uint8) for i in (0, 2, 4, 6, 8)])
    want = R.planes_to_rgb(*R.i420_planes(picked, 64, 96), "420jpeg", "full")
    assert torch.equal(clips[0], torch.from_numpy(want))
    with y4m.Y4MReader(cont[0]["path"]) as r:
        assert len(list(r)) == 17 and r.range == "limited"
    # input_rate: keep (the default) takes the last frames as they are
    kept = cli.load_clip_y4m(_config(tmp_path, input_video=str(fast), input_frames=5), 8, 12, dev)
    assert kept[1] is None and kept[2] is None
    want = R.planes_to_rgb(*R.i420_planes(np.stack([np.frombuffer(f, np.uint8) for f in payloads[4:]]), 64, 96), "420jpeg", "full")
    assert torch.equal(clips[1], torch.from_numpy(want))


def test_cli_continues_a_larger_y4m_with_cover(tmp_path):
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    yy, xx = np.mgrid[0:128, 0:192]
    frames = np.stack([np.stack([(xx + 9 * t) % 256, (2 * yy + 5 * t) % 256, (xx + yy) % 256], -1) for t in range(6)]).astype(np.uint8)
    big = str(tmp_path / "big.y4m")
    y4m.write_y4m(big, iter(R.rgb_to_i420(frames, "limited")), 192, 128)
    cfg = _config(tmp_path, data_path=str(p), input_video=big, input_fit="cover", video_codec="y4m")
    recs = cli.run("inference", cfg, device=torch.device("cuda", 0))
    assert recs[0]["input_size"] == [192, 128] and recs[0]["input_frames"] == 5 and "input_rate" not in recs[0]
    assert recs[0]["frames"] == 1 + 4 * (2 + 3 - 1) and recs[0]["codec"] == "y4m" and recs[0]["range"] == "limited"
    with pytest.raises(ValueError, match="input_fit"):
        cli.run("inference", _config(tmp_path, data_path=str(p), input_video=big), device=torch.device("cuda", 0))
