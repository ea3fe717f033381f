"""Animated previews on the GPU ("Animated previews: GIF"): the LZW coder, the quantiser and whole files byte for
byte against the restatement (tests/gif_ref.py, itself checked by PIL in test_gif_host.py) and through PIL back to palette[indices]; the
CLI's `gif_preview` beside two codecs against gif.quantize of the frames the writer was handed, and `input_video: clip.gif`."""
import functools
import io
import os

import numpy as np
import pytest
import torch

import gif_cases as K
import gif_ref as R
from longlive_amd import cli

pytestmark = pytest.mark.gpu
DEV = "cuda"
Image = pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def gif():
    from longlive_amd import gif as g
    return g


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def decode_gif(data):
    with Image.open(io.BytesIO(data)) as im:
        assert im.n_frames == 1
        return np.asarray(im.convert("RGB"))


# ---- coder --------------------------------------------------------------------------------------------------------------------------
ROWS = K.lzw_rows()


@functools.lru_cache(maxsize=None)
def restated(name):
    return R.lzw(ROWS[name])


@pytest.mark.parametrize("name", sorted(ROWS))
def test_lzw_streams_are_the_restatements(gif, name):
    row = ROWS[name]
    buf, sizes = gif.lzw(dev(row[None]))
    assert buf.shape == (1, R.lzw_capacity(row.size)) and int(sizes[0]) <= buf.shape[1]
    got, = gif.files(buf, sizes)
    assert got == restated(name)


def test_rows_of_one_call_share_nothing(gif):
    n = 2 * K.C + 1
    a, b, c = ROWS[f"few_values_{n}"], ROWS[f"random_{n}"], ROWS[f"all_equal_{n}"]
    pad = torch.full((3, n + 11), 0x5A, dtype=torch.uint8, device=DEV)
    pad[:, :n] = dev(np.stack([a, b, c]))
    got = gif.files(*gif.lzw(pad[:, :n]))                          # a row stride that is no multiple of anything
    assert got == [restated(f"few_values_{n}"), restated(f"random_{n}"), restated(f"all_equal_{n}")]
    assert got[1] == gif.files(*gif.lzw(dev(b[None])))[0]


# ---- quantiser ----------------------------------------------------------------------------------------------------------------------
FRAMES = {**K.quantiser_frames(), **K.block_edge_frames()}
MODES = [(p, d) for p in R.PALETTES for d in R.DITHERS]


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_quantiser_and_files_are_the_restatements(gif, name):
    frames = FRAMES[name]
    T, H, W, _ = frames.shape
    for palette, dither in MODES:
        want_idx, want_pal, want_used = R.quantize(frames, palette, dither)
        idx, pal, used = gif.quantize(dev(frames), palette, dither)
        assert used.cpu().tolist() == want_used.tolist(), (palette, dither)
        assert np.array_equal(pal.cpu().numpy(), want_pal), (palette, dither)
        assert np.array_equal(idx.cpu().numpy(), want_idx), (palette, dither)
        buf, sizes = gif.encode(dev(frames), palette, dither)
        assert buf.shape == (T, R.file_capacity(H, W)) == (T, gif.sizes(T, H, W, palette)[0])
        files = gif.files(buf, sizes)
        for t, data in enumerate(files):
            p = want_pal[t if palette == "frame" else 0]
            assert np.array_equal(decode_gif(data), p[want_idx[t]]), (palette, dither, t)
            assert data == R.gif_file(want_idx[t], p), (palette, dither, t)


def test_three_frames_with_a_padded_stride(gif):
    frames = FRAMES["smooth_T3_33x47"]
    T, H, W, _ = frames.shape
    pad = torch.full((T, H * W * 3 + 37), 0xA5, dtype=torch.uint8, device=DEV)
    view = pad[:, :H * W * 3].view(T, H, W, 3)
    view.copy_(dev(frames))
    assert view.stride(0) == H * W * 3 + 37
    for palette, dither in MODES:
        want = R.quantize(frames, palette, dither)
        got = gif.quantize(view, palette, dither)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), (palette, dither)
        assert gif.files(*gif.encode(view, palette, dither)) == R.encode(frames, palette, dither)
    assert bool((pad[:, H * W * 3:] == 0xA5).all())
    assert want[1].shape == (T, 256, 3) and R.quantize(frames, "clip", "none")[1].shape == (1, 256, 3)


def test_wrappers(gif):
    frame = dev(FRAMES["smooth_7x9"])
    with pytest.raises(RuntimeError, match="expected uint8"):
        gif.encode(frame.float())
    with pytest.raises(RuntimeError, match="expected uint8"):
        gif.lzw(frame.view(1, -1).float())
    strided = frame.view(1, -1)[:, ::2]                            # made contiguous by the wrapper
    got, = gif.files(*gif.lzw(strided))
    assert got == R.lzw(strided.cpu().numpy()[0])


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------
def _config(tmp_path, **kw):
    base = dict(profile=False, denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3), output_folder=str(tmp_path / "out"),
                inference_iter=-1, num_output_frames=3, use_ema=False, seed=0, num_samples=1, save_with_index=True,
                global_sink=True, context_noise=0, synthetic=True,
                synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12))
    base.update(kw)
    return cli.Config(**base)


def test_cli_writes_a_preview_beside_png_and_y4m_and_continues_from_it(gif, tmp_path, monkeypatch):
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    handed = []
    inner = cli._write_gif_preview

    def spy(path, frames, preview):
        handed.append(frames.clone())                               # the uint8 RGB frames the preview writer was handed
        return inner(path, frames, preview)

    monkeypatch.setattr(cli, "_write_gif_preview", spy)
    d = torch.device("cuda", 0)
    one = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="png", gif_preview=True, output_folder=str(tmp_path / "a")),
                  device=d)
    two = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="y4m", gif_preview=True, gif_every=2, gif_size=[32, 40],
                                       gif_palette="frame", gif_dither="none", output_folder=str(tmp_path / "b")), device=d)
    assert len(handed) == 2
    assert one[0]["codec"] == "png" and one[0]["gif"].endswith(".gif") and one[0]["gif_bytes"] == os.path.getsize(one[0]["gif"])
    assert handed[0].shape == (9, 64, 96, 3) and handed[0].is_cuda and handed[0].float().std() > 1.0
    idx, pal, _ = gif.quantize(handed[0], "clip", "bayer")
    want = pal[0][idx.long()].cpu().numpy()
    with Image.open(one[0]["gif"]) as im:
        assert im.n_frames == 9 and im.size == (96, 64) and im.info["loop"] == 0
        for t in range(9):
            im.seek(t)
            assert im.info["duration"] == [60, 70, 60, 60][t % 4], t
            assert np.array_equal(np.asarray(im.convert("RGB")), want[t]), t

    assert two[0]["codec"] == "y4m" and two[0]["frames"] == 9 and handed[1].shape == (9, 64, 96, 3)
    from longlive_amd import ops
    kept = ops.resize_u8(handed[1][::2], (32, 40), fit="stretch")
    idx, pal, _ = gif.quantize(kept, "frame", "none")
    want2 = torch.stack([pal[t][idx[t].long()] for t in range(5)]).cpu().numpy()
    with Image.open(two[0]["gif"]) as im:
        assert im.n_frames == 5 and im.size == (40, 32)
        for t in range(5):
            im.seek(t)
            assert im.info["duration"] == [130, 120][t % 2], t
            assert np.array_equal(np.asarray(im.convert("RGB")), want2[t]), t

    assert np.array_equal(cli.read_input_video(one[0]["gif"]).numpy(), want)
    assert torch.equal(cli.load_clip(cli.Config(input_video=one[0]["gif"]), 8, 12), torch.from_numpy(want))
    recs = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="apng", input_video=one[0]["gif"],
                                        output_folder=str(tmp_path / "cont")), device=d)
    assert recs[0]["input_frames"] == 9 and recs[0]["frames"] == 1 + 4 * (3 + 3 - 1) and "gif" not in recs[0]
