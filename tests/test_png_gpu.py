"""Lossless frames out on the GPU ("Lossless frames: PNG"): the filter stage, the zlib compressor and whole
files byte for byte against the restatement (tests/png_ref.py, itself checked by zlib and PIL in test_png_host.py) and through PIL /
zlib back to the input; the CLI's `video_codec: png | apng` against the uint8 frames the pipeline handed to the writer."""
import functools
import io
import zlib

import numpy as np
import pytest
import torch

import png_cases as K
import png_ref as R
from longlive_amd import cli

pytestmark = pytest.mark.gpu
DEV = "cuda"
Image = pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as o
    return o


def decode_png(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- filter --------------------------------------------------------------------------------------------------------------------------
FILTER = K.filter_frames()


@pytest.mark.parametrize("name", sorted(FILTER))
def test_filter_rows_are_the_restatements(ops, name):
    frames = FILTER[name]
    got = ops.png_filter(dev(frames)).cpu().numpy()
    want = R.filter_frames(frames)
    assert got.shape == want.shape and np.array_equal(got[..., 0], want[..., 0]), "filter types"
    assert np.array_equal(got, want)
    if name.startswith("wins_by_one_"):
        assert got[0, 2, 0] == int(name[-1])
    if name == "tie":
        assert got[0, 0, 0] == 1


def test_filter_and_files_of_three_frames_with_a_padded_stride(ops):
    g = np.random.default_rng(17)
    H, W = 17, 33
    frames = np.stack([K.whole_frames()["gradient_17x33"], g.integers(0, 256, (H, W, 3), dtype=np.uint8), np.full((H, W, 3), 200, np.uint8)])
    pad = torch.full((3, H * W * 3 + 37), 0xA5, dtype=torch.uint8, device=DEV)
    view = pad[:, :H * W * 3].view(3, H, W, 3)
    view.copy_(dev(frames))
    assert view.stride(0) == H * W * 3 + 37
    assert np.array_equal(ops.png_filter(view).cpu().numpy(), R.filter_frames(frames))
    buf, sizes = ops.png_encode(view)
    files = ops.png_bytes(buf, sizes)
    assert files == [R.png_file(f) for f in frames]
    assert files[1] == ops.png_bytes(*ops.png_encode(dev(frames[1:2])))[0]          # no state leaks between frames
    assert bool((pad[:, H * W * 3:] == 0xA5).all())


# ---- compressor ----------------------------------------------------------------------------------------------------------------------
ROWS = K.compressor_rows()


@functools.lru_cache(maxsize=None)
def restated(name):
    return R.zlib_compress(ROWS[name])


@pytest.mark.parametrize("name", sorted(ROWS))
def test_zlib_streams_are_the_restatements(ops, name):
    row = ROWS[name]
    buf, sizes = ops.zlib_compress(dev(row[None]))
    assert buf.shape == (1, R.zlib_capacity(row.size)) and int(sizes[0]) <= buf.shape[1]
    got, = ops.png_bytes(buf, sizes)
    assert zlib.decompress(got) == row.tobytes()
    assert got == restated(name)


def test_rows_of_one_call_share_nothing(ops):
    a = ROWS["few_values_16385"]
    b = np.random.default_rng(23).integers(0, 256, a.size, dtype=np.uint8)
    c = np.full(a.size, 3, np.uint8)
    pad = torch.full((3, a.size + 11), 0x5A, dtype=torch.uint8, device=DEV)
    pad[:, :a.size] = dev(np.stack([a, b, c]))
    got = ops.png_bytes(*ops.zlib_compress(pad[:, :a.size]))                       # a row stride that is no multiple of anything
    assert got == [R.zlib_compress(a), R.zlib_compress(b), R.zlib_compress(c)]
    assert got[0] == restated("few_values_16385") and len(got[1]) == 2 + a.size + 10 + 4 <= R.zlib_capacity(a.size)
    assert [zlib.decompress(x) for x in got] == [a.tobytes(), b.tobytes(), c.tobytes()]


# ---- whole frames --------------------------------------------------------------------------------------------------------------------
WHOLE = K.whole_frames()


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_files_are_the_restatements_and_pil_reads_them(ops, name):
    frame = WHOLE[name]
    buf, sizes = ops.png_encode(dev(frame[None]))
    H, W, _ = frame.shape
    assert buf.shape == (1, R.png_capacity(H, W)) == (1, ops.png_sizes(1, H, W)[0]) and int(sizes[0]) <= buf.shape[1]
    got, = ops.png_bytes(buf, sizes)
    assert np.array_equal(decode_png(got), frame)
    assert all(ok for _, _, ok in R.read_chunks(got))
    assert got == R.png_file(frame)


def test_ops_wrappers(ops):
    frame = dev(WHOLE["gradient_16x16"][None])
    with pytest.raises(RuntimeError, match="expected uint8"):
        ops.png_encode(frame.float())
    with pytest.raises(RuntimeError, match="expected uint8"):
        ops.zlib_compress(frame.view(1, -1).float())
    strided = frame.view(1, -1)[:, ::2]                           # made contiguous by the wrapper
    got, = ops.png_bytes(*ops.zlib_compress(strided))
    assert zlib.decompress(got) == strided.cpu().numpy().tobytes()


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def _config(tmp_path, **kw):
    base = dict(profile=False, denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                model_kwargs=cli.Config(local_attn_size=12, timestep_shift=5.0, sink_size=3), output_folder=str(tmp_path / "out"),
                inference_iter=-1, num_output_frames=3, use_ema=False, seed=0, num_samples=1, save_with_index=True,
                global_sink=True, context_noise=0, synthetic=True,
                synthetic_overrides=cli.Config(num_layers=2, t5_layers=1, lat_h=8, lat_w=12))
    base.update(kw)
    return cli.Config(**base)


def test_cli_writes_png_files_and_an_apng(tmp_path, monkeypatch):
    import os
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    seen = []
    for name in ("_write_png", "_write_apng"):
        inner = getattr(cli, name)

        def spy(path, frames, inner=inner):
            seen.append(frames.cpu().numpy())                   # the uint8 frames the pipeline handed to the writer
            return inner(path, frames)

        monkeypatch.setattr(cli, name, spy)
    d = torch.device("cuda", 0)
    one = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="png", output_folder=str(tmp_path / "a")), device=d)
    two = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="apng", output_folder=str(tmp_path / "b")), device=d)
    assert len(seen) == 2 and seen[0].shape == (9, 64, 96, 3) and seen[0].std() > 1.0 and np.array_equal(seen[0], seen[1])
    assert len(one) == 1 and one[0]["codec"] == "png" and one[0]["frames"] == 9 and one[0]["path"].endswith(".frames")
    names = sorted(os.listdir(one[0]["path"]))
    assert names == [f"{t:05d}.png" for t in range(9)]
    files = [open(os.path.join(one[0]["path"], n), "rb").read() for n in names]
    assert one[0]["bytes"] == sum(map(len, files)) < 9 * 64 * 96 * 3
    assert np.array_equal(np.stack([decode_png(f) for f in files]), seen[0])
    assert len(two) == 1 and two[0]["codec"] == "apng" and two[0]["frames"] == 9 and two[0]["path"].endswith(".png")
    assert two[0]["bytes"] == os.path.getsize(two[0]["path"])
    with Image.open(two[0]["path"]) as im:
        assert im.n_frames == 9 and abs(im.info["duration"] - 62.5) < 1e-6
    assert np.array_equal(cli.read_input_video(two[0]["path"]).numpy(), seen[0])
    assert torch.equal(cli.load_clip(cli.Config(input_video=two[0]["path"]), 8, 12), torch.from_numpy(seen[0]))


def test_cli_continues_a_png_clip_as_it_does_its_frames(tmp_path):
    p = tmp_path / "prompts.txt"
    p.write_text("a cat on a mat\n")
    g = np.random.default_rng(31)
    yy, xx = np.mgrid[0:64, 0:96]
    frames = np.stack([np.stack([(3 * xx + 5 * t) % 256, (2 * yy + xx + t) % 256, (xx * yy // 8) % 256], -1) for t in range(5)])
    frames = (frames + g.integers(0, 4, frames.shape)).astype(np.uint8)
    from longlive_amd import ops
    files = ops.png_bytes(*ops.png_encode(dev(frames)))
    cli.write_apng(str(tmp_path / "clip.png"), files)
    torch.save(torch.from_numpy(frames), str(tmp_path / "clip.pt"))
    d = torch.device("cuda", 0)
    outs = []
    for k, clip in enumerate(("clip.png", "clip.pt")):
        recs = cli.run("inference", _config(tmp_path, data_path=str(p), video_codec="apng", input_video=str(tmp_path / clip),
                                            output_folder=str(tmp_path / f"cont{k}")), device=d)
        assert recs[0]["input_frames"] == 5 and recs[0]["frames"] == 1 + 4 * (2 + 3 - 1) and recs[0]["codec"] == "apng"
        outs.append(open(recs[0]["path"], "rb").read())
    assert outs[0] == outs[1]                                    # the same latents in, the same video out, byte for byte
    assert cli.read_input_video(str(tmp_path / "clip.png")).shape == (5, 64, 96, 3)
