"""The host logic of longlive_amd/vae.py held to the launches recorded in tests/golden/vae_launch_trace.json (tests/vae_trace.py runs
the real decoder and encoder on CPU tensors over recording ops; tools/record_vae_goldens.py wrote the file, which names the commit):
the same ll calls on the same views in the same order, every history frame from the same launch, the same torch copies between them.
On a mismatch, `python tests/vae_trace.py --dump FILE` here and in a checkout of that commit gives two files to diff."""
import json
import os

import pytest
import torch

import vae_trace as VT
from conftest import GOLDEN as GOLDEN_DIR
from longlive_amd import synth

bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "vae_launch_trace.json")) as f:
        return json.load(f)["scenarios"]


@pytest.mark.parametrize("setting", VT.SETTINGS)
@pytest.mark.parametrize("scenario", list(VT.SCENARIOS))
def test_launch_trace_is_the_recorded_one(golden, scenario, setting):
    got, want = VT.summary(VT.run(scenario, setting)), golden[scenario][setting]
    assert got["counts"] == want["counts"]
    assert got["sha256"] == want["sha256"], "same counts, another order, view or history frame: diff two --dump files"


def _halves():
    from longlive_amd.vae import WanVAEDecoderHIP, WanVAEEncoderHIP
    for cls in (WanVAEDecoderHIP, WanVAEEncoderHIP):
        m = cls(synth.VaeConfig(), device="cpu", fuse_rms=True)
        m._pack()                                                              # torch only: no library call
        yield m


def test_every_consumer_of_a_fused_handoff_is_temporal():
    """_consumer offers the handoff to temporal convolutions only; in both layouts of the default VaeConfig that is every residual
    block's first convolution and the head's, so nothing is held back by the condition."""
    for m in _halves():
        readers = [(i - 1, L[1] + ".residual.2") for i, L in enumerate(m.layers) if L[0] == "res"] + [(len(m.layers) - 1, m._head[1])]
        assert len(readers) == sum(L[0] == "res" for L in m.layers) + 1
        for i, name in readers:                                                # layer i's output (i = -1: the front end's) is read by `name`
            assert m._convs[name].hist == 2, name
            gamma, conv = m._consumer(i)
            assert conv is m._convs[name]
        others = [i for i in range(-1, len(m.layers)) if i not in dict(readers)]
        assert all(m._consumer(i) is None for i in others)                     # an attention block or a resample comes next


@pytest.mark.parametrize("T,H", [(3, 2), (2, 3)])
def test_a_staged_input_of_the_wrong_size_raises(T, H):
    dec = next(_halves())
    x = torch.zeros(2, 2, 4, 384, dtype=bf16)
    wrong = dec._convs["decoder.middle.0.residual.2"].input(T, H, 4, "cpu")
    with pytest.raises(RuntimeError, match="staged input"):
        dec._res_block(x, "decoder.middle.0", wrong)
    with pytest.raises(RuntimeError, match="staged input"):
        dec._walk(x, wrong)


def test_time_conv_input_before_any_frame_raises():
    enc = list(_halves())[1]
    tc = next(c for n, c in enc._convs.items() if n.endswith(".time_conv"))
    with pytest.raises(RuntimeError, match="before the stream's first chunk"):
        tc.input(4, 4, 8, "cpu")
