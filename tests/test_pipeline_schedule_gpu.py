"""The stream schedule of the delivery path on the device, held to tests/golden/pipeline_stream_schedule.json (tests/pipeline_trace.py,
device half; tools/record_pipeline_goldens.py recorded the file on an MI355X, and it names the commit): every generator call, decode,
JPEG encode, fetch, wait, event and record_stream on the stream it was on when the file was recorded, in the same order -- what the
bit-for-bit tests cannot see, since a decode or a wait on another stream usually still gives the same bytes -- and the outputs'
SHA-256 from the same recording.  Toy pipeline and VAE of tests/test_frames_out_gpu.py: latents 8 x 12, 9 new frames, 3 per block."""
import json
import os

import pytest

import pipeline_trace as PT
from conftest import GOLDEN as GOLDEN_DIR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "pipeline_stream_schedule.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def toy():
    return PT.make_toy()


@pytest.mark.parametrize("entry", PT.SCHED_ENTRIES)
def test_stream_schedule_and_outputs_are_the_recorded_ones(golden, toy, entry):
    assert sorted(c for c in golden if c.startswith(entry + "/")) == sorted(PT.schedule_cases(entry))
    for case in PT.schedule_cases(entry):
        got, want = PT.run_schedule(toy, case), golden[case]
        assert got["log"] == want["log"], case
        assert got["sha256"] == want["sha256"], case
