"""The host logic of the delivery path held to the calls recorded in tests/golden/pipeline_call_trace.json (tests/pipeline_trace.py runs
both pipelines on the CPU over recording fakes; tools/record_pipeline_goldens.py wrote the file, which names the commit): the same
generator, VAE and JPEG calls with the same arguments in the same order, the same profiler marks between them, the same results.  On a
mismatch, `python tools/record_pipeline_goldens.py trace - --out FILE` here and in a checkout of that commit gives two files to diff."""
import json
import os

import pytest

import pipeline_trace as PT
from conftest import GOLDEN as GOLDEN_DIR


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "pipeline_call_trace.json")) as f:
        return json.load(f)["cases"]


def test_the_golden_file_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(PT.host_cases())


@pytest.mark.parametrize("case", PT.host_cases())
def test_call_trace_is_the_recorded_one(golden, case):
    got, want = PT.run_host(case), golden[case]
    assert got["log"] == want["log"]
    assert got == want


@pytest.mark.parametrize("entry", [e for e in PT.ENTRIES if e != "stream"])
@pytest.mark.parametrize("bad", PT.BAD_FORMS, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_a_bad_form_is_refused_before_anything_is_called(entry, bad):
    """Not a text encoder call, not a cache reset, not a launch."""
    exc, log = PT.run_refusal(entry, bad)
    key = "frames" if len(bad) == 1 else sorted(set(bad) - {"frames"})[0]
    assert isinstance(exc, ValueError) and str(exc).startswith(key + ":"), exc
    assert log == []
