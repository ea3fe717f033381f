"""longlive_amd/ops.py held to the calls recorded in tests/golden/ops_call_trace.json (tests/ops_trace.py runs every public wrapper, and
the toy model over them, on the CPU against a recording fake of the library; tools/record_ops_goldens.py wrote the file): the same entry
points with the same integers, floats and pointers in the same order, the same timer tags and work values, the same results, the same
refusals with the same words, and the same public signatures.  The golden was recorded from commit
6914820 ("Add lossless frames out: a GPU PNG encoder, CLI png and apng codecs"), the last one before ops.py was consolidated; the
file names it too.  On a mismatch, `python tests/ops_trace.py --dump FILE` here and with `--source` a checkout of that commit gives
two files to diff."""
import json
import os
import re

import pytest

import ops_trace as OT
from conftest import GOLDEN as GOLDEN_DIR

RECORDED_FROM = "6914820"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "ops_call_trace.json")) as f:
        return json.load(f)


def test_the_golden_file_is_the_parents_and_holds_exactly_the_cases(golden):
    assert golden["recorded_from"].startswith(RECORDED_FROM)
    assert sorted(golden["cases"]) == sorted(OT.CASES)
    assert sorted(golden["model"]) == sorted(OT.model_cases())


def test_public_signatures_are_the_recorded_ones(golden):
    """Names, order and defaults: callers and the trace harnesses bind arguments by name.  Names added since are listed here."""
    added = set(OT.ADDED)
    got = OT.signatures()
    assert {n: s for n, s in got.items() if n not in added} == golden["signatures"]
    assert added <= set(got)
    assert got["ln_modulate_tab_q8"] == got["ln_modulate_tab_f8"] and got["gemm_w8a8_qkv_v_insert"] == got["gemm_f8_qkv_v_insert"]


@pytest.mark.parametrize("name", list(OT.CASES))
def test_wrapper_trace_is_the_recorded_one(golden, name):
    got = OT.run_case(name)
    assert got["rows"] == golden["cases"][name]
    assert got["events"] == 0


@pytest.mark.parametrize("name", list(OT.ADDED))
def test_a_name_added_since_repeats_the_recorded_rows_of_the_call_it_takes_over(golden, name):
    assert OT.run_case(name)["rows"] == golden["cases"][OT.ADDED[name][3]]


@pytest.mark.parametrize("name", list(OT.model_cases()))
def test_model_trace_is_the_recorded_one(golden, name):
    got, want = OT.summary(OT.run_model(name)), golden["model"][name]
    assert got["counts"] == want["counts"]
    assert got == want


def _untimed(rows):
    return [r for r in rows if r[0] != "timer"]


def test_without_a_timer_no_timer_row_and_no_event(golden):
    some_timed = 0
    for name in OT.CASES:
        got = OT.run_case(name, timed=False)
        assert got["rows"] == _untimed(golden["cases"][name]), name
        assert got["events"] == 0, name
        some_timed += len(got["rows"]) != len(golden["cases"][name])
    assert some_timed > 100
    for name in ("None/None", "mxfp8/mxfp8/fuse_attn_quant, kernel", "int8/None/fuse_v_insert off"):
        timed, plain = OT.run_model(name), OT.run_model(name, timed=False)
        assert plain["rows"] == _untimed(timed["rows"]) and len(plain["rows"]) < len(timed["rows"]), name
        assert plain["events"] == 0, name


def test_every_public_function_is_exercised_or_listed_host_only():
    from longlive_amd import ops
    used = set()
    for name in list(OT.CASES) + list(OT.ADDED):
        OT.run_case(name, used=used)
    public = set(OT.public_functions(ops))
    assert set(OT.HOST_ONLY) <= public
    assert public - used - set(OT.HOST_ONLY) == set()


def test_every_entry_point_is_reached_or_listed_never_called(golden):
    """The golden's rows cover the ABI but for the entries neither ops.py nor model.py names, and a search confirms each of those."""
    from longlive_amd import _lib
    reached = {r[0] for rows in golden["cases"].values() for r in rows if r[0].startswith("ll_")}
    for m in golden["model"].values():
        reached |= set(m["counts"])
    assert reached | set(OT.NEVER_CALLED) == set(_lib.SIGNATURES)
    assert not reached & set(OT.NEVER_CALLED)
    text = "".join(open(os.path.join(ROOT, "longlive_amd", f)).read() for f in ("ops.py", "model.py"))
    for entry in OT.NEVER_CALLED:
        assert not re.search(rf"\b{entry}\b(?!_)", text), entry


def test_the_patches_are_put_back():
    import torch
    from longlive_amd import _lib, ops
    before = (_lib.load, ops._stream, ops.timer, torch.cuda.current_stream, torch.cuda.current_device, torch.cuda.Event, torch.cuda._lazy_init,
              ops.gemm, ops.JPEG_SPLIT_AUTO_SEGMENTS)
    OT.run_case("gemm", used=set())
    OT.run_case("jpeg_decode/auto, many segments")
    assert before == (_lib.load, ops._stream, ops.timer, torch.cuda.current_stream, torch.cuda.current_device, torch.cuda.Event,
                      torch.cuda._lazy_init, ops.gemm, ops.JPEG_SPLIT_AUTO_SEGMENTS)
    assert not torch.zeros(1).is_cuda


def test_launches_and_buffers_go_through_the_helpers():
    """No wrapper checks a status or makes a plan buffer itself: `_lib.check` and `create_string_buffer` appear in the helpers alone."""
    src = open(os.path.join(ROOT, "longlive_amd", "ops.py")).read()
    assert len(re.findall(r"_lib\.check\(", src)) == 2, "one in the launch helper, one in the host-query helper"
    assert len(re.findall(r"create_string_buffer\(", src)) == 1
