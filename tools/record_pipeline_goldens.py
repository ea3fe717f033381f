#!/usr/bin/env python3
"""Records what the pipelines' delivery path calls on the host (tests/golden/pipeline_call_trace.json, for
tests/test_pipeline_trace_host.py) and how it schedules its streams on the device (tests/golden/pipeline_stream_schedule.json, for
tests/test_pipeline_schedule_gpu.py).  Run by hand against the `longlive_amd` package the later ones are to equal, never against the
one under test: `--source DIR` imports the package from DIR (a checkout of that commit; for `schedule` a copy of its package with the
built library in it will do); COMMIT is written into the file's header.

  python tools/record_pipeline_goldens.py trace COMMIT [--source DIR] [--out OUT]       # host only, no device, no library
  python tools/record_pipeline_goldens.py schedule COMMIT [--source DIR] [--out OUT]    # on an MI355X

Every case is recorded twice and the two must agree: what differs between two runs of one package cannot be held to a golden.  The
cases live in tests/pipeline_trace.py; this tool only runs them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _opt(argv, flag, default=None):
    return argv[argv.index(flag) + 1] if flag in argv else default


def main(argv):
    mode, commit = argv[0], argv[1]
    import pipeline_trace as PT
    if "--source" in argv:
        print(f"longlive_amd from {PT.use_package_source(_opt(argv, '--source')).__file__}")
    if mode == "trace":
        name, what = "pipeline_call_trace.json", "tests/pipeline_trace.py, host half: per case the call log, what came back, last_profile's keys"
        runs = [{case: PT.run_host(case) for case in PT.host_cases()} for _ in range(2)]
    else:
        name, what = "pipeline_stream_schedule.json", "tests/pipeline_trace.py, device half: per case the stream schedule and the SHA-256 of the output"
        toy = PT.make_toy()
        runs = [{case: PT.run_schedule(toy, case) for entry in PT.SCHED_ENTRIES for case in PT.schedule_cases(entry)} for _ in range(2)]
    differ = [case for case in runs[0] if runs[0][case] != runs[1][case]]
    if differ:
        raise SystemExit(f"two recordings disagree on {differ}")
    out = _opt(argv, "--out", os.path.join(ROOT, "tests", "golden", name))
    with open(out, "w") as f:
        json.dump({"recorded_from": commit, "what": what, "cases": runs[0]}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{out}: {len(runs[0])} cases recorded twice from {commit}, the two agree")


if __name__ == "__main__":
    main(sys.argv[1:])
