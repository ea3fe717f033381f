#!/usr/bin/env python3
"""Records what longlive_amd/ops.py hands to the library (tests/golden/ops_call_trace.json, for tests/test_ops_trace_host.py): the
signatures of its public functions, the rows of every wrapper case and a summary of every model case of tests/ops_trace.py.  Run by
hand against the `longlive_amd` package the later ones are to equal, never against the one under test: SOURCE is a checkout of that
commit, and its commit hash is written into the file's header.  Host only: no device, no built library.

  python tools/record_ops_goldens.py SOURCE [--out OUT]

Everything is recorded twice and the two must agree: what differs between two runs of one package cannot be held to a golden.  The
cases live in tests/ops_trace.py; this tool only runs them."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv):
    source = os.path.abspath(argv[0])
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "tests", "golden", "ops_call_trace.json")
    import ops_trace as OT
    print(f"longlive_amd from {OT.use_package_source(source).__file__}")
    commit = subprocess.run(["git", "-C", source, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    runs = [OT.record() for _ in range(2)]
    differ = [f"{part}: {name}" for part in runs[0] for name in runs[0][part] if runs[0][part][name] != runs[1][part].get(name)]
    if differ:
        raise SystemExit(f"two recordings disagree on {differ}")
    with open(out, "w") as f:
        json.dump({"recorded_from": commit, "what": "tests/ops_trace.py: signatures of ops' public functions, rows per wrapper case, "
                   "call counts and SHA-256 of the rows per model case", **runs[0]}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(runs[0]['cases'])} wrapper cases and {len(runs[0]['model'])} model cases recorded twice from {commit}, the two agree")


if __name__ == "__main__":
    main(sys.argv[1:])
