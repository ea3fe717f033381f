#!/usr/bin/env python3
"""Records what the attention entry points answer (tests/golden/attn_plans.json) and write (tests/golden/attn_route_hashes.json) from the
library LONGLIVE_HIP_LIB names, for tests/test_attn_plans_host.py and tests/test_attn_routes_gpu.py to hold later libraries to.  Run by
hand against the library the later ones are to equal, never against the one under test:

  LONGLIVE_HIP_LIB=<that library> python tools/record_attn_goldens.py plans            # host only, no device needed
  LONGLIVE_HIP_LIB=<that library> python tools/record_attn_goldens.py routes [OUT]     # on an MI355X; OUT instead of the golden file

Record `routes` twice (two OUT files) and compare: a route whose bytes differ between two runs of one library cannot be held to a hash.
The cases live in the two test modules; this tool only runs them and writes the files."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    mode = sys.argv[1]
    assert os.environ.get("LONGLIVE_HIP_LIB"), "name the library to record from in LONGLIVE_HIP_LIB"
    if mode == "plans":
        import test_attn_plans_host as T
        doc = T.encode(T.answers(T._lib()))
        with open(T.GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join(f'"{k}": ' + ("[\n" + ",\n".join(json.dumps(t) for t in v) + "\n]" if k in ("strings", "refusals")
                                                      else json.dumps(v, separators=(",", ":"))) for k, v in doc.items()) + "\n}\n")
        print(f"{T.GOLDEN}: {os.path.getsize(T.GOLDEN)} bytes, {len(doc['strings'])} strings")
    else:
        import test_attn_routes_gpu as T
        out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
        doc = {name: T.run_route(name) for name in T.ROUTES}
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(f"{out}: {len(doc)} routes")


if __name__ == "__main__":
    main()
