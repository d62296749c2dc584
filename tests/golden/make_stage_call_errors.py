"""Records tests/golden/stage_call_errors.json: what a build of the library answers to every call of tests/stage_call_cases.py, as
[return code, trgl_last_error text] per case, in two parts - "host" (c = NULL, needs no GPU) and "context" (one small context on GPU 0).

    python tests/golden/make_stage_call_errors.py host [--lib PATH] [--out FILE]
    python tests/golden/make_stage_call_errors.py context [--lib PATH] [--out FILE]

A run replaces the part it names and keeps the other.  The file is a characterisation of the build it was recorded from: record it
from the commit whose answers are to be kept, never from the code a test of it is about to judge."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import stage_call_cases as SC      # noqa: E402
from tinyrenderder_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=("host", "context"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "stage_call_errors.json"))
    a = ap.parse_args()
    L = api.load_library(a.lib)
    results = (SC.run_host_part(L) if a.part == "host" else SC.run_context_part(L))[0]
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc[a.part] = results
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.part}: {len(results)} cases -> {a.out}")


if __name__ == "__main__":
    main()
