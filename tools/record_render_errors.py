#!/usr/bin/env python3
"""Record what the camera entry points answer to bad calls: drives a 3-env peg-in-hole handle and a 3-env random-fly handle through the
table of tests/render_error_cases.py and writes tests/golden/render_errors.json, rows of [entry point, case name, return code, exact
pih_last_error text].  Needs a GPU.  Run it on the build whose behaviour is to be pinned -- before a change to the argument checks of
pih_hip.hip, not after; tests/test_gpu_render_errors.py replays the table against the file.
usage: python tools/record_render_errors.py [OUTPUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from peg_in_hole_gym_amd.vec_env import PihVecEnv  # noqa: E402
from tests import render_error_cases as R  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "render_errors.json")
    hs = R.Handles(torch, PihVecEnv(R.N), PihVecEnv(R.N, task_id=1))
    rows = R.run_table(hs)
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d rows (%d with a non-zero return code) -> %s" % (len(rows), sum(r[2] != 0 for r in rows), path))


if __name__ == "__main__":
    main()
