"""Record tests/golden/pair_pass_bits.json: tests/pair_pass_cases.py's record() on the library PIH_LIB_PATH names, on an MI355X.
The committed file was recorded on the build BEFORE the pair pass got its per-segment broad phase and compacted narrow phase (its parent
commit); record again, on the build before the change, when a change is MEANT to alter a self-collision contact.  The file names the
build that made it: the commit given as BUILD (free text) and the sha256 of the library file.
usage: PIH_LIB_PATH=/path/to/libpih_hip.so python tests/golden/make_pair_pass_golden.py BUILD [OUT.json]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from peg_in_hole_gym_amd import _lib  # noqa: E402
from tests import pair_pass_cases as X  # noqa: E402

build = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "pair_pass_bits.json")
got = X.record(torch)
got["build"] = {"commit": build, "library_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()}
with open(out, "w") as f:
    json.dump(got, f, separators=(",", ":"))
    f.write("\n")
print("wrote %s: %d cases, %d contacts, build %s" % (out, len(got["n"]), sum(got["n"]), got["build"]))
