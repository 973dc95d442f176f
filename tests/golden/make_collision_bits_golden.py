"""Record tests/golden/collision_bits.json: tests/collision_bits_run.py on the library PIH_LIB_PATH names, on an MI355X.
The committed file was recorded on the build BEFORE collide() got its wave form (its parent commit); record again, on the build before
the change, when a change is MEANT to alter a contact.
usage: PIH_LIB_PATH=/path/to/libpih_hip.so python tests/golden/make_collision_bits_golden.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tests import collision_bits_run as X  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "collision_bits.json")
got = X.record(torch)
with open(out, "w") as f:
    json.dump(got, f, separators=(",", ":"))
    f.write("\n")
print("wrote %s: %s" % (out, {k: len(v["n"]) for k, v in got.items()}))
