"""Record tests/golden/step_bits_rollout.npz: the rollouts of tests/step_bits_rollout.py on the library PIH_LIB_PATH names, on an MI355X.
The committed file was recorded on the build BEFORE step_env's finiteness scan became lane-parallel (its parent commit); record again, on
the build before the change, when a change is MEANT to alter the step's arithmetic.
usage: PIH_LIB_PATH=/path/to/libpih_hip.so python tests/golden/make_step_bits_golden.py [OUT.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from peg_in_hole_gym_amd.vec_env import PihVecEnv  # noqa: E402
from tests import step_bits_rollout as X  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "step_bits_rollout.npz")
got = X.rollout(torch, PihVecEnv(X.N, seed=X.SEED, auto_reset=1))
np.savez_compressed(out, **got)
print("wrote %s: %s" % (out, {k: v.shape for k, v in got.items()}))
