"""A change that only re-schedules the peg-in-hole step must not move a bit.  step_env's scan of the 86 checked state words, one word per
lane with a flag in LDS where every lane used to read all 86 in turn, is such a change: the rollouts of tests/step_bits_rollout.py on this
build against tests/golden/step_bits_rollout.npz, recorded on the build before it -- iteration counts, solver variants, contact counts,
reward, done, observations and the final states, bit for bit.  (What the scan answers for non-finite words is the subject of
tests/test_gpu_step_stages.py::test_gpu_tail_nonfinite_reset.)

That the recording is worth comparing with is asserted on the recording itself: after reset the exit test ends solves after 20 and 36
iterations, the pre-rolled steps run every row-space solver variant with up to 25 contacts."""
import os

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import step_bits_rollout as X

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_bits_rollout.npz")


@pytest.fixture(scope="module")
def runs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    want = dict(np.load(GOLDEN))
    got = X.rollout(torch, PihVecEnv(X.N, seed=X.SEED, auto_reset=1))
    return want, got


def test_recording_covers_early_exits_and_every_variant(runs):
    want, _ = runs
    it = want["reset_iters"]
    seen = set(np.unique(it).tolist())
    print("   iteration counts after reset: %s ; pre-rolled: %s" % (sorted(seen), np.unique(want["prerolled_iters"]).tolist()))
    assert seen <= {1, 2, 3, 4, 20, 36, 50} and {20, 36, 50} <= seen                               # only checked iterations end a solve
    assert (it < 50).mean() > 0.05                                                                 # (779 of the 10 240 env-steps)
    assert {1, 2, 5} <= set(np.unique(want["prerolled_solver"]).tolist())                          # both one-row-per-lane variants, two rows per lane
    assert want["prerolled_ncontact"].max() >= 20 and want["prerolled_ncontact"].mean() > 4
    assert np.isfinite(want["reset_state"]).all() and np.isfinite(want["prerolled_state"]).all()


@pytest.mark.parametrize("part", ["reset", "prerolled"])
def test_rollout_bit_for_bit(runs, part):
    want, got = runs
    for k in X.ARRAYS:
        a, b = want[part + "_" + k], got[part + "_" + k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            raise AssertionError("%s_%s differs at %d places, first %s: recorded %r, this build %r" % (part, k, len(bad), bad[0].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))
    assert got[part + "_state"].shape == (X.N, _lib.S_CACHE_LAMBDA + 48)
