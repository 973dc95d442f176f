"""Collision detection may be re-scheduled, never re-computed: every contact of every case of tests/collision_cases.py (2249 cases, classes
T H F A S C M) on this build against tests/golden/collision_bits.json, recorded on the build before collide() got its wave form
(pih_wave.h: table constants read once, one walk over the pipe samples, slots handed out afterwards) -- contact count, the arm-involving
contacts, and a digest of the live rows' geometry words in slot order, bit for bit.

That the recording is worth comparing with is asserted on the recording itself: full contact lists (48), capped arm passes that
overflow, contacts from the samples 63 and 64 (the last lane of the first chunk of 64 samples, the first of the second) and 122 (the
last sample), and every class."""
import json
import os

import numpy as np
import pytest

from tests import collision_bits_run as X
from tests import collision_cases as K

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collision_bits.json")


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return X.record(torch)


def test_recording_covers_caps_chunk_boundaries_and_every_class(want):
    assert set(want) == set(K.CLASSES)
    total = 0; full = 0; overflow = 0; seen = 0
    for name in K.CLASSES:
        cs = K.cases(name); w = want[name]
        assert len(w["n"]) == len(w["arm"]) == len(w["samples"]) == len(w["digest"]) == len(cs) > 0, name
        assert max(w["n"]) > 0, name
        total += len(cs)
        full += sum(n == K.CMAX for n in w["n"])
        # a capped pass overflowed: the reference holds more arm-involving candidates than the cap, the recording kept exactly the cap
        overflow += sum(c.narm > K.CAMAX and a == K.CAMAX for c, a in zip(cs, w["arm"]))
        for s in w["samples"]:
            seen |= s
        assert all(a <= K.CAMAX and a <= n <= K.CMAX for a, n in zip(w["arm"], w["n"])), name
    print("   recording: %d cases, %d with %d contacts, %d with an overflowing arm pass, watched samples %s" % (total, full, K.CMAX, overflow, bin(seen)))
    assert total == 2249
    assert full >= 10 and overflow >= 5
    assert seen == (1 << len(X.WATCHED_SAMPLES)) - 1                   # samples 63, 64 and 122 each gave a contact


@pytest.mark.parametrize("name", K.CLASSES)
def test_class_bit_for_bit(want, got, name):
    w, g = want[name], got[name]
    for field in ("n", "arm", "samples", "digest"):
        if w[field] != g[field]:
            bad = [i for i, (a, b) in enumerate(zip(w[field], g[field])) if a != b]
            cs = K.cases(name)
            raise AssertionError("class %s: %r differs in %d of %d cases, first case %d (%s): recorded %r, this build %r" % (
                name, field, len(bad), len(cs), bad[0], cs[bad[0]].tag, w[field][bad[0]], g[field][bad[0]]))
    assert np.sum(g["n"]) == np.sum(w["n"])
