"""The pair pass may be re-scheduled, never re-computed: the cases of tests/pair_pass_cases.py (survivor lists of 0, 1, 63, 64, 65 ... 253
entries, emitting pairs at list positions 63 and 64 and at the old chunk boundaries, CMAX reached inside the pass, self collision off)
on this build against tests/golden/pair_pass_bits.json, recorded on the build BEFORE the pass got its per-segment broad phase and its
compacted narrow phase -- contact count, arm-involving contacts and a digest of the live rows' geometry words in slot order, bit for
bit.  One launch per config (299 envs and 1), one step each."""
import json
import os

import pytest

from tests import collision_cases as K
from tests import pair_pass_cases as PP

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_pass_bits.json")


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return PP.record(torch)


def test_recording_names_its_build_and_holds_full_lists_and_no_self_contact_with_selfcol_off(want):
    cs = PP.cases()
    assert len(want["build"]["commit"]) == 40 and len(want["build"]["library_sha256"]) == 64
    assert len(want["n"]) == len(want["arm"]) == len(want["digest"]) == len(cs)
    assert all(0 <= n <= K.CMAX for n in want["n"]) and sum(n == K.CMAX for n in want["n"]) >= 10
    assert want["n"][0] == 0 and want["n"][-1] == 0                    # the straight pipe; the whole pipe one bundle with self collision off
    # away from the discontinuities the recording holds what the reference holds: as many contacts
    plain = [i for i, c in enumerate(cs) if not c.sensitive]
    assert len(plain) >= 100 and all(want["n"][i] == len(cs[i].kept) for i in plain)


def test_bit_for_bit(want, got):
    cs = PP.cases()
    for field in ("n", "arm", "digest"):
        if want[field] != got[field]:
            bad = [i for i, (a, b) in enumerate(zip(want[field], got[field])) if a != b]
            raise AssertionError("%r differs in %d of %d cases, first case %d (%s): recorded %r, this build %r" % (
                field, len(bad), len(cs), bad[0], cs[bad[0]].tag, want[field][bad[0]], got[field][bad[0]]))
