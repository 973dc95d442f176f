"""The pipe's self-collision pass filters its 253 pairs by a predicate on per-segment records and walks ONE compacted list of the
survivors (pih_wave.h, collide; pih_common.h, segments_in_reach).  On the host: the case set of tests/pair_pass_cases.py holds what the
list handling can get wrong, and the predicate -- which may round differently from the per-pair one it replaces -- never filters out a
pair that has a contact: every self-collision contact of the independent reference (tests/collision_cases.py) is a survivor of the numpy
fp32 replica of the predicate, over the cases and over 2 000 random folded and random-joint states."""
import collections

import numpy as np

from tests import collision_cases as K
from tests import pair_pass_cases as PP


def test_case_set_covers_list_lengths_round_boundaries_and_the_cap():
    cs = PP.cases()
    assert 280 <= len(cs) <= 320 and len(K.group_by_config(cs)) == 2
    assert max(len(part) for part in K.group_by_config(cs).values()) <= PP.MAX_ENVS
    cov = PP.coverage(cs)
    n = collections.Counter(cov["counts"])
    print("   survivors per case: %s" % sorted(n.items()))
    for exact in (0, 1, 63, 64, 65, 253):
        assert n[exact] >= 1, "no case with exactly %d survivors" % exact
    for lo, hi in ((66, 128), (129, 192), (193, 252)):
        assert any(lo <= k <= hi for k in n), "no case with %d .. %d survivors" % (lo, hi)
    assert cov["straddle"] >= 1, "no case whose list entries 63 and 64 both emit a kept contact"
    assert cov["cap"] >= 1, "no case that reaches CMAX inside the pair pass behind table contacts"
    assert all(i in cov["emit_idx"] for i in PP.BOUNDARY_PAIRS), sorted(set(PP.BOUNDARY_PAIRS) - cov["emit_idx"])
    assert cov["selfcol0_full"] == 1 and cs[-1].cfg["selfcol"] == 0 and not any(1000 <= c.key < 2000 for c in cs[-1].kept)


def test_every_contact_of_the_reference_survives_the_fp32_predicate():
    checked = 0
    for c in PP.cases():
        if c.cfg["selfcol"]:
            sv = set(PP.survivors(c.state)[0].tolist())
            em = PP.emitters(c)
            assert sv.issuperset(em), (c.tag, sorted(set(em) - sv))
            checked += len(em)
    states = PP.random_states()
    assert len(states) == 2000
    with_contact = 0
    for s in states:
        sv = set(PP.survivors(s)[0].tolist())
        em = PP.self_emitters(s)
        assert sv.issuperset(em), sorted(set(em) - sv)
        checked += len(em); with_contact += bool(em)
    print("   %d contacts checked, %d of the random states have one" % (checked, with_contact))
    assert with_contact >= 500


def test_replica_is_fp32_and_agrees_with_the_exact_predicate_away_from_the_threshold():
    """the replica against the same inequality in fp64, on every pair that is not within 1e-5 (relative) of the threshold"""
    for c in PP.cases()[::7]:
        v = PP.vertices32(c.state); idx, _ = PP.survivors(c.state, v=v)
        v64 = v.astype(np.float64)
        mid = v64[:-1] + v64[1:]; ln = np.linalg.norm(v64[1:] - v64[:-1], axis=1)
        d = np.linalg.norm(mid[PP.PAIR_S] - mid[PP.PAIR_T], axis=1)
        reach = ln[PP.PAIR_S] + ln[PP.PAIR_T] + 2 * (2 * K.RADIUS + K.MARGIN) + 1e-4
        clear = np.abs(d - reach) > 1e-5 * reach
        got = np.zeros(253, bool); got[idx] = True
        assert np.array_equal(got[clear], (d <= reach)[clear]), c.tag
