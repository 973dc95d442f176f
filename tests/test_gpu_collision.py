"""Collision detection of the peg-in-hole step on the GPU over its whole input domain: the case classes of tests/collision_cases.py, one case
per env, ONE step per launch from set_state with debug = 1, the contact list read back from DBG_CONTACT -- in the fused launch, the
two-launch step and the fused launch without dispatch order (the forms of test_fused_launch_equals_the_two_launch_step).

Against the independent numpy fp64 reference: keys and link pairs identical and in order on the cases that are not sensitive; points,
normals and depths within 8 x the maxima of the fp32 HOST build of the same source (tests/test_collision_domain.py F32_HOST_MAX), the
project's factor for the -ffast-math GPU build against a correctly rounded host build; a sensitive case gets one of its
admissible answers; S_NCONTACT is the reference's count.  All launch forms give the same bits, and a case gets the same bits among cases of
its own class and among cases of every class (light and heavy neighbours in the wavefront's compaction passes and in the dispatch order).

The host wave layer compacts serially: the ballot / popcount compaction over passes of 64 lanes (NSAMP = 123: two passes, 253 pairs: four)
runs only here.

Random-fly: the candidate pass on the cases of collision_cases.fly_cases for both objects, in the quad and the lane layout, with the IK in
controller wavefronts and inside the step wavefront; all four forms give the same bits."""
import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import collision_cases as K
from tests.test_collision_domain import F32_HOST_MAX, F32_HOST_MAX_FLY, _cfg_kw

pytestmark = pytest.mark.gpu
GPU_FACTOR = 8
MAX_ENVS = 512
SCHEDULES = (1, 1 + 8, 0)                                    # fused launch, two-launch step, fused launch with block i = env i


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


def run_gpu(torch, states, cfg, schedule):
    """one step of len(states) <= MAX_ENVS envs from `states` -> (contact rows [n, CMAX, 12], DBG_NCONTACT, S_NCONTACT, S_INVALID) as float32 numpy"""
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    n = len(states)
    assert n <= MAX_ENVS
    g = PihVecEnv(n, seed=5, schedule=schedule, debug=1, **cfg)
    st = g.state().cpu().numpy()
    st[:, :K.WORDS] = np.asarray(states, dtype=np.float32); st[:, _lib.S_CACHE_N] = 0
    g.set_state(torch.tensor(st, dtype=torch.float32))
    g.step(torch.zeros(n, 4))
    d = g.debug().cpu().numpy(); s = g.state().cpu().numpy()
    rows = d[:, _lib.DBG_CONTACT:_lib.DBG_CONTACT + K.CMAX * 12].reshape(n, K.CMAX, 12)
    return rows, d[:, _lib.DBG_NCONTACT].astype(int), s[:, _lib.S_NCONTACT].astype(int), s[:, _lib.S_INVALID]


def _live(rows, cnt):
    """the rows that hold contacts, geometry words only (the multiplier word depends on the solve), as bits; the rest zeroed"""
    out = np.zeros(rows.shape[:2] + (11,), np.int32)
    for e in range(len(rows)):
        out[e, :cnt[e]] = np.ascontiguousarray(rows[e, :cnt[e], :11]).view(np.int32)
    return out


@pytest.mark.parametrize("name", K.CLASSES)
def test_gpu_class_against_the_reference(torch_mod, name):
    cs = K.cases(name)
    tol = tuple(GPU_FACTOR * np.array(F32_HOST_MAX[name])) + (1e-6,)
    worst = np.zeros(3); bad = []
    for key, idx in K.group_by_config(cs).items():
        for lo in range(0, len(idx), MAX_ENVS):
            part = idx[lo:lo + MAX_ENVS]
            first = None
            for sched in SCHEDULES:
                rows, dn, sn, inv = run_gpu(torch_mod, [cs[i].state for i in part], _cfg_kw(key), sched)
                assert (dn == sn).all()
                if first is None:
                    first = (_live(rows, sn), sn)
                    for j, i in enumerate(part):
                        c = cs[i]
                        if not c.sensitive and sn[j] != len(c.kept):
                            bad.append("case %d (%s): %d contacts, reference %d" % (i, c.tag, sn[j], len(c.kept))); continue
                        err, e = K.compare(c, rows[j].astype(np.float64), sn[j], *tol, near_relief=True)
                        if err:
                            bad.append("case %d (%s): %s" % (i, c.tag, err))
                        else:
                            worst = np.maximum(worst, e)
                else:
                    np.testing.assert_array_equal(sn, first[1], err_msg="schedule %d" % sched)
                    np.testing.assert_array_equal(_live(rows, sn), first[0], err_msg="schedule %d" % sched)
    print("   GPU class %s: %d cases, max point %.3e normal %.3e depth %.3e (host fp32 %s); %d failures" % (name, len(cs), *worst, F32_HOST_MAX[name], len(bad)))
    assert not bad, "GPU class %s: %d cases differ from the reference, the first: %s" % (name, len(bad), bad[:5])


def test_gpu_pair_index_map_every_index(torch_mod):
    """idx -> (s, t) with the GPU's approximate square root (the s++ correction never fires on the host): for every one of the 253 indices a
    fold case that holds the pair for certain must show its key with the pair's links"""
    S = K.cases("S")[:3 * len(K.PAIRS)]
    key0 = K.cfg_key(S[0].cfg)
    assert all(K.cfg_key(c.cfg) == key0 for c in S)
    rows = []; cnt = []
    for lo in range(0, len(S), MAX_ENVS):
        r, dn, sn, inv = run_gpu(torch_mod, [c.state for c in S[lo:lo + MAX_ENVS]], _cfg_kw(key0), 1)
        rows.append(r); cnt.append(sn)
    rows = np.concatenate(rows); cnt = np.concatenate(cnt)
    for idx, (s, t) in enumerate(K.PAIRS):
        key = 1000 + s * 24 + t
        held = [3 * idx + v for v in range(3) if any(k.key == key and not k.optional for k in S[3 * idx + v].kept)]
        assert held, "pair index %d = (%d, %d): no case holds it" % (idx, s, t)
        for e in held:
            r = rows[e][:cnt[e]]
            hit = r[r[:, 10] == key]
            assert len(hit) == 1 and (hit[0, 0], hit[0, 1]) == (K.ANL + s, K.ANL + t), "pair index %d = (%d, %d) not emitted as such: keys %s" % (idx, s, t, r[:, 10].astype(int).tolist())


def test_gpu_same_bits_among_own_class_and_among_all(torch_mod):
    """48 cases of each of T, H, F, A, S and C (no scripted grasp) at ONE config (defaults: both arm passes, self collision): a batch per
    class and one shuffled batch of all 288 must give every case the same bits"""
    torch = torch_mod
    rng = np.random.default_rng(17)
    cfg = _cfg_kw(K.cfg_key({}))
    states = {}; single = {}
    for name in ("T", "H", "F", "A", "S", "C"):
        cs = [c for c in K.cases(name) if c.cfg.get("mode", 0) == 0]
        pick = rng.choice(len(cs), 48, replace=False)
        states[name] = np.array([cs[i].state for i in pick])
        rows, dn, sn, inv = run_gpu(torch, states[name], cfg, 1)
        single[name] = (_live(rows, sn), sn)
    allst = np.concatenate([states[n] for n in states]); want_rows = np.concatenate([single[n][0] for n in states]); want_n = np.concatenate([single[n][1] for n in states])
    assert want_n.min() == 0 and want_n.max() == K.CMAX                     # light and heavy envs side by side
    perm = rng.permutation(len(allst))
    rows, dn, sn, inv = run_gpu(torch, allst[perm], cfg, 1)
    np.testing.assert_array_equal(sn, want_n[perm])
    np.testing.assert_array_equal(_live(rows, sn), want_rows[perm])


FLY_SCHEDULES = (1, 1 + 8, 1 + 32, 1 + 8 + 32)             # quad / lane layout, IK in controller wavefronts / inside the step wavefront


@pytest.mark.parametrize("ob", [0, 1])
def test_gpu_fly_candidates_against_the_reference(torch_mod, ob):
    torch = torch_mod
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    cs = K.fly_cases(ob)
    n = len(cs)
    assert n <= MAX_ENVS
    tol = tuple(GPU_FACTOR * np.array(F32_HOST_MAX_FLY[ob]))
    first = None
    for sched in FLY_SCHEDULES:
        g = PihVecEnv(n, task_id=1, seed=5, max_episode_steps=480, contact_margin=K.FLY_MARGIN, schedule=sched, object_id=ob, debug=1)
        st = g.state().cpu().numpy()
        st[:, :K.FLY_WORDS] = np.array([c.state for c in cs], dtype=np.float32)
        g.set_state(torch.tensor(st, dtype=torch.float32))
        g.step(torch.zeros(n, 6))
        d = g.debug().cpu().numpy(); sg = g.state().cpu().numpy()
        cand = d[:, _lib.DBG_FLY_CAND:_lib.DBG_FLY_CAND + K.FNC * 10].reshape(n, K.FNC, 10)
        valid = cand[:, :, 0] != 0
        assert (d[:, _lib.DBG_FLY_NCONTACT] == valid.sum(1)).all() and (sg[:, _lib.F_NCONTACT] == valid.sum(1)).all()
        if first is None:
            first = cand.copy().view(np.int32)
            worst = np.zeros(3); bad = []
            for i, c in enumerate(cs):
                err, e = K.fly_compare(c, cand[i].astype(np.float64), *tol)
                if err:
                    bad.append("case %d (%s): %s" % (i, c.tag, err))
                else:
                    worst = np.maximum(worst, e)
            print("   GPU random-fly object %d: %d cases, max point %.3e normal %.3e depth %.3e (host fp32 %s); %d failures" % (ob, n, *worst, F32_HOST_MAX_FLY[ob], len(bad)))
            assert not bad, "GPU random-fly object %d: %d cases differ from the reference, the first: %s" % (ob, len(bad), bad[:5])
            assert not cand[:, K.OBJ_NSPH[ob]:K.FNS, 0].any() and not cand[:, K.FNS + K.OBJ_NSPH[ob]:2 * K.FNS, 0].any()
        else:
            np.testing.assert_array_equal(cand.view(np.int32), first, err_msg="schedule %d" % sched)
