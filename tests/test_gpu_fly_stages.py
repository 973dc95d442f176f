"""The stages of the random-fly step between collision detection and the tail, on the GPU: the classes, metrics and bounds of
tests/fly_stage_cases.py, which tests/test_fly_stages.py runs on the host builds.  One step per launch from set_state through the C ABI,
at most 512 envs per launch, in the four launch forms of tests/test_gpu_fly.py: one env per quad of lanes or per lane, the IK in
controller wavefronts or inside the step wavefront.

  * free acceleration (DBG_FLY_UDOT, class V), contact rows (N), many contacts (K), limit rows (L) and the motor bound (M) against
    oracle.FlyOracle within GPU_FACTOR x the fp32 host build's MEASURED figures, at 1 / 2 / 5 sweeps and, the well-conditioned env-steps, at 50;
  * per env, on bits: the two forms of a layout agree; an env's post-step record, DBG_FLY_UDOT, candidates and DBG_FLY_LAMBDA do not
    depend on the batch it is stepped in (its own class, a shuffled batch of all classes, ragged batches of 1 .. 257 envs with sentinel rows
    behind obs, reward and done), nor on a neighbour in its wavefront that repeats the solve, has more than KR contacts, is frozen or
    holds a NaN (every case of N, K, L and M, both objects); schedule + 64
    (every limit row, always) gives the same bits; DBG_FLY_LIMIT_ROWS reads 0 / 1 / 2 on wave-uniform blocks.

No file of the reference tree is read here."""
import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import fly_stage_cases as G
from tests import parity_util as P
from tests.test_ik_domain import F32_HOST_MAX_A

pytestmark = pytest.mark.gpu
FORMS = (1, 1 + 8, 1 + 32, 1 + 8 + 32)                      # quad / lane layout, IK in controller wavefronts / inside the step wavefront
IK_TOL = G.GPU_FACTOR * F32_HOST_MAX_A["ur5"][(0.5, 20)]   # F_TARGET: the bound of tests/test_gpu_ik.py's in-step reading
SENTINEL = -7777.25
TAIL = 64
RAGGED = (1, 15, 16, 17, 63, 65, 257)                       # 16 envs per wavefront in the quad layout, 64 in the lane layout


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


def gpu_step(states, actions, ob, iters, sched, tail=False):
    """one step of `states` -> (post-step record float32 [n, 48], debug words float32 [n, DEBUG_WORDS])"""
    n = len(states)
    assert n <= 512
    g = P.GpuProduct(n, task_id=1, seed=5, schedule=sched, debug=1, object_id=ob, solver_iters=iters, **G.CFG)
    g.set_state(states)
    if tail:
        torch = g.torch; dev = g.env.obs.device
        big = [torch.full((n + TAIL, 6), SENTINEL, device=dev), torch.full((n + TAIL,), SENTINEL, device=dev), torch.full((n + TAIL,), 77, dtype=torch.uint8, device=dev)]
        g.env.obs, g.env.reward, g.env.done = big[0][:n], big[1][:n], big[2][:n]
    g.step(actions)
    if tail:
        assert (big[0][n:] == SENTINEL).all() and (big[1][n:] == SENTINEL).all() and (big[2][n:] == 77).all(), "n = %d writes behind the batch" % n
    return g.env.state().cpu().numpy(), g.env.debug().cpu().numpy()


def bits(state, dbg):
    """what an env's step produced, as bits [n, words]: the record, DBG_FLY_UDOT, contact and sweep count, candidates, live multipliers
    (DBG_FLY_LIMIT_ROWS is wavefront-wide by construction and not among them)"""
    lam = dbg[:, _lib.DBG_FLY_LAMBDA:_lib.DBG_FLY_LAMBDA + G.FNC].copy()
    lam[np.arange(G.FNC)[None, :] >= dbg[:, _lib.DBG_FLY_NCONTACT][:, None]] = 0
    w = np.concatenate([state, dbg[:, _lib.DBG_FLY_UDOT:_lib.DBG_FLY_LIMIT_ROWS], dbg[:, _lib.DBG_FLY_CAND:_lib.DBG_FLY_CAND + _lib.DBG_FLY_CAND_STRIDE * G.FNC], lam], 1)
    return np.ascontiguousarray(w, dtype=np.float32).view(np.int32)


_RUN = {}


def class_run(name, ob, iters, sched):
    key = (name, ob, iters, sched)
    if key not in _RUN:
        c = G.cases(name, ob)
        parts = [gpu_step(c.states[lo:lo + 512], c.actions[lo:lo + 512], ob, iters, sched) for lo in range(0, c.n, 512)]
        _RUN[key] = tuple(np.concatenate(x) for x in zip(*parts))
    return _RUN[key]


def _ratios(w, bound):
    return {k: "%.2e = %.2f x" % (v, v / bound[k]) if bound[k] > 0 else "%.1e" % v for k, v in w.items() if k in bound}


@pytest.mark.parametrize("ob", G.OBJECTS)
def test_gpu_free_acceleration_against_the_oracle(torch_mod, oracle_mod, ob):
    runs = {s: class_run("V", ob, 1, s) for s in FORMS}
    for a, b in ((FORMS[0], FORMS[1]), (FORMS[2], FORMS[3])):
        np.testing.assert_array_equal(bits(*runs[a]), bits(*runs[b]), err_msg="schedules %d and %d" % (a, b))
    c = G.cases("V", ob)
    for s in (FORMS[0], FORMS[2]):
        f = G.udot_errors(ob, runs[s][1])
        for k, rate in enumerate(G.RATE_SETS):
            print("   GPU schedule %d object %d rate set %-12s: %s" % (s, ob, rate, {g: "%.2e" % v[c.rate == k].max() for g, v in f.items()}))
        w = G.worst(f, np.ones(c.n, bool))
        print("   GPU schedule %d object %d free acceleration / fp32 host build: %s" % (s, ob, _ratios(w, G.MEASURED["V"])))
        for g, v in w.items():
            assert v <= G.GPU_FACTOR * G.MEASURED["V"][g], (s, g, v)


@pytest.mark.parametrize("ob", G.OBJECTS)
@pytest.mark.parametrize("name", G.STEP_CLASSES)
def test_gpu_rows_and_solve_against_the_oracle(torch_mod, oracle_mod, name, ob):
    """1 / 2 / 5 sweeps: every env, the sensitive ones at SENS_FACTOR x the bound; LONG sweeps: the well-conditioned env-steps"""
    for it in G.SHORT + (G.LONG,):
        long = it == G.LONG
        bound = G.MEASURED[name]["long" if long else "short"]
        runs = {s: class_run(name, ob, it, s) for s in FORMS}
        for a, b in ((FORMS[0], FORMS[1]), (FORMS[2], FORMS[3])):
            np.testing.assert_array_equal(bits(*runs[a]), bits(*runs[b]), err_msg="schedules %d and %d" % (a, b))
        loose = G.ill_conditioned(name, ob) if long else G.reference(name, ob, it).sensitive
        for s in (FORMS[0], FORMS[2]):
            st, dbg = runs[s]
            assert (st[:, _lib.F_INVALID] == 0).all()
            f = G.step_errors(name, ob, it, st, dbg, tag="GPU schedule %d class %s object %d, %d sweeps" % (s, name, ob, it))
            w = G.worst(f, ~loose); ws = G.worst(f, loose)
            print("   GPU schedule %d class %s object %d, %d sweeps / fp32 host build: %s ; target %.2e of %.2e" % (s, name, ob, it, _ratios(w, bound), w["target"], IK_TOL))
            if name == "L":
                e = int(np.argmax(f["qd"])); c = G.cases("L", ob)
                print("      largest qd figure: env %d, joint %d, %s" % (e, c.joint[e], G.L_KINDS[c.kind[e]]))
            assert w["target"] <= IK_TOL
            for k in bound:
                assert w[k] <= G.GPU_FACTOR * bound[k], (s, it, k, w[k])
                if not long:
                    assert ws[k] <= G.SENS_FACTOR * G.GPU_FACTOR * bound[k], (s, it, k, ws[k])


@pytest.mark.parametrize("ob", G.OBJECTS)
def test_gpu_an_envs_bits_do_not_depend_on_its_batch(torch_mod, oracle_mod, ob):
    """every case of N, K, L and M at 5 sweeps keeps the bits it has in a batch of its own class: in a shuffled batch of all classes; in
    ragged batches with sentinel rows behind the outputs; with every second env of the shuffled batch a frozen env or one whose state
    holds a NaN; with every second env a class-L case that fires the verification (the wavefront's solve is repeated) or a class-K case
    with more than KR contacts (ncw > KR: the quad layout's sweep goes on into lane memory)"""
    it = 5
    cs = [G.cases(n, ob) for n in G.STEP_CLASSES]
    states = np.concatenate([c.states for c in cs]); actions = np.concatenate([c.actions for c in cs])
    total = len(states)
    perm = np.random.default_rng(11).permutation(total)
    L = G.cases("L", ob); off = {n: sum(c.n for c in cs[:i]) for i, n in enumerate(G.STEP_CLASSES)}
    fire = off["L"] + np.flatnonzero((L.kind == G.L_KINDS.index("fire")) & (L.joint < 3))
    many = off["K"] + np.flatnonzero(G.reference("K", ob, it).nc > G.KR)
    assert len(fire) >= 8 and (ob == 1 or len(many) >= 30)
    loud = np.concatenate([fire, many]) if len(many) else fire
    for s in FORMS:
        own = np.concatenate([bits(*class_run(n, ob, it, s)) for n in G.STEP_CLASSES])
        for lo in range(0, total, 512):
            part = perm[lo:lo + 512]
            np.testing.assert_array_equal(bits(*gpu_step(states[part], actions[part], ob, it, s)), own[part], err_msg="schedule %d, shuffled" % s)
        for n in RAGGED:
            got = bits(*gpu_step(states[perm[:n]], actions[perm[:n]], ob, it, s, tail=True))
            np.testing.assert_array_equal(got, own[perm[:n]], err_msg="schedule %d, %d envs" % (s, n))
        for lo in range(0, total, 256):
            part = perm[lo:lo + 256]; m = len(part)
            for kind in ("frozen / NaN", "firing / many contacts"):
                st = np.repeat(states[part], 2, 0); ac = np.repeat(actions[part], 2, 0)
                if kind == "frozen / NaN":
                    st[1::4, _lib.F_DONE] = 1.0; st[3::4, _lib.F_Q + (lo // 256) % 6] = np.nan
                else:
                    nb = loud[(lo + np.arange(m)) % len(loud)]
                    st[1::2] = states[nb]; ac[1::2] = actions[nb]
                got_st, got_dbg = gpu_step(st, ac, ob, it, s)
                np.testing.assert_array_equal(bits(got_st, got_dbg)[0::2], own[part], err_msg="schedule %d, neighbours %s" % (s, kind))
                if kind == "frozen / NaN":
                    assert (got_st[3::4, _lib.F_INVALID] == 1).all() and np.isfinite(got_st).all()


def test_gpu_limit_rows_word_neighbours_and_every_row_always(torch_mod, oracle_mod):
    """class L at 5 sweeps.  Four blocks of 64 envs (whole wavefronts in both layouts): every joint far from its limits (word 0); a joint
    inside the band (1); far cases and ONE case that fires the verification (2 in its wavefront: 64 envs of the lane layout, 16 of the
    quad layout -- the solve of those neighbours is repeated); far cases next to a frozen env and an env whose state holds a NaN.  Every
    case keeps the bits it has in a batch of its own class.  schedule + 64 gives the whole class the same bits."""
    ob, it = 0, 5
    c = G.cases("L", ob); kind = c.kind
    far = np.flatnonzero(kind == G.L_KINDS.index("far")); band = np.flatnonzero((kind <= G.L_KINDS.index("beyond")))
    fire = np.flatnonzero((kind == G.L_KINDS.index("fire")) & (c.joint < 3))
    assert len(far) >= 32 and len(band) >= 64 and len(fire) >= 1
    blocks = [np.resize(far, 64), band[:64], np.resize(far, 64).copy(), np.resize(far, 64).copy()]
    blocks[2][0] = fire[0]
    idx = np.concatenate(blocks)
    states = c.states[idx].copy(); actions = c.actions[idx].copy()
    odd = np.arange(192, 256)[1::2]
    states[odd[0::2], _lib.F_DONE] = 1.0                            # frozen neighbours
    states[odd[1::2], _lib.F_Q + 2] = np.nan                        # neighbours with a NaN
    cases = np.setdiff1d(np.arange(256), odd)
    for s in FORMS:
        own = bits(*class_run("L", ob, it, s))
        st, dbg = gpu_step(states, actions, ob, it, s)
        np.testing.assert_array_equal(bits(st, dbg)[cases], own[idx][cases], err_msg="schedule %d" % s)
        assert (st[odd[1::2], _lib.F_INVALID] == 1).all() and np.isfinite(st).all()
        word = dbg[:, _lib.DBG_FLY_LIMIT_ROWS]
        wave = 64 if s & 32 else 16
        assert (word[:64] == 0).all() and (word[64:128] == 1).all(), (s, word[:128])
        assert (word[128:128 + wave] == 2).all() and (word[128 + wave:192] == 0).all(), (s, word[128:192])
        full = bits(*gpu_step(c.states, c.actions, ob, it, s + 64))
        np.testing.assert_array_equal(full, own, err_msg="schedule %d + 64" % s)
