"""Cases for the pipe's self-collision pass (collide(), pih_wave.h: per-segment broad phase, one compacted narrow phase), built with the
helpers of tests/collision_cases.py, shared by tests/test_pair_pass.py (host) and tests/test_gpu_pair_pass.py (GPU, against
tests/golden/pair_pass_bits.json).

The pass filters its 253 segment pairs by a predicate on 24 per-segment records (m = p + q, len = |q - p|): a pair survives when
|m_s - m_t|^2 <= (len_s + len_t + 2 (2 r + margin) + 1e-4)^2.  The survivors go, in pair-index order, into ONE list that the narrow phase
walks 64 entries at a time.  What can go wrong there depends on HOW MANY pairs survive (list lengths around 64, 128, 192, the full 253),
WHERE in the list the pairs that emit a contact sit (the last entry of a round of 64, the first of the next), and which pair indices
emit (the old chunk boundaries).  survivors() is a numpy fp32 replica of the predicate; coverage() counts what the case set holds, and
the tests assert it on the set itself.

A fan of k folded joints (collision_cases._zigzag) has k (k + 1) / 2 pairs in reach; counts in between come from a second small fan and
jittered joints, found by the seeded search below (on the host; nothing here touches the GPU)."""
import functools

import numpy as np

from tests import collision_cases as K

MAX_ENVS = 512
SCHEDULE = 1
CFG = dict(armcol=0, selfcol=1)
SEED = 211
PAIR_S = np.array([s for s, t in K.PAIRS]); PAIR_T = np.array([t for s, t in K.PAIRS])
BOUNDARY_PAIRS = (63, 64, 127, 128, 191, 192, 252)                 # last / first pair index of the old chunks of 64, and the last pair


def vertices32(state):
    """the 25 pipe vertices of a state, rounded to fp32 (the sample positions the pass reads)"""
    R, o = K.fk(np.asarray(state, dtype=np.float64))
    return K.samples(R, o)[K.VERT_SAMPLE].astype(np.float32)


def survivors(state, margin=K.MARGIN, v=None):
    """numpy fp32 replica of the per-segment broad phase -> sorted pair indices that survive, and the least relative distance of any pair
    from the threshold (how far the count is from depending on rounding)"""
    v = vertices32(state) if v is None else v
    f = np.float32
    m = v[:-1] + v[1:]
    d = v[1:] - v[:-1]
    ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], dtype=np.float32)
    dm = m[PAIR_S] - m[PAIR_T]
    d2 = dm[:, 0] * dm[:, 0] + dm[:, 1] * dm[:, 1] + dm[:, 2] * dm[:, 2]
    reach = ln[PAIR_S] + ln[PAIR_T] + f(2) * (f(2) * f(K.RADIUS) + f(margin)) + f(1e-4)
    r2 = reach * reach
    assert d2.dtype == np.float32 and r2.dtype == np.float32
    return np.flatnonzero(d2 <= r2), float(np.min(np.abs(d2 - r2) / r2))


def emitters(case, kept_only=False):
    """pair indices of the self-collision contacts of a case's reference (every candidate, or those that survive the caps)"""
    lst = [c for c in case.kept if 1000 <= c.key < 2000] if kept_only else case.passes[-1]
    return [K.PAIR_INDEX[c.key] for c in lst]


def _fan_state(rng, fans, jitter=0.0, Rroot=None, at=None):
    """a pipe with the given fans (j0, k, delta) folded in, every joint turned by up to `jitter` more, parked away from everything"""
    qj = np.zeros(23)
    for j0, k, delta in fans:
        qj[j0:j0 + k] = K._zigzag(j0, k, delta)[j0:j0 + k]
    if jitter:
        qj += rng.uniform(-jitter, jitter, 23)
    return K.place_pipe(K.base_state(), 0, K.FAR if at is None else at, K._rand_R(rng) if Rroot is None else Rroot, qj)


def _count_search(rng, want, tries=4000):
    """states whose survivor count is exactly each of `want` (and not within 1e-3 of changing): a fan of 10 or 11 joints, a second small fan
    behind it, jittered joints"""
    found = {}
    for _ in range(tries):
        if len(found) == len(want):
            break
        k1 = int(rng.integers(9, 12)); k2 = int(rng.integers(1, 6)); j2 = k1 + 2 + int(rng.integers(0, 23 - k1 - 2 - k2 + 1))
        s = _fan_state(rng, [(0, k1, rng.uniform(0.05, 0.3)), (j2, k2, rng.uniform(0.05, 0.3))], jitter=rng.choice([0.0, 0.02, 0.1]))
        idx, clear = survivors(K.f32(s))
        if len(idx) in want and len(idx) not in found and clear > 1e-3:
            found[len(idx)] = s
    return found


def _one_search(rng, tries=400):
    """exactly one survivor: the first two joints of the pipe bent until segments 0 and 2 are in reach and nothing else is"""
    for _ in range(tries):
        qj = np.zeros(23); qj[0] = rng.uniform(0.5, 2.5); qj[1] = rng.uniform(0.5, 2.5)
        s = K.place_pipe(K.base_state(), 0, K.FAR, K._rand_R(rng), qj)
        idx, clear = survivors(K.f32(s))
        if len(idx) == 1 and clear > 1e-3:
            return s
    return None


def _straddle_search(rng, tries=600):
    """a state whose list entries 63 and 64 (the last of the first narrow round, the first of the second) both emit a contact that is kept:
    a LOOSE fan in front (in reach of each other, not in contact) fills the list, a tight one behind it emits"""
    for _ in range(tries):
        k1 = int(rng.integers(10, 13)); k2 = int(rng.integers(2, 7)); j2 = k1 + 2 + int(rng.integers(0, 23 - k1 - 2 - k2 + 1))
        s = _fan_state(rng, [(0, k1, rng.uniform(0.5, 1.3)), (j2, k2, rng.uniform(0.03, 0.2))], jitter=rng.choice([0.0, 0.05]))
        idx, clear = survivors(K.f32(s))
        if len(idx) < 66 or clear < 1e-3:
            continue
        c = K.Case(s, CFG, "P:straddle")
        kept = set(emitters(c, True))
        if int(idx[63]) in kept and int(idx[64]) in kept:
            return c
    return None


def _cap_search(rng, tries=200):
    """table contacts in front, then more pairs than the slots that are left: CMAX is reached inside the pair pass and the tail is dropped"""
    for _ in range(tries):
        ax = rng.normal(size=2); ax = np.array([ax[0], ax[1], 0]) / np.hypot(*ax)
        Rr = K.rot_axis(ax, rng.uniform(0.1, 0.5)) @ K._rand_R(rng)
        s = _fan_state(rng, [(int(rng.integers(0, 6)), 14, rng.uniform(0.06, 0.2))], Rroot=Rr, at=np.array([2.0, 2.0, 0.5]))
        R, o = K.fk(K.f32(np.concatenate([s, np.zeros(K.STATE_WORDS - len(s))])))
        z = np.sort(K.samples(R, o)[K.VERT_SAMPLE, 2])
        T = int(rng.integers(3, 12))
        s[K.S_POS + 2] += K.TABLE_Z + K.RADIUS + K.MARGIN - 0.5 * (z[T] + z[T - 1])
        c = K.Case(s, CFG, "P:cap")
        npair = len(c.passes[-1])
        if len(c.passes[0]) == T and len(c.passes[1]) == 0 and T + npair > K.CMAX and len(emitters(c, True)) == K.CMAX - T:
            return c
    return None


@functools.lru_cache(maxsize=None)
def cases():
    """the committed cases (computed once, with their reference); the LAST one is the 253-survivor case again with selfcol = 0"""
    rng = np.random.default_rng(SEED)
    out = []
    out.append(K.Case(_fan_state(rng, []), CFG, "P:straight"))                                       # 0 survivors
    for k in range(1, 24):                                                                           # fans of every size, three tightnesses
        for delta in (0.06, 0.15, 0.4):
            j0 = int(rng.integers(0, 23 - k + 1))
            out.append(K.Case(_fan_state(rng, [(j0, k, delta)], jitter=(0.0, 0.03)[k % 2]), CFG, "P:fan%d" % k))
    out.append(K.Case(_fan_state(rng, [(0, 23, 0.03)]), CFG, "P:all"))                               # the whole pipe one bundle: all 253
    full = out[-1]
    s = _one_search(rng)
    if s is not None:
        out.append(K.Case(s, CFG, "P:count1"))
    for n, s in sorted(_count_search(rng, (63, 64, 65)).items()):
        out.append(K.Case(s, CFG, "P:count%d" % n))
    c = _straddle_search(rng)
    if c is not None:
        out.append(c)
    c = _cap_search(rng)
    if c is not None:
        out.append(c)
    for idx in BOUNDARY_PAIRS:                                                                       # the pairs at the old chunk boundaries, folded into contact
        s, t = K.PAIRS[idx]
        for v in range(2):
            gap = 2 * K.RADIUS + rng.uniform(-0.006, K.MARGIN - 0.0005)
            out.append(K.Case(K.place_pipe(K.base_state(), 0, K.FAR, K._rand_R(rng), K.fold_joints(s, t, gap, rng, jitter=(0.0, 0.03)[v])), CFG, "P:pair%d" % idx))
    while len(out) < 299:                                                                            # two fans and jitter: counts and list positions all over
        k1 = int(rng.integers(1, 16)); k2 = int(rng.integers(1, 23 - k1 - 1)); j2 = k1 + 2 + int(rng.integers(0, 23 - k1 - 2 - k2 + 1))
        s = _fan_state(rng, [(0, k1, np.exp(rng.uniform(np.log(0.03), np.log(1.2)))), (j2, k2, np.exp(rng.uniform(np.log(0.03), np.log(1.2))))], jitter=rng.choice([0.0, 0.03, 0.3]))
        out.append(K.Case(s, CFG, "P:two-fans"))
    out.append(K.Case(full.state, dict(armcol=0, selfcol=0), "P:all-selfcol0"))
    return tuple(out)


def coverage(cs):
    """what the case set holds, from the fp32 predicate and the reference alone"""
    cov = dict(counts=[], straddle=0, cap=0, emit_idx=set(), selfcol0_full=0)
    for c in cs:
        idx, _ = survivors(c.state, c.cfg.get("margin", K.MARGIN))
        n = len(idx)
        if not c.cfg["selfcol"]:
            cov["selfcol0_full"] += n == 253 and not c.passes[-1]
            continue
        cov["counts"].append(n)
        kept = set(emitters(c, True))
        cov["emit_idx"] |= kept
        if n >= 65 and int(idx[63]) in kept and int(idx[64]) in kept:
            cov["straddle"] += 1
        T = len(c.passes[0])
        if T >= 1 and c.ncand > K.CMAX and len(c.kept) == K.CMAX and 0 < len(kept) < len(c.passes[-1]) and c.kept[-1].key >= 1000:
            cov["cap"] += 1
    return cov


def random_states(n=2000, seed=212):
    """random folded and random-joint pipe states (host test only): -> float32 [n, WORDS]"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 2:
            s, t = K.PAIRS[int(rng.integers(0, 253))]
            qj = K.fold_joints(s, t, 2 * K.RADIUS + rng.uniform(-0.006, K.MARGIN + 0.004), rng, jitter=rng.choice([0.0, 0.03, 0.25]))
            if i % 4 == 3:
                qj += rng.uniform(-0.3, 0.3, 23)
        else:
            qj = rng.uniform(-1, 1, 23) * np.exp(rng.uniform(np.log(0.05), np.log(3.1)))
        out.append(K.f32(K.place_pipe(K.base_state(), 0, K.FAR, K._rand_R(rng), qj)))
    return np.asarray(out, dtype=np.float32)


def self_emitters(state, margin=K.MARGIN):
    """pair indices of every self-collision contact collision_cases.reference emits for a state (optional ones included)"""
    return [K.PAIR_INDEX[c.key] for c in K.reference(np.asarray(state, dtype=np.float64), armcol=0, selfcol=1, margin=margin)[-1]]


def record(torch):
    """-> {"n": [...], "arm": [...], "digest": [...]} of this build, case order of cases(): one step from set_state per config group"""
    from peg_in_hole_gym_amd import _lib
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    from tests.collision_bits_run import summarize
    from tests.test_collision_domain import _cfg_kw
    cs = cases()
    cnt = [0] * len(cs); arm = [0] * len(cs); dig = [""] * len(cs)
    for key, part in K.group_by_config(cs).items():
        assert len(part) <= MAX_ENVS
        g = PihVecEnv(len(part), seed=5, schedule=SCHEDULE, debug=1, **_cfg_kw(key))
        st = g.state().cpu().numpy()
        st[:, :K.WORDS] = np.asarray([cs[i].state for i in part], dtype=np.float32); st[:, _lib.S_CACHE_N] = 0
        g.set_state(torch.tensor(st, dtype=torch.float32))
        g.step(torch.zeros(len(part), 4))
        d = g.debug().cpu().numpy(); s = g.state().cpu().numpy()
        rows = d[:, _lib.DBG_CONTACT:_lib.DBG_CONTACT + K.CMAX * 12].reshape(len(part), K.CMAX, 12)
        for j, i in enumerate(part):
            cnt[i] = int(s[j, _lib.S_NCONTACT])
            arm[i], _, dig[i] = summarize(rows[j], cnt[i])
    return {"n": cnt, "arm": arm, "digest": dig}
