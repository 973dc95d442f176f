"""What tests/test_gpu_collision_bits.py compares and tests/golden/make_collision_bits_golden.py records: every case of
tests/collision_cases.py (classes T H F A S C M), grouped by config, at most 512 envs per launch, ONE step each from set_state at
schedule 1 with debug = 1.  Per case: S_NCONTACT, the number of live contacts that involve the arm (the contacts the cap CAMAX counts:
attach, weld, arm spheres, pads; read off the keys), which of the samples 63, 64 and 122 gave a contact (bits 0, 1, 2), and a 64-bit
digest of the live contact rows' 11 geometry words (links, point, normal, depth, mu, key -- in slot order, so order is part of it)."""
import hashlib

import numpy as np

from peg_in_hole_gym_amd import _lib
from tests import collision_cases as K
from tests.test_collision_domain import _cfg_kw

MAX_ENVS = 512
SCHEDULE = 1
WATCHED_SAMPLES = (63, 64, 122)


def sample_of_key(key):
    """pipe sample a contact key belongs to, or -1 (pairs, attach, weld, arm spheres against the table)"""
    if key < 100:
        return int(K.VERT_SAMPLE[key])                           # table: key = vertex ordinal
    if key < 100 + K.NSAMP:
        return key - 100                                         # tube
    if 300 <= key < 300 + 2 * K.NSAMP:
        return (key - 300) % K.NSAMP                             # pads
    if key >= 5000:
        return (key - 5000) % K.NSAMP                            # arm spheres against the pipe
    return -1


def arm_key(key):
    return key in (2000, 2001) or 300 <= key < 300 + 2 * K.NSAMP or key >= 3000


def summarize(rows, n):
    """(arm-involving live contacts, watched-sample bits, digest) of one case's live rows [n, 12] (float32)"""
    live = np.ascontiguousarray(rows[:n, :11], dtype=np.float32)
    keys = live[:, 10].astype(int).tolist()
    bits = 0
    for b, s in enumerate(WATCHED_SAMPLES):
        if any(sample_of_key(k) == s for k in keys):
            bits |= 1 << b
    return sum(arm_key(k) for k in keys), bits, hashlib.blake2b(live.tobytes(), digest_size=8).hexdigest()


def record(torch):
    """-> {class: {"n": [...], "arm": [...], "samples": [...], "digest": [...]}} of this build, case order of collision_cases.cases"""
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    out = {}
    for name in K.CLASSES:
        cs = K.cases(name)
        cnt = [0] * len(cs); arm = [0] * len(cs); smp = [0] * len(cs); dig = [""] * len(cs)
        for key, idx in K.group_by_config(cs).items():
            for lo in range(0, len(idx), MAX_ENVS):
                part = idx[lo:lo + MAX_ENVS]
                g = PihVecEnv(len(part), seed=5, schedule=SCHEDULE, debug=1, **_cfg_kw(key))
                st = g.state().cpu().numpy()
                st[:, :K.WORDS] = np.asarray([cs[i].state for i in part], dtype=np.float32); st[:, _lib.S_CACHE_N] = 0
                g.set_state(torch.tensor(st, dtype=torch.float32))
                g.step(torch.zeros(len(part), 4))
                d = g.debug().cpu().numpy(); s = g.state().cpu().numpy()
                rows = d[:, _lib.DBG_CONTACT:_lib.DBG_CONTACT + K.CMAX * 12].reshape(len(part), K.CMAX, 12)
                for j, i in enumerate(part):
                    cnt[i] = int(s[j, _lib.S_NCONTACT])
                    arm[i], smp[i], dig[i] = summarize(rows[j], cnt[i])
        out[name] = {"n": cnt, "arm": arm, "samples": smp, "digest": dig}
    return out
