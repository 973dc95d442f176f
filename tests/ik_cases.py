"""Seeded inverse-kinematics problems over the whole input domain of calculateInverseKinematics (envs/utils.py:67,79), shared by the
host-build tests (tests/test_ik_domain.py) and the GPU tests (tests/test_gpu_ik.py).

The reference is the fp64 oracle (oracle.ik / oracle.ik_ur5 with a config).  Every input (q0, tpos, tquat, and the float fields of the
config) is rounded to fp32 BEFORE it goes to the oracle, so both sides see the same numbers; the oracle gets the rounded quaternion
normalised in double (see ref_ik).  Everything here is a property of the inputs and of the oracle alone: nothing looks
at the product.

  A  arithmetic      ik_residual = 0 (no discrete branch).  Start poses over the full joint range (UR5: +-2 pi, every fourth block of eight
                     cases +-20 rad; Panda: the joint limits of include/pih_model.h), target = oracle FK(q0) displaced by U(-s, s)^3 with
                     s = 0 / 0.02 / 0.3 / 2.0 m (2.0 m is out of reach: the 30-degree clamp acts on every iteration) and turned by
                     0..170 degrees about a random axis; every other case passes -tquat.  >= 40 start poses per m_to_q branch.
  B  fixed point     target = oracle FK(q0) exactly: the exit test fires in iteration 0, q* = q0 bit for bit.
  C  exit in loop    default ik_residual, displacement log-uniform in [1.2e-4, 2e-3] m, zero orientation error.  The oracle alone says which
                     cases exit in mid-loop (result differs from ik_residual = 0) and which are threshold-sensitive (results at 0.98 x and
                     1.02 x ik_residual differ: the fp32 FK error of 2-5e-7 m is 0.2-0.5 % of the threshold, the band is four times that).
  D  sign symmetry   the class A problems at the default config with tquat AND with -tquat: the two results agree.
"""
import functools

import numpy as np

from tests.render_ref import macro as _macro          # the one reader of include/pih_model.h

CHAINS = ("ur5", "panda")
DEFAULT = (0.5, 20)                                                      # (ik_damping, ik_iters) of pih_default_config
CONFIGS_A = ((0.5, 20), (0.5, 1), (0.5, 50), (0.05, 1), (0.05, 3))       # low damping for few iterations only: at (0.05, 50) the fp64 oracle itself amplifies 1e-12 to 6e-7
RESIDUAL = 1e-4                                                          # ik_residual of pih_default_config
SCALES = (0.0, 0.02, 0.3, 2.0)
N_A, N_B, N_C = 250, 400, 400
# seeds of numpy.random.default_rng (class A: the first seed per chain whose start poses put >= 45 of 250 into every m_to_q branch)
SEEDS = {("ur5", "A"): 6, ("panda", "A"): 0, ("ur5", "B"): 2, ("panda", "B"): 3, ("ur5", "C"): 4, ("panda", "C"): 5}
ARM = {"ur5": 6, "panda": 7}                                             # joints the IK moves
WORDS = {"ur5": 6, "panda": 9}                                           # words of a pih_ik_ur5 / pih_ik problem (Panda: + two finger entries)
FINGER = 0.02


def f32(x):
    """rounded to fp32, kept as float64 (what the oracle and the host builds take)"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def fk(O, chain, q):
    return O.fk_ur5(q, 6) if chain == "ur5" else O.fk_arm(q, 9)


def ref_ik(O, chain, q0, tpos, tquat, damping=DEFAULT[0], iters=DEFAULT[1], residual=RESIDUAL):
    # (pih_config holds floats: the oracle gets the numbers the product gets)
    cfg = O.default_config(ik_damping=float(np.float32(damping)), ik_iters=iters, ik_residual=float(np.float32(residual)))
    # the oracle restates Bullet's 2 acos(w), which wants a UNIT quaternion (oracle/pih_oracle.c ik_rot_error): the orientation that the
    # fp32 numbers denote, normalised in double.  The product's angle and axis do not depend on the norm.
    tquat = np.asarray(tquat, dtype=np.float64)
    return (O.ik_ur5 if chain == "ur5" else O.ik)(q0, tpos, tquat / np.linalg.norm(tquat), cfg)


def ref_batch(O, chain, q0, tpos, tquat, **kw):
    return np.array([ref_ik(O, chain, q0[i], tpos[i], tquat[i], **kw) for i in range(len(q0))])


def q_mul(a, b):
    """quaternion product, (x, y, z, w)"""
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                     [2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w],
                     [2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]])


def m_to_q_branch(R):
    """which of the four branches of m_to_q (pih_math.h) a rotation takes: 0 trace > 0, else 1 / 2 / 3 = largest diagonal entry xx / yy / zz"""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        return 1
    return 2 if R[1, 1] > R[2, 2] else 3


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def start_poses(rng, chain, n):
    """[n, WORDS] fp32-valued start poses over the full range of the chain"""
    if chain == "ur5":
        q = rng.uniform(-2 * np.pi, 2 * np.pi, (n, 6))
        wide = (np.arange(n) // 8) % 4 == 0                   # "a few tens of radians" (sincos_joint, pih_math.h)
        q[wide] = rng.uniform(-20, 20, (int(wide.sum()), 6))
        return f32(q)
    lo, hi = _macro("PIH_LINK_LO")[:7], _macro("PIH_LINK_HI")[:7]
    q = np.full((n, 9), FINGER)
    q[:, :7] = rng.uniform(lo, hi, (n, 7))
    return f32(q)


@functools.lru_cache(maxsize=None)
def _class_a(chain):
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(SEEDS[chain, "A"])
    q0 = start_poses(rng, chain, N_A)
    tpos = np.zeros((N_A, 3)); tquat = np.zeros((N_A, 4)); branch = np.zeros(N_A, int)
    idx = np.arange(N_A)
    neg = idx % 2 == 1; scale = np.array(SCALES)[(idx // 2) % 4]
    for i in range(N_A):
        p, qe = fk(O, chain, q0[i])
        branch[i] = m_to_q_branch(quat_to_R(qe))
        ang = np.deg2rad(rng.uniform(0, 170)); ax = _unit(rng)         # (not up to 180: the axis of a half turn is undefined in any precision)
        tq = q_mul(np.concatenate([np.sin(ang / 2) * ax, [np.cos(ang / 2)]]), qe)
        tquat[i] = (-1 if neg[i] else 1) * tq / np.linalg.norm(tq)
        tpos[i] = p + rng.uniform(-1, 1, 3) * scale[i]
    counts = np.bincount(branch, minlength=4)
    assert counts.min() >= 40, "m_to_q branches of the %s start poses: %s" % (chain, counts)
    out = dict(q0=q0, tpos=f32(tpos), tquat=f32(tquat), neg=neg, scale=scale, branch=branch)
    for a in out.values():
        a.setflags(write=False)
    return out


def class_a(chain):
    """dict q0 [250, WORDS], tpos, tquat (fp32-valued), neg (passes -tquat), scale [m], branch (m_to_q branch of the start pose)"""
    return _class_a(chain)


@functools.lru_cache(maxsize=None)
def _class_b(chain):
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(SEEDS[chain, "B"])
    q0 = start_poses(rng, chain, N_B)
    pq = [fk(O, chain, q) for q in q0]
    out = dict(q0=q0, tpos=f32([x[0] for x in pq]), tquat=f32([x[1] for x in pq]))
    for a in out.values():
        a.setflags(write=False)
    return out


def class_b(chain):
    return _class_b(chain)


@functools.lru_cache(maxsize=None)
def _class_c(chain):
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(SEEDS[chain, "C"])
    q0 = start_poses(rng, chain, N_C)
    pq = [fk(O, chain, q) for q in q0]
    disp = np.exp(rng.uniform(np.log(1.2e-4), np.log(2e-3), N_C))
    tpos = f32([pq[i][0] + disp[i] * _unit(rng) for i in range(N_C)]); tquat = f32([x[1] for x in pq])
    ref = ref_batch(O, chain, q0, tpos, tquat)
    free = ref_batch(O, chain, q0, tpos, tquat, residual=0.0)
    lo = ref_batch(O, chain, q0, tpos, tquat, residual=0.98 * RESIDUAL); hi = ref_batch(O, chain, q0, tpos, tquat, residual=1.02 * RESIDUAL)
    exits = np.abs(ref - free).max(1) > 0
    band = np.abs(lo - hi).max(1)
    assert exits.mean() >= 0.30, "class C %s: only %.0f %% of the cases exit in mid-loop" % (chain, 100 * exits.mean())
    assert (band > 0).mean() <= 0.30, "class C %s: %.0f %% of the cases are threshold-sensitive" % (chain, 100 * (band > 0).mean())
    out = dict(q0=q0, tpos=tpos, tquat=tquat, ref=ref, exits=exits, band=band)
    for a in out.values():
        a.setflags(write=False)
    return out


def class_c(chain):
    """as class_a plus ref (the oracle at the default config), exits (bool), band (|oracle at 0.98 x - at 1.02 x ik_residual|, 0 = not sensitive)"""
    return _class_c(chain)


def class_c_bound(case, tol):
    """per-case bound: the class tolerance, or for a threshold-sensitive case twice what the oracle's own two band runs differ by"""
    return np.maximum(tol, 2 * case["band"])


@functools.lru_cache(maxsize=None)
def _ref_a(chain, cfg):
    from oracle import oracle as O
    A = class_a(chain)
    r = ref_batch(O, chain, A["q0"], A["tpos"], A["tquat"], damping=cfg[0], iters=cfg[1], residual=0.0)
    r.setflags(write=False)
    return r


def ref_a(chain, cfg=DEFAULT):
    """the oracle's answers to class A at (ik_damping, ik_iters), ik_residual = 0 (computed once)"""
    return _ref_a(chain, tuple(cfg))


def class_d(chain):
    """class A twice: rows [0, 250) as generated, rows [250, 500) with the target quaternion negated"""
    A = class_a(chain)
    return dict(q0=np.concatenate([A["q0"], A["q0"]]), tpos=np.concatenate([A["tpos"], A["tpos"]]), tquat=np.concatenate([A["tquat"], -A["tquat"]]))
