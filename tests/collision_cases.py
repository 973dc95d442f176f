"""Seeded collision-detection cases over the whole input domain of collide() (csrc/pih_common.h) and an INDEPENDENT numpy fp64 reference
of the contact list, shared by the host tests (tests/test_collision_domain.py) and the GPU tests (tests/test_gpu_collision.py).

Nothing here restates the product's arithmetic: the forward kinematics is a generic walk over the link tables of include/pih_model.h, the
geometry comes from the definitions --

  point - tube     distance to the rectangle [-hl, hl] x [Rin, Rout] in (axial, radial) by projection; inside, the nearest of its four edges
  point - box      projection onto the box in its own frame; inside, the nearest of its six faces
  segment - segment  the least of the four end-point-to-segment distances and of the common perpendicular when both of its feet lie inside
                   (the product walks Ericson's clamp chain)

-- and the caps are applied to the finished candidate lists (passes in key order, CAMAX arm-involving contacts, CMAX in all, the tail of
a pass dropped first).  reference_geometry_check() holds the three primitives against brute-force minimisation (scipy).

A case is a state record (the 98 physical words, and ATTACH_QZ behind them), rounded to fp32 BEFORE anybody sees it, plus the config
fields that collision reads (mode, contact_margin, enable_arm_collision, enable_self_collision).  Only the contact list of the one step
from that state is read.

Where the answer is discontinuous in the input the reference says so instead of guessing: a candidate carries every admissible
(point, normal, depth) and may be `optional` (a depth within 1e-5 of the margin); a case with such a candidate is `sensitive`.  The
discontinuities: depth ~ margin, |dx - dy| < 1e-6 inside the tube wall, two box faces equally near, parallel segments (the closest pair
is a set), and a sample within 1e-4 of the tube axis (the radial direction is noise: only the axial parts are compared).

Classes (each generator reports, from the reference alone, how many contacts land in each branch; FLOORS are asserted by the tests):
  T table   H tube   F pad boxes   A arm spheres   S self collision (all 253 keys)   C caps   M margin 0.02 / 0.006
and, at the end of the file, the candidate pass of the random-fly task (sphere against capsule, sphere and capsule ends against the table).
"""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 128                                                    # a case: the 98 physical words of the state record, and behind them the derived words (ATTACH_QZ is word 113)
S_QARM, S_POS, S_QUAT, S_QJ, S_TARGET, S_FSM, S_FSMT, S_GRASP, S_RANDY, S_ATTACH_QZ = 0, 18, 21, 31, 77, 86, 87, 89, 90, 113
STATE_WORDS = 128
CMAX, CAMAX, MAX_FRICTION = 48, 12, 10.0
MARGIN = float(np.float32(0.005))                              # contact_margin of pih_default_config, as the float it is
EDGE = 1e-5                                                    # a depth this close to the margin may fall on either side
TIE = 1e-6
AXIS_EPS = 1e-4
# segments parallel "within 1e-6" still enclose up to 1e-6 rad: the closest pairs of the set differ by that much in normal and depth / length
PARALLEL_SLACK = 1e-5
# the generators keep a TARGETED sample at least this far off a surface it is outside of: the normal there is (x - foot) / distance, whose
# error is the position error over the distance (the other samples of the pipe fall where they fall)
NEAR = 1e-3


def _macro(name):
    hdr = open(os.path.join(ROOT, "include", "pih_model.h")).read()
    body = re.search(r"#define %s (.*)" % name, hdr).group(1).split("/*")[0]
    return np.array(eval(body.replace("{", "[").replace("}", "]")), dtype=float)


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


ANL, NL, NSAMP = 9, 33, 123
PARENT = _macro("PIH_LINK_PARENT").astype(int); JTYPE = _macro("PIH_LINK_JTYPE").astype(int)
RFIX = _macro("PIH_LINK_RFIX").reshape(NL, 3, 3); TFIX = _macro("PIH_LINK_TFIX"); AXIS = _macro("PIH_LINK_AXIS")
LINK_MU = _macro("PIH_LINK_MU"); LINK_LO = _macro("PIH_LINK_LO"); LINK_HI = _macro("PIH_LINK_HI")
BASE_R = _macro("PIH_ARM_BASE_R").reshape(3, 3)
EE_PARENT = int(_macro("PIH_EE_PARENT")); EE_R = _macro("PIH_EE_R").reshape(3, 3); EE_T = _macro("PIH_EE_T")
ARM_REST = _macro("PIH_ARM_REST")
BOX_C = _macro("PIH_FINGER_BOX_C"); BOX_H = _macro("PIH_FINGER_BOX_H"); FINGER0 = int(_macro("PIH_FINGER_LINK0"))
NSPH = int(_macro("PIH_ARM_NSPH")); SPH_LINK = _macro("PIH_ARM_SPH_LINK").astype(int); SPH_C = _macro("PIH_ARM_SPH_C"); SPH_R = _macro("PIH_ARM_SPH_R")
PIPE_SPH0 = int(_macro("PIH_ARM_PIPE_SPH0"))
RADIUS = float(_macro("PIH_PIPE_RADIUS"))
SAMP_LINK = _macro("PIH_PIPE_SAMP_LINK").astype(int); SAMP_Y = _macro("PIH_PIPE_SAMP_Y"); SAMP_VERTEX = _macro("PIH_PIPE_SAMP_VERTEX").astype(bool)
TABLE_Z = float(eval(re.search(r"#define PIH_TABLE_Z (\S+)", open(os.path.join(ROOT, "include", "pih_model.h")).read()).group(1)))
TABLE_MU = float(_macro("PIH_TABLE_MU")); HOLE_MU = float(_macro("PIH_HOLE_MU"))
HOLE_POS = _macro("PIH_HOLE_POS"); HOLE_HL = float(_macro("PIH_HOLE_HALFLEN")); RIN = float(_macro("PIH_HOLE_RIN")); ROUT = float(_macro("PIH_HOLE_ROUT"))
VERT_SAMPLE = np.flatnonzero(SAMP_VERTEX)                      # sample index of vertex v (25 vertices: 24 segments)
PAIRS = [(s, t) for s in range(24) for t in range(s + 2, 24)]  # the 253 self-collision pairs in key order
UR5_RFIX = _macro("PIH_UR5_RFIX").reshape(6, 3, 3); UR5_TFIX = _macro("PIH_UR5_TFIX"); UR5_AXIS = _macro("PIH_UR5_AXIS")
UR5_BASE_T = _macro("PIH_UR5_BASE_T"); UR5_EE_R = _macro("PIH_UR5_EE_R").reshape(3, 3); UR5_EE_T = _macro("PIH_UR5_EE_T")


# ------------------------------------------------------------------------------------------------ kinematics
def rot_axis(axis, th):
    """rotation by th about a unit axis, as the matrix exponential of its cross-product matrix"""
    x, y, z = axis
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def quat_to_R(q):
    """(x, y, z, w) -> matrix, the homogeneous form: what an almost-unit fp32 quaternion denotes in every build"""
    x, y, z, w = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                     [2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w],
                     [2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]])


def R_to_quat(R):
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(R).as_quat()


def chain_fk(parent, jtype, rfix, tfix, axis, q, base_R=np.eye(3), base_t=np.zeros(3), floating=None):
    """generic tree walk: link frame = parent frame * (RFIX, TFIX) * joint(q).  -> R [n, 3, 3], o [n, 3]"""
    n = len(parent)
    R = np.zeros((n, 3, 3)); o = np.zeros((n, 3))
    for L in range(n):
        if jtype[L] == 2:
            R[L], o[L] = floating
            continue
        Rp, op = (base_R, base_t) if parent[L] < 0 else (R[parent[L]], o[parent[L]])
        Rj = Rp @ rfix[L]; oj = op + Rp @ tfix[L]
        if jtype[L] == 0:
            R[L] = Rj @ rot_axis(axis[L], q[L]); o[L] = oj
        else:
            R[L] = Rj; o[L] = oj + q[L] * (Rj @ axis[L])
    return R, o


def fk(state):
    """link frames of the peg-in-hole world (9 arm links, 24 pipe links) from a state record"""
    q = np.zeros(NL)
    q[:ANL] = state[S_QARM:S_QARM + ANL]; q[ANL + 1:] = state[S_QJ:S_QJ + 23]
    return chain_fk(PARENT, JTYPE, RFIX, TFIX, AXIS, q, BASE_R, np.zeros(3), (quat_to_R(state[S_QUAT:S_QUAT + 4]), state[S_POS:S_POS + 3]))


def fk_ur5(q):
    """-> R [6, 3, 3], o [6, 3], ee position, ee rotation"""
    R, o = chain_fk(np.arange(-1, 5), np.zeros(6, int), UR5_RFIX, UR5_TFIX, UR5_AXIS, q, np.eye(3), UR5_BASE_T)
    return R, o, o[5] + R[5] @ UR5_EE_T, R[5] @ UR5_EE_R


def ee_pose(R, o):
    return o[EE_PARENT] + R[EE_PARENT] @ EE_T, R[EE_PARENT] @ EE_R


def samples(R, o):
    L = ANL + SAMP_LINK
    return o[L] + R[L][:, :, 1] * SAMP_Y[:, None]


# ------------------------------------------------------------------------------------------------ geometry from the definitions
def tube_sdf(a, rho):
    """signed distance of a point of the (axial, radial) half plane to the rectangle |a| <= hl, Rin <= rho <= Rout
    -> (sdf, [(grad_a, grad_rho), ...] every admissible gradient, region name)"""
    lo = np.array([-HOLE_HL, RIN]); hi = np.array([HOLE_HL, ROUT]); x = np.array([a, rho])
    proj = np.minimum(np.maximum(x, lo), hi)
    sa = "+" if a >= 0 else "-"; so = "out" if rho >= 0.5 * (RIN + ROUT) else "in"
    if (proj != x).any():
        d = x - proj; dist = np.hypot(*d)
        region = ("corner" + sa + so) if (d != 0).all() else (("face" + sa) if d[0] != 0 else ("wall-" + so))
        return dist, [tuple(d / dist)], region
    edges = [(hi[0] - a, (1.0, 0.0)), (a - lo[0], (-1.0, 0.0)), (hi[1] - rho, (0.0, 1.0)), (rho - lo[1], (0.0, -1.0))]
    best = min(e[0] for e in edges)
    grads = [g for d, g in edges if d - best < TIE]
    axial = grads[0][0] != 0
    return -best, grads, "interior-" + ("axial" + sa if axial else "radial-" + so)


def box_sdf(pl, h):
    """signed distance of a point (box frame) to the box |x_k| <= h_k -> (sdf, [unit gradient, ...], region)"""
    proj = np.clip(pl, -h, h)
    d = pl - proj
    nout = int((d != 0).sum())
    if nout:
        dist = np.linalg.norm(d)
        return dist, [d / dist], ("face", "edge", "corner")[nout - 1] + ("" if nout > 1 else "xyz"[int(np.flatnonzero(d)[0])] + ("+" if d.sum() > 0 else "-"))
    pen = h - np.abs(pl)
    best = pen.min()
    grads = []
    for k in range(3):
        if pen[k] - best < TIE:
            g = np.zeros(3); g[k] = 1.0 if pl[k] >= 0 else -1.0; grads.append(g)
    return -best, grads, "interior-" + "xyz"[int(np.argmin(pen))]


def _pt_seg(x, a, d):
    dd = d @ d
    t = 0.0 if dd == 0 else min(1.0, max(0.0, (x - a) @ d / dd))
    return t


def seg_seg(p1, q1, p2, q2):
    """closest points of two segments -> (distance, [(c1, c2), ...] every closest pair found, kind, parallel)
    kind: 'interior' (common perpendicular), 'clamp-s' / 'clamp-t' (an end point of segment 1 / 2 against the inside of the other), 'end-end'"""
    d1 = q1 - p1; d2 = q2 - p2
    cands = []
    for s in (0.0, 1.0):
        x = p1 + s * d1; t = _pt_seg(x, p2, d2); cands.append((s, t))
    for t in (0.0, 1.0):
        x = p2 + t * d2; s = _pt_seg(x, p1, d1); cands.append((s, t))
    n = np.cross(d1, d2); nn = n @ n
    parallel = nn <= 1e-12 * (d1 @ d1) * (d2 @ d2)
    if not parallel:
        w = p2 - p1
        s = np.cross(w, d2) @ n / nn; t = np.cross(w, d1) @ n / nn
        if 0 <= s <= 1 and 0 <= t <= 1:
            cands.append((s, t))
    pts = [(p1 + s * d1, p2 + t * d2, s, t) for s, t in cands]
    dist = [np.linalg.norm(a - b) for a, b, _, _ in pts]
    best = min(dist)
    k = int(np.argmin(dist))
    keep = [(a, b) for (a, b, _, _), d in zip(pts, dist) if d - best < 0.1 * PARALLEL_SLACK] if parallel else [pts[k][:2]]
    s, t = pts[k][2], pts[k][3]
    es, et = s in (0.0, 1.0), t in (0.0, 1.0)
    kind = "end-end" if es and et else ("clamp-s" + str(int(s)) if es else ("clamp-t" + str(int(t)) if et else "interior"))
    return best, keep, kind, parallel


def point_capsule(x, a, b, rad):
    """distance of a point to a capsule built as a cylinder side and two end spheres -> (signed distance, foot on the axis, part)"""
    ab = b - a; l2 = ab @ ab
    u = (x - a) @ ab / l2 if l2 > 0 else -1.0
    if 0 <= u <= 1 and l2 > 0:
        foot = a + u * ab; part = "side"
    else:
        da, db = np.linalg.norm(x - a), np.linalg.norm(x - b)
        foot, part = (a, "endA") if (da <= db) else (b, "endB")
    return np.linalg.norm(x - foot) - rad, foot, part


# ------------------------------------------------------------------------------------------------ the contact list
class Cand:
    """a contact candidate: key, links, friction, every admissible (p, n, depth), optional = may be absent, free_radial = only the axial parts count"""
    __slots__ = ("key", "la", "lb", "mu", "alts", "optional", "free_radial", "branch", "arm", "slack", "cond")

    def __init__(self, key, la, lb, mu, alts, optional=False, free_radial=False, branch="", arm=False, slack=0.0, cond=np.inf):
        self.cond = cond           # distance over which the normal is formed, (x - foot) / cond: its error is the position error over cond
        self.key, self.la, self.lb, self.alts, self.optional, self.free_radial, self.branch, self.arm, self.slack = key, la, lb, alts, optional, free_radial, branch, arm, slack
        self.mu = min(MAX_FRICTION, max(-MAX_FRICTION, mu))

    @property
    def sensitive(self):
        return self.optional or self.free_radial or len(self.alts) > 1 or self.slack > 0


def _margin_gate(depth, margin):
    """-> (present, optional)"""
    if abs(depth - margin) < EDGE:
        return True, True
    return depth < margin, False


def _sphere_contact(sp, n, depth):
    """contact of a pipe sample sphere: the point half way between the sphere's surface and the other body's, along the normal"""
    return sp - (RADIUS + 0.5 * depth) * n, n, depth


def reference(state, mode=0, margin=MARGIN, armcol=3, selfcol=1, attach_ball=0):
    """-> list of passes, each a list of Cand in key order, BEFORE the caps (see apply_caps)"""
    R, o = fk(state)
    sp = samples(R, o)
    passes = []
    # table: the 25 rope vertices against the plane z = TABLE_Z
    P = []
    for v, i in enumerate(VERT_SAMPLE):
        depth = sp[i, 2] - TABLE_Z - RADIUS
        ok, opt = _margin_gate(depth, margin)
        if ok:
            L = ANL + SAMP_LINK[i]
            P.append(Cand(v, L, -1, LINK_MU[L] * TABLE_MU, [_sphere_contact(sp[i], np.array([0, 0, 1.0]), depth)], opt, branch="table"))
    passes.append(P)
    # hole tube, axis x through HOLE_POS
    P = []
    for i in range(NSAMP):
        d = sp[i] - HOLE_POS
        rho = np.hypot(d[1], d[2])
        sdf, grads, region = tube_sdf(d[0], rho)
        depth = sdf - RADIUS
        ok, opt = _margin_gate(depth, margin)
        if not ok:
            continue
        L = ANL + SAMP_LINK[i]
        radial = any(g[1] != 0 for g in grads)
        if radial and rho < AXIS_EPS:
            # the radial direction is rounding noise (and undefined on the axis itself): present or not, only its axial parts are checked
            n = np.array([grads[0][0], 0.0, 0.0])
            P.append(Cand(100 + i, L, -1, LINK_MU[L] * HOLE_MU, [_sphere_contact(sp[i], n, depth)], True, True, branch="tube:" + region))
            continue
        e = np.array([0, d[1] / rho, d[2] / rho]) if rho > 0 else np.zeros(3)
        alts = [_sphere_contact(sp[i], np.array([ga, 0, 0]) + gr * e, depth) for ga, gr in grads]
        P.append(Cand(100 + i, L, -1, LINK_MU[L] * HOLE_MU, alts, opt, branch="tube:" + region, cond=sdf if sdf > 0 else np.inf))
    passes.append(P)
    # attach (ball joint) and weld of the scripted grasp, FSM states 4..6
    P = []
    if mode == 1 and 4 <= state[S_FSM] <= 6:
        from scipy.spatial.transform import Rotation
        g = int(state[S_GRASP]); L = ANL if g == 0 else NL - 1
        a1 = o[L] + R[L] @ np.array([0, (0.045 if g == 0 else 0.015) + state[S_RANDY], 0])
        ee, eR = ee_pose(R, o)
        d = a1 - ee; dist = np.linalg.norm(d)
        P.append(Cand(2000, L, EE_PARENT, -1.0, [(0.5 * (a1 + ee), d / dist, dist)], branch="attach", arm=True))
        if not attach_ball:
            Rcf = Rotation.from_euler("xyz", [0, -np.pi, np.pi / 2 + state[S_ATTACH_QZ]]).as_matrix()
            th = Rotation.from_matrix(R[L] @ Rcf @ eR.T).as_rotvec()
            P.append(Cand(2001, L, EE_PARENT, -2.0, [(th, np.array([1.0, 0, 0]), 0.0)], branch="weld", arm=True))
    passes.append(P)
    # arm spheres against the table
    P = []
    cw = o[SPH_LINK] + np.einsum("nij,nj->ni", R[SPH_LINK], SPH_C)
    if armcol & 1:
        for i in range(NSPH):
            depth = cw[i, 2] - TABLE_Z - SPH_R[i]
            ok, opt = _margin_gate(depth, margin)
            if ok:
                p = np.array([cw[i, 0], cw[i, 1], cw[i, 2] - SPH_R[i] - 0.5 * depth])
                P.append(Cand(3000 + i, SPH_LINK[i], -1, LINK_MU[SPH_LINK[i]] * TABLE_MU, [(p, np.array([0, 0, 1.0]), depth)], opt, branch="arm-table", arm=True))
    passes.append(P)
    # finger pad boxes
    for f in range(2):
        P = []
        LF = FINGER0 + f
        bc = o[LF] + R[LF] @ BOX_C[f]
        near = np.flatnonzero(np.linalg.norm(sp - bc, axis=1) < np.linalg.norm(BOX_H) + RADIUS + margin + 1e-3)
        for i in near:
            sdf, grads, region = box_sdf(R[LF].T @ (sp[i] - bc), BOX_H)
            depth = sdf - RADIUS
            ok, opt = _margin_gate(depth, margin)
            if ok:
                L = ANL + SAMP_LINK[i]
                P.append(Cand(300 + f * NSAMP + i, L, LF, LINK_MU[L] * LINK_MU[LF], [_sphere_contact(sp[i], R[LF] @ g, depth) for g in grads], opt,
                              branch="box%d:%s" % (f, region), arm=True, cond=sdf if sdf > 0 else np.inf))
        passes.append(P)
    # arm spheres PIPE_SPH0.. against the pipe samples: the deepest sphere per sample
    P = []
    if armcol & 2:
        D = np.linalg.norm(sp[:, None, :] - cw[None, PIPE_SPH0:, :], axis=2)
        dep = D - RADIUS - SPH_R[None, PIPE_SPH0:]
        for i in np.flatnonzero(dep.min(1) < margin + EDGE):
            order = np.argsort(dep[i], kind="stable")
            s0 = int(order[0]); best = dep[i, s0]
            ok, opt = _margin_gate(best, margin)
            if not ok:
                continue
            tied = [int(s) for s in order if dep[i, s] - best < 1e-7]
            L = ANL + SAMP_LINK[i]
            if len(tied) > 1:       # two spheres equally deep: either (never generated on purpose; kept so that it is not silently dropped)
                opt = True
            s = PIPE_SPH0 + s0
            n = (sp[i] - cw[s]) / D[i, s0]
            P.append(Cand(5000 + s * NSAMP + i, L, SPH_LINK[s], LINK_MU[L] * LINK_MU[SPH_LINK[s]], [_sphere_contact(sp[i], n, best)], opt, branch="arm-pipe:%d" % s, arm=True))
    passes.append(P)
    # self collision: capsule segments s, t >= s + 2
    P = []
    if selfcol:
        vt = sp[VERT_SAMPLE]
        mid = 0.5 * (vt[:-1] + vt[1:]); half = 0.5 * np.linalg.norm(vt[1:] - vt[:-1], axis=1)
        for s, t in PAIRS:
            if np.linalg.norm(mid[s] - mid[t]) > half[s] + half[t] + 2 * RADIUS + margin + 1e-3:
                continue
            dist, pairs, kind, par = seg_seg(vt[s], vt[s + 1], vt[t], vt[t + 1])
            depth = dist - 2 * RADIUS
            ok, opt = _margin_gate(depth, margin)
            if not ok:
                continue
            if dist < 1e-6:                # crossing axes have no normal (the product drops the pair below 1e-9): present or not, nothing compared
                P.append(Cand(1000 + s * 24 + t, ANL + s, ANL + t, LINK_MU[ANL + s] * LINK_MU[ANL + t], [(0.5 * (pairs[0][0] + pairs[0][1]), np.zeros(3), depth)],
                              True, branch="self:crossing", slack=1.0))
                continue
            alts = [(0.5 * (c1 + c2), (c1 - c2) / dist, depth) for c1, c2 in pairs]
            P.append(Cand(1000 + s * 24 + t, ANL + s, ANL + t, LINK_MU[ANL + s] * LINK_MU[ANL + t], alts, opt, branch="self:" + ("parallel" if par else kind),
                          slack=PARALLEL_SLACK if par else 0.0, cond=dist))
    passes.append(P)
    return passes


def apply_caps(passes):
    """the documented caps on the candidate lists: at most CAMAX contacts that involve the arm, each arm pass losing its tail first; then
    at most CMAX contacts in all, the tail of the list lost.  -> (kept list, candidates in all, arm-involving candidates in all)"""
    out = []; nca = 0
    for P in passes:
        if P and P[0].arm:
            P = P[:max(0, CAMAX - nca)]
            nca += len(P)
        out += P
    return out[:CMAX], sum(len(P) for P in passes), sum(len(P) for P in passes if P and P[0].arm)


# ------------------------------------------------------------------------------------------------ cases
class Case:
    __slots__ = ("state", "cfg", "tag", "passes", "kept", "ncand", "narm", "sensitive")

    def __init__(self, state, cfg, tag=""):
        s = np.zeros(STATE_WORDS); s[:len(state)] = state
        self.state = f32(s); self.cfg = dict(cfg); self.tag = tag
        self.passes = reference(self.state, **cfg)
        self.kept, self.ncand, self.narm = apply_caps(self.passes)
        # a candidate that may be absent shifts every later slot: the whole list of such a case is compared as a set of admissible answers
        self.sensitive = any(c.sensitive for P in self.passes for c in P)


def cfg_key(cfg):
    d = dict(mode=0, margin=MARGIN, armcol=3, selfcol=1)
    d.update(cfg)
    return tuple(sorted(d.items()))


FAR = np.array([3.0, 3.0, 1.0])                                # a pipe parked here touches nothing


def base_state(rng=None, arm=None):
    s = np.zeros(WORDS)
    s[S_QARM:S_QARM + ANL] = ARM_REST if arm is None else arm
    s[S_TARGET:S_TARGET + ANL] = s[S_QARM:S_QARM + ANL]
    s[S_POS:S_POS + 3] = FAR; s[S_QUAT + 3] = 1.0
    return s


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _rand_R(rng):
    from scipy.spatial.transform import Rotation
    return Rotation.from_quat(rng.normal(size=4)).as_matrix()


def place_pipe(s, i, x, Rroot, qj=None):
    """root pose such that sample sphere i sits at the world point x with the root link turned by Rroot (joints qj)"""
    if qj is not None:
        s[S_QJ:S_QJ + 23] = qj
    s[S_QUAT:S_QUAT + 4] = f32(R_to_quat(Rroot)); s[S_POS:S_POS + 3] = 0
    R, o = fk(f32(np.concatenate([s, np.zeros(STATE_WORDS - len(s))])))
    s[S_POS:S_POS + 3] = x - samples(R, o)[i]
    return s


def random_arm(rng, open_fingers=True):
    q = rng.uniform(LINK_LO[:ANL], LINK_HI[:ANL])
    if open_fingers:
        q[7:] = rng.uniform(0.015, 0.04, 2)
    return q


def _arm_clear(q, zmin=0.12):
    """the arm's spheres and pads stay above the table by zmin (so that a class meant for the pipe alone sees the pipe alone)"""
    s = base_state(arm=q); R, o = fk(np.concatenate([s, np.zeros(STATE_WORDS - WORDS)]))
    cw = o[SPH_LINK] + np.einsum("nij,nj->ni", R[SPH_LINK], SPH_C)
    return (cw[:, 2] - SPH_R).min() - TABLE_Z > zmin


SAMPLE_PICKS = (0, 7, 61, 62, 63, 64, 117, 122)                # first / middle / last, and the lanes 62..64 around the first pass of 64


def class_T(rng, n=60, margin=MARGIN):
    out = []
    for k in range(n):
        s = base_state()
        qj = rng.uniform(-0.25, 0.25, 23) if k % 2 else np.zeros(23)
        Rr = rot_axis(_unit(rng), rng.uniform(0, 0.12)) @ rot_axis(np.array([0, 0, 1.0]), rng.uniform(-np.pi, np.pi))
        if k % 5 == 0:                                                   # upright: one end on the table (vertex 0, or the special key 24)
            Rr = rot_axis(np.array([1.0, 0, 0]), (1 if k % 10 else -1) * (np.pi / 2 - rng.uniform(0, 0.2))) @ Rr
        s = place_pipe(s, 0, np.array([2.0, 2.0, 1.0]), Rr, qj)
        R, o = fk(np.concatenate([f32(s), np.zeros(STATE_WORDS - WORDS)]))
        zmin = samples(R, o)[VERT_SAMPLE, 2].min()
        s[S_POS + 2] += TABLE_Z + RADIUS + rng.uniform(-0.004, margin + 0.002) - zmin
        out.append(Case(s, dict(margin=margin, selfcol=0), "T"))
    return out


TUBE_REGIONS = ("interior-axial+", "interior-axial-", "interior-radial-in", "interior-radial-out", "wall-in", "wall-out", "face+", "face-",
                "corner+in", "corner+out", "corner-in", "corner-out", "outside")


def _tube_point(rng, region, margin):
    """(a, rho) in a region of the rectangle's plane, its depth spread over (-r, margin) and a little beyond"""
    hw = 0.5 * (ROUT - RIN); rc = 0.5 * (RIN + ROUT)
    reach = RADIUS + margin
    far = lambda: rng.uniform(NEAR, reach * 1.05)
    if region.startswith("interior"):
        if "axial" in region:
            dx = -rng.uniform(1e-5, hw); dy = -rng.uniform(-dx + 1e-5, hw) if -dx + 1e-5 < hw else -hw
            sa = 1 if region.endswith("+") else -1; sr = rng.choice([-1, 1])
        else:
            dy = -rng.uniform(1e-5, hw); dx = -rng.uniform(-dy + 1e-5, HOLE_HL)
            sa = rng.choice([-1, 1]); sr = 1 if region.endswith("out") else -1
    elif region.startswith("wall"):
        dx = -rng.uniform(0, HOLE_HL); sa = rng.choice([-1, 1]); sr = 1 if region.endswith("out") else -1
        dy = far() if sr > 0 else rng.uniform(NEAR, min(reach * 1.05, RIN - 2 * AXIS_EPS))
    elif region.startswith("face"):
        dx = far(); dy = -rng.uniform(0, hw); sa = 1 if region.endswith("+") else -1; sr = rng.choice([-1, 1])
    elif region.startswith("corner"):
        sa = 1 if region[6] == "+" else -1; sr = 1 if region.endswith("out") else -1
        rad = far(); ang = rng.uniform(0.05, np.pi / 2 - 0.05)
        dx = rad * np.cos(ang); dy = rad * np.sin(ang)
        if sr < 0:
            dy = min(dy, RIN - 2 * AXIS_EPS)
    else:                                                                # outside the margin, by up to 1 cm
        sa = rng.choice([-1, 1]); sr = 1
        rad = reach + rng.uniform(2 * EDGE, 0.01); ang = rng.uniform(0, np.pi / 2)
        dx = rad * np.cos(ang); dy = rad * np.sin(ang)
    return sa * (HOLE_HL + dx), rc + sr * (hw + dy)


def class_H(rng, per_region=44, margin=MARGIN, tag="H"):
    out = []
    for region in TUBE_REGIONS:
        for k in range(per_region):
            a, rho = _tube_point(rng, region, margin)
            phi = rng.uniform(-np.pi, np.pi) if k % 4 else (k // 4 % 4) * np.pi / 2            # several azimuths, the four axes among them
            x = HOLE_POS + np.array([a, rho * np.cos(phi), rho * np.sin(phi)])
            i = SAMPLE_PICKS[k % len(SAMPLE_PICKS)]
            qj = rng.uniform(-0.3, 0.3, 23) if k % 3 == 0 else np.zeros(23)
            s = place_pipe(base_state(), i, x, _rand_R(rng), qj)
            out.append(Case(s, dict(margin=margin, armcol=0, selfcol=0), tag + ":" + region))
    return out


def class_H_axis(rng, n=24, margin=float(np.float32(0.006))):
    """sample spheres on and within 1e-4 of the tube axis, at a margin that reaches the inner wall from there (Rin - r = 5.36 mm)"""
    out = []
    for k in range(n):
        a = rng.uniform(-HOLE_HL, HOLE_HL) if k % 3 else rng.choice([-1, 1]) * (HOLE_HL + rng.uniform(1e-3, 4e-3))
        rho = 0.0 if k % 2 == 0 else rng.uniform(0, AXIS_EPS * 0.9)
        phi = rng.uniform(-np.pi, np.pi)
        x = HOLE_POS + np.array([a, rho * np.cos(phi), rho * np.sin(phi)])
        Rr = rot_axis(np.array([0, 0, 1.0]), -np.pi / 2) if k % 4 == 0 else _rand_R(rng)            # k % 4 == 0: the pipe threaded along the axis
        s = place_pipe(base_state(), SAMPLE_PICKS[k % len(SAMPLE_PICKS)], x, Rr)
        out.append(Case(s, dict(margin=margin, armcol=0, selfcol=0), "M:axis"))
    return out


BOX_REGIONS = ("interior-x", "interior-y", "interior-z", "facex+", "facex-", "facey+", "facey-", "facez+", "facez-", "edge", "corner", "beyond")


def _box_point(rng, region, margin):
    h = BOX_H; reach = RADIUS + margin
    if region.startswith("interior"):
        k = "xyz".index(region[-1])
        pen = rng.uniform(1e-4, h.min() * 0.95)
        pl = np.sign(rng.uniform(-1, 1, 3)) * (h - pen - rng.uniform(2 * TIE, 1.0, 3) * (h - pen))
        pl[k] = rng.choice([-1, 1]) * (h[k] - pen)
        return pl
    if region.startswith("face"):
        k = "xyz".index(region[4]); sg = 1 if region[5] == "+" else -1
        pl = rng.uniform(-h, h); pl[k] = sg * (h[k] + rng.uniform(NEAR, reach * 1.05))
        return pl
    if region == "beyond":                                               # between the exact reach (half diagonal + r + margin) and well past 5 cm
        return _unit(rng) * rng.uniform(np.linalg.norm(h) + reach + 1e-4, 0.07)
    nout = 2 if region == "edge" else 3
    ks = rng.permutation(3)[:nout]
    v = np.abs(rng.normal(size=nout)) + 0.2; v *= rng.uniform(NEAR, reach * 1.05) / np.linalg.norm(v)
    pl = rng.uniform(-h, h)
    pl[ks] = np.sign(rng.uniform(-1, 1, nout)) * (h[ks] + v)
    return pl


def class_F(rng, per_region=16, margin=MARGIN, tag="F"):
    out = []
    for region in BOX_REGIONS:
        for k in range(per_region):
            f = k % 2
            while True:
                q = random_arm(rng) if k % 4 < 3 else np.concatenate([ARM_REST[:7], rng.uniform(0.015, 0.04, 2)])
                if _arm_clear(q):
                    break
            s = base_state(arm=q)
            R, o = fk(np.concatenate([f32(s), np.zeros(STATE_WORDS - WORDS)]))
            LF = FINGER0 + f
            x = o[LF] + R[LF] @ (BOX_C[f] + _box_point(rng, region, margin))
            s = place_pipe(s, SAMPLE_PICKS[(k // 2) % len(SAMPLE_PICKS)], x, _rand_R(rng))
            out.append(Case(s, dict(margin=margin, armcol=0 if k % 3 else 3, selfcol=0), "%s:box%d:%s" % (tag, f, region)))
    return out


def class_A(rng, n_table=48, n_pipe=72):
    out = []
    k = 0
    while k < n_table:                                                   # arm poses whose spheres straddle the table's margin
        q = random_arm(rng)
        s = base_state(arm=q); R, o = fk(np.concatenate([f32(s), np.zeros(STATE_WORDS - WORDS)]))
        cw = o[SPH_LINK] + np.einsum("nij,nj->ni", R[SPH_LINK], SPH_C)
        dep = cw[:, 2] - TABLE_Z - SPH_R
        if not (-0.03 < dep.min() < MARGIN + 0.003):
            continue
        out.append(Case(s, dict(armcol=(3, 1, 2, 0)[k % 4] if k >= 8 else 3, selfcol=0), "A:table"))
        k += 1
    for k in range(n_pipe):                                              # a pipe sample at the surface of one of the hand / wrist spheres
        while True:
            q = random_arm(rng)
            if _arm_clear(q):
                break
        s = base_state(arm=q); R, o = fk(np.concatenate([f32(s), np.zeros(STATE_WORDS - WORDS)]))
        sph = PIPE_SPH0 + k % (NSPH - PIPE_SPH0)
        c = o[SPH_LINK[sph]] + R[SPH_LINK[sph]] @ SPH_C[sph]
        x = c + _unit(rng) * (SPH_R[sph] + RADIUS + rng.uniform(-0.008, MARGIN + 0.002))
        s = place_pipe(s, SAMPLE_PICKS[(k // 7) % len(SAMPLE_PICKS)], x, _rand_R(rng))
        out.append(Case(s, dict(armcol=(3, 2, 1, 0)[k % 4] if k >= 16 else 3, selfcol=0), "A:pipe"))
    return out


def fold_joints(s, t, gap, rng, jitter=0.0):
    """pipe joint angles that bring segments s and t (t >= s + 2) to about `gap` of each other: one joint between them folded to a V whose
    legs hold s and t at (about) the same distance from the apex; `jitter` turns the neighbouring joints a little, out of the plane"""
    seg = 0.055
    j = (s + t - 1) // 2                                                 # joint j sits between segments j and j + 1
    m = (t - s - 1) // 2 if (t - s) % 2 else (t - s) // 2                # distance of the nearer ends from the apex, in links
    m = max(m, 1)
    half = np.arcsin(min(1.0, gap / (2 * m * seg)))
    qj = np.zeros(23)
    qj[j] = (np.pi - 2 * half) * rng.choice([-1, 1])
    if jitter:
        lo, hi = max(0, s), min(22, t - 1)
        for k in range(lo, hi + 1):
            if k != j:
                qj[k] += rng.uniform(-jitter, jitter)
    return qj


def class_S(rng, margin=MARGIN):
    """every one of the 253 pairs folded into reach (three gaps each, the last with the neighbouring joints turned out of the plane), then
    sub-classes built on purpose: crossing segments (interior common perpendicular), exactly parallel and near-parallel pairs, and
    collinear segments whose gap straddles 2 r + margin (the edge of the broad phase's reach)"""
    out = []
    cfg = dict(margin=margin, armcol=0, selfcol=1)
    for s, t in PAIRS:
        for v in range(3):
            gap = 2 * RADIUS + rng.uniform(-0.006, margin - 0.0005)
            qj = fold_joints(s, t, gap, rng, jitter=(0.0, 0.03, 0.25)[v])
            st = place_pipe(base_state(), 0, FAR, _rand_R(rng), qj)
            out.append(Case(st, cfg, "S:fold"))
    for k in range(60):                                                  # crossing: fold at a z joint, then lift the far leg about an x joint
        j = int(rng.integers(2, 20))
        qj = np.zeros(23)
        qj[j] = (np.pi - rng.uniform(0.15, 0.5)) * rng.choice([-1, 1])
        qj[j + 1] = rng.uniform(-0.6, 0.6); qj[j - 1] = rng.uniform(-0.6, 0.6); qj[j + 2] = rng.uniform(-0.8, 0.8)
        out.append(Case(place_pipe(base_state(), 0, FAR, _rand_R(rng), qj), cfg, "S:cross"))
    for k in range(40):                                                  # parallel: two joints of one axis that add up to a half turn
        a = int(rng.integers(1, 14))
        th = np.arcsin(rng.uniform(0.012, 2 * RADIUS + margin - 1e-3) / 0.11)
        qj = np.zeros(23); qj[a] = th; qj[a + 2] = np.pi - th
        if k % 2:                                                        # near-parallel: off by 1e-3 .. 3e-2 rad
            qj[a + 2] += rng.choice([-1, 1]) * np.exp(rng.uniform(np.log(1e-3), np.log(3e-2)))
        Rr = np.eye(3) if k % 4 == 0 else _rand_R(rng)
        out.append(Case(place_pipe(base_state(), 0, FAR, Rr, qj), cfg, "S:parallel" if k % 2 == 0 else "S:near-parallel"))
    for k in range(40):                                                  # collinear with a gap around 2 r + margin: segments a and a + 5
        a = int(rng.integers(1, 15))
        g = 2 * RADIUS + margin + (rng.uniform(2 * EDGE, 4e-4) * (1 if k % 2 else -1))
        phi = np.arccos(0.5 * g / 0.11)
        qj = np.zeros(23); qj[a] = phi; qj[a + 2] = -2 * phi; qj[a + 4] = phi
        out.append(Case(place_pipe(base_state(), 0, FAR, _rand_R(rng), qj), cfg, "S:reach-in" if k % 2 == 0 else "S:reach-out"))
    return out


EXACT_QUATS = [np.array(q, float) for q in ((0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (.5, .5, .5, .5), (-.5, .5, .5, .5), (.5, -.5, .5, .5), (.5, .5, -.5, .5))]


PAIR_INDEX = {1000 + s * 24 + t: i for i, (s, t) in enumerate(PAIRS)}


def _zigzag(j0, k, delta):
    """joints j0 .. j0 + k - 1 folded to pi - delta each (the joint axes alternate z, x): a fan of k + 1 segments about 5.5 cm long in which
    every segment is near many others, the rest of the pipe straight"""
    qj = np.zeros(23); qj[j0:j0 + k] = np.pi - delta * (1 + 0.3 * np.sin(1.7 * np.arange(k)))       # (uneven: equal folds make segments cross exactly)
    return qj


LANE_TARGETS = {63: "C:lane63", 64: "C:lane64", 127: "C:lane127", 128: "C:lane128", 191: "C:lane191"}       # and any index >= 192: "C:lane-partial"


def _cap_lane_cases(rng):
    """cases whose LAST kept contact (slot CMAX - 1) is the self-collision pair of index 63, 64, 127, 128, 191 or one of 192 .. 252 -- the
    last lane of a pass of 64 and the first of the next, and the partial fourth pass -- from a zig-zag that puts `pos` self contacts in
    front of the pair, tilted and lifted so that exactly T = CMAX - 1 - pos of its vertices reach the table; and cases whose 48th contact
    is the TUBE contact of sample 63 / 64 (the pass of 123 samples cut at its lane boundary): the whole pipe folded to a bundle across
    the tube, all but a few of its samples within reach of the wall"""
    out = []; want = set(LANE_TARGETS.values()) | {"C:lane-partial"}
    for j0, k in ((0, 14), (0, 10), (4, 14), (5, 14), (6, 8), (8, 10), (10, 8)):
        for delta in (0.06, 0.1, 0.15, 0.2):
            for trial in range(2):
                ax = rng.normal(size=2); ax = np.array([ax[0], ax[1], 0]) / np.hypot(*ax)
                Rr = rot_axis(ax, rng.uniform(0.1, 0.5)) @ _rand_R(rng)
                s = place_pipe(base_state(), 0, np.array([2.0, 2.0, 0.5]), Rr, _zigzag(j0, k, delta))
                probe = Case(s, dict(armcol=0, selfcol=1), "C:lane")
                lst = probe.passes[-1]
                if any(c.sensitive for c in lst):
                    continue
                R, o = fk(probe.state); z = np.sort(samples(R, o)[VERT_SAMPLE, 2])
                for pos, c in enumerate(lst):
                    idx = PAIR_INDEX[c.key]
                    tag = LANE_TARGETS.get(idx, "C:lane-partial" if idx >= 192 else None)
                    T = CMAX - 1 - pos
                    if tag in want and 1 <= T <= 24 and len(lst) > pos + 1 and z[T] - z[T - 1] > 20 * EDGE:
                        s2 = s.copy()
                        s2[S_POS + 2] += TABLE_Z + RADIUS + MARGIN - 0.5 * (z[T] + z[T - 1])
                        c2 = Case(s2, dict(armcol=0, selfcol=1), tag)
                        if not c2.sensitive and c2.ncand > CMAX and c2.kept[-1].key == c.key and len(c2.passes[0]) == T:
                            out.append(c2); want.discard(tag)
    for delta, off, lat in ((0.14, 0.012, 0.003), (0.3, 0.0125, 0.003), (0.1, 0.011, 0.011), (0.2, 0.011, 0.008)):    # (found by a scan of the offset)
        s = place_pipe(base_state(), 60, HOLE_POS + np.array([0.002, off, lat]), np.eye(3), _zigzag(0, 23, delta))
        c = Case(s, dict(armcol=0, selfcol=0), "C:tube")
        if not c.sensitive and c.ncand > CMAX and c.kept[-1].key in (163, 164):
            c.tag = "C:tube%d" % (c.kept[-1].key - 100)
            out.append(c)
    return out


def class_C(rng, n_total=40, n_arm=40, n_attach=40):
    out = []
    flat = rot_axis(np.array([0, 0, 1.0]), 0.3)
    for k in range(n_total):                                             # flat on the table, folded once: 25 table + the self contacts of a V
        qj = np.zeros(23)
        j = 2 * int(rng.integers(4, 8))                                  # a z joint: the V stays in the table's plane
        qj[j] = np.pi - np.exp(rng.uniform(np.log(0.004), np.log(0.12)))
        s = place_pipe(base_state(), 0, np.array([2.0, 2.0, 0]), rot_axis(np.array([0, 0, 1.0]), rng.uniform(-3, 3)), qj)
        s[S_POS + 2] = TABLE_Z + RADIUS + rng.uniform(-0.002, 0.003)
        out.append(Case(s, dict(armcol=0, selfcol=1), "C:total"))
    out += _cap_lane_cases(rng)
    for k in range(n_arm):                                               # a straight or gently bent pipe through the open gripper
        while True:
            q = random_arm(rng) if k % 2 else np.concatenate([ARM_REST[:7], rng.uniform(0.02, 0.04, 2)])
            if _arm_clear(q):
                break
        s = base_state(arm=q); R, o = fk(np.concatenate([f32(s), np.zeros(STATE_WORDS - WORDS)]))
        LF = FINGER0 + k % 2
        x = o[LF] + R[LF] @ (BOX_C[k % 2] + rng.uniform(-1, 1, 3) * np.array([0.012, 0.012, 0.03]))
        axis = R[LF] @ (np.array([0, 0, 1.0]) + 0.3 * rng.normal(size=3))              # along the finger, towards the hand
        axis /= np.linalg.norm(axis)
        side = np.cross(axis, _unit(rng)); side /= np.linalg.norm(side)
        Rr = np.stack([side, axis, np.cross(side, axis)], axis=1)                        # the root link's y axis (the pipe) along `axis`
        qj = rng.uniform(-0.05, 0.05, 23) if k % 3 == 0 else np.zeros(23)
        s = place_pipe(s, int(rng.integers(20, 100)), x, Rr, qj)
        out.append(Case(s, dict(armcol=3, selfcol=1), "C:arm"))
    for k in range(n_attach):                                            # scripted grasp, FSM states 4..6: attach + weld count against the arm cap
        q = np.concatenate([ARM_REST[:7], rng.uniform(0.0, 0.012, 2)])
        s = base_state(arm=q); R, o = fk(np.concatenate([f32(s), np.zeros(STATE_WORDS - WORDS)]))
        ee, eR = ee_pose(R, o)
        g = k % 2
        s[S_FSM] = 4 + k % 3; s[S_FSMT] = 0; s[S_GRASP] = g; s[S_RANDY] = f32(rng.uniform(-0.01, 0.01)); s[S_ATTACH_QZ] = f32(rng.uniform(-0.7, 0.7))
        s[S_QUAT:S_QUAT + 4] = EXACT_QUATS[k % len(EXACT_QUATS)]                    # exactly unit in fp32: the weld's rotation error is that of a rotation
        s[S_POS:S_POS + 3] = 0
        R, o = fk(np.concatenate([f32(s), np.zeros(STATE_WORDS - WORDS)]))
        L = ANL if g == 0 else NL - 1
        a1 = o[L] + R[L] @ np.array([0, (0.045 if g == 0 else 0.015) + s[S_RANDY], 0])
        s[S_POS:S_POS + 3] = ee - a1 + _unit(rng) * rng.uniform(1e-3, 6e-3)
        out.append(Case(s, dict(mode=1, armcol=3, selfcol=1), "C:attach"))
    return out


M20 = float(np.float32(0.02))
SEEDS = {"T": 101, "H": 102, "F": 103, "A": 104, "S": 105, "C": 106, "M": 107}


@functools.lru_cache(maxsize=None)
def cases(name):
    """the committed cases of a class (computed once, with their reference)"""
    rng = np.random.default_rng(SEEDS[name])
    if name == "M":
        return tuple(class_H(rng, 12, M20, "M:H") + class_F(rng, 8, M20, "M:F") + class_H_axis(rng))
    return tuple({"T": class_T, "H": class_H, "F": class_F, "A": class_A, "S": class_S, "C": class_C}[name](rng))


CLASSES = ("T", "H", "F", "A", "S", "C", "M")


def branch_counts(cs):
    """contacts of the reference per branch label, kept after the caps"""
    n = {}
    for c in cs:
        for k in c.kept:
            n[k.branch] = n.get(k.branch, 0) + 1
    return n


def tag_counts(cs):
    n = {}
    for c in cs:
        n[c.tag] = n.get(c.tag, 0) + 1
    return n


def group_by_config(cs):
    g = {}
    for i, c in enumerate(cs):
        g.setdefault(cfg_key(c.cfg), []).append(i)
    return g


# ------------------------------------------------------------------------------------------------ comparing an answer with the reference
def compare(case, rows, n, tol_p, tol_n, tol_d, tol_mu=1e-9, near_relief=False):
    """rows [CMAX, 12] (link a, link b, p, n, depth, mu, key, -) and count n of one env against the reference of `case`.
    -> (error string or None, (max point error, max normal error, max depth error) over the contacts compared)"""
    got = rows[:n]
    keys = [int(round(k)) for k in got[:, 10]]
    ep = en = ed = 0.0
    if not case.sensitive:
        want = [c.key for c in case.kept]
        if keys != want:
            return "keys %s, reference %s" % (keys, want), None
        cands = case.kept
    else:
        # admissible lists: every kept-or-droppable candidate may appear; order must be the reference's; what is certain must be there unless
        # a cap could have taken it (then the count decides: checked below)
        allc = {c.key: c for P in case.passes for c in P}
        order = [c.key for P in case.passes for c in P]
        if any(k not in allc for k in keys):
            return "keys %s: %s not among the reference's candidates" % (keys, [k for k in keys if k not in allc]), None
        pos = [order.index(k) for k in keys]
        if pos != sorted(pos) or len(set(keys)) != len(keys):
            return "keys %s out of order" % keys, None
        if case.ncand <= CMAX and case.narm <= CAMAX:
            missing = [c.key for c in allc.values() if not c.optional and c.key not in keys]
            if missing:
                return "certain contacts %s missing" % missing, None
        cands = [allc[k] for k in keys]
    for r, c in zip(got, cands):
        if (int(round(r[0])), int(round(r[1]))) != (c.la, c.lb):
            return "key %d: links (%d, %d), reference (%d, %d)" % (c.key, r[0], r[1], c.la, c.lb), None
        if abs(r[9] - c.mu) > tol_mu:
            return "key %d: friction %g, reference %g" % (c.key, r[9], c.mu), None
        best = None
        alts = list(c.alts)
        if c.slack and len(alts) > 1:           # a SET of closest pairs: any point between two of the found ones is one
            for p, nn, d in c.alts:
                for p2, _, _ in c.alts:
                    u = p2 - p; t = min(1.0, max(0.0, (r[2:5] - p) @ u / (u @ u))) if u @ u > 0 else 0.0
                    alts.append((p + t * u, nn, d))
        for p, nn, d in alts:
            if c.free_radial:
                e = (abs(r[2] - p[0]), abs(r[5] - nn[0]), abs(r[8] - d))
            else:
                e = (np.abs(r[2:5] - p).max(), np.abs(r[5:8] - nn).max(), abs(r[8] - d))
            if best is None or max(e[0] / tol_p, e[1] / tol_n, e[2] / tol_d) < max(best[0] / tol_p, best[1] / tol_n, best[2] / tol_d):
                best = e
        best = tuple(max(0.0, x - c.slack) for x in best)
        if near_relief:                # fp32 builds only: a normal formed over less than NEAR has its error counted in proportion
            best = (best[0], best[1] * min(1.0, c.cond / NEAR), best[2])
        if c.free_radial and abs(np.linalg.norm(r[5:8]) - 1) > 1e-5:
            return "key %d: normal of length %g" % (c.key, np.linalg.norm(r[5:8])), None
        if best[0] > tol_p or best[1] > tol_n or best[2] > tol_d:
            return "key %d (%s): point %.3e normal %.3e depth %.3e off the reference" % (c.key, c.branch, best[0], best[1], best[2]), None
        if not c.sensitive:
            ep, en, ed = max(ep, best[0]), max(en, best[1]), max(ed, best[2])
    return None, (ep, en, ed)


# ------------------------------------------------------------------------------------------------ the reference against brute force
def reference_geometry_check(n=2000, seed=9):
    """tube_sdf, box_sdf and seg_seg against bounded minimisation over the surfaces / the parameter square -> largest |difference| of the
    (signed) distance per primitive"""
    from scipy.optimize import minimize
    rng = np.random.default_rng(seed)
    worst = {"tube": 0.0, "box": 0.0, "segment": 0.0}

    def argmin(f, bounds, starts):
        best = np.inf
        for x0 in starts:
            r = minimize(f, x0, bounds=bounds, method="L-BFGS-B", options=dict(ftol=1e-15, gtol=1e-12))
            best = min(best, r.fun)
        return best

    for k in range(n):
        kind = ("tube", "box", "segment")[k % 3]
        if kind == "tube":
            x = np.array([rng.uniform(-0.04, 0.04), 0, 0]) + np.concatenate([[0], rng.uniform(-0.04, 0.04, 2)])
            rho = np.hypot(x[1], x[2]); phi0 = np.arctan2(x[2], x[1])
            surf = [(lambda u, R_=R_: np.sum((x - np.array([u[0], R_ * np.cos(u[1]), R_ * np.sin(u[1])])) ** 2), [(-HOLE_HL, HOLE_HL), (phi0 - 4, phi0 + 4)]) for R_ in (RIN, ROUT)]
            surf += [(lambda u, A_=A_: np.sum((x - np.array([A_, u[0] * np.cos(u[1]), u[0] * np.sin(u[1])])) ** 2), [(RIN, ROUT), (phi0 - 4, phi0 + 4)]) for A_ in (-HOLE_HL, HOLE_HL)]
            d = np.sqrt(min(argmin(f, b, [np.array([0.5 * (b[0][0] + b[0][1]), phi0 + e]) for e in (0.0, 0.7, -0.7)]) for f, b in surf))
            inside = abs(x[0]) <= HOLE_HL and RIN <= rho <= ROUT
            worst[kind] = max(worst[kind], abs((-d if inside else d) - tube_sdf(x[0], rho)[0]))
        elif kind == "box":
            h = BOX_H; x = rng.uniform(-2.5, 2.5, 3) * h
            best = np.inf
            for ax in range(3):
                for sg in (-1, 1):
                    o2 = [a for a in range(3) if a != ax]

                    def f(u):
                        y = np.zeros(3); y[ax] = sg * h[ax]; y[o2] = u
                        return np.sum((x - y) ** 2)
                    best = min(best, argmin(f, [(-h[a], h[a]) for a in o2], [np.zeros(2)]))
            d = np.sqrt(best)
            worst[kind] = max(worst[kind], abs((-d if (np.abs(x) <= h).all() else d) - box_sdf(x, h)[0]))
        else:
            p1, p2 = rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.05, 0.05, 3)
            d1 = _unit(rng) * rng.uniform(0.01, 0.09)
            d2 = _unit(rng) * rng.uniform(0.01, 0.09) if k % 9 else d1 * rng.uniform(-1.5, 1.5)          # every third segment pair is parallel
            f = lambda u: np.sum((p1 + u[0] * d1 - p2 - u[1] * d2) ** 2)
            d = np.sqrt(argmin(f, [(0, 1), (0, 1)], [np.array([a, b]) for a in (0.1, 0.9) for b in (0.1, 0.9)]))
            worst[kind] = max(worst[kind], abs(d - seg_seg(p1, p1 + d1, p2, p2 + d2)[0]))
    return worst


# ------------------------------------------------------------------------------------------------ random-fly: the candidate pass
FLY_WORDS = 48
F_Q, F_TARGET, F_OPOS, F_OQUAT = 0, 12, 18, 21
FLY_MARGIN = float(np.float32(0.02))
CAP_A = _macro("PIH_UR5_CAP_A"); CAP_B = _macro("PIH_UR5_CAP_B"); CAP_R = _macro("PIH_UR5_CAP_R")
OBJ_NSPH = _macro("PIH_FLY_OBJ_NSPH").astype(int); OBJ_SPH_C = _macro("PIH_FLY_OBJ_SPH_C"); OBJ_SPH_R = _macro("PIH_FLY_OBJ_SPH_R")
FNS, FNA = OBJ_SPH_C.shape[1], 5
FNC = 2 * FNS + FNA                                             # slots: sphere i vs its deepest capsule, sphere i vs the table, link 1 + a vs the table


def fly_capsules(q):
    R, o, _, _ = fk_ur5(q)
    return o + np.einsum("nij,nj->ni", R, CAP_A), o + np.einsum("nij,nj->ni", R, CAP_B)


def fly_reference(state, ob, margin=FLY_MARGIN):
    """-> list of FNC slots, each None (invalid) or dict(alts=[(link, p, n, depth), ...], optional, branch)"""
    A, B = fly_capsules(state[F_Q:F_Q + 6])
    Ro = quat_to_R(state[F_OQUAT:F_OQUAT + 4]); op = state[F_OPOS:F_OPOS + 3]
    slots = [None] * FNC
    for i in range(OBJ_NSPH[ob]):
        x = op + Ro @ OBJ_SPH_C[ob][i]; rs = OBJ_SPH_R[ob][i]
        per = []
        for L in range(6):
            sd, foot, part = point_capsule(x, A[L], B[L], CAP_R[L])
            dist = sd + CAP_R[L]
            per.append((sd - rs, L, foot, part, dist))
        best = min(p[0] for p in per)
        ok, opt = _margin_gate(best, margin)
        if ok:
            alts = []; branch = None
            for depth, L, foot, part, dist in per:
                if depth - best < TIE:                                   # a tie between links (their capsules overlap at every joint): either
                    n = (x - foot) / dist
                    alts.append((L, x - (rs + 0.5 * depth) * n, n, depth))
                    branch = branch or ("cap:" + part + (":axis" if dist < 1e-5 else ""))
            slots[i] = dict(alts=alts, optional=opt or min(p[4] for p in per) < 1e-8, branch=branch if len(alts) == 1 else "cap:tie")
        depth = x[2] - TABLE_Z - rs
        ok, opt = _margin_gate(depth, margin)
        if ok:
            slots[FNS + i] = dict(alts=[(-1, np.array([x[0], x[1], x[2] - rs - 0.5 * depth]), np.array([0, 0, 1.0]), depth)], optional=opt, branch="obj-table")
    for a in range(FNA):
        L = 1 + a
        ends = [A[L], B[L]]
        low = min(e[2] for e in ends)
        alts = []
        for e in ends:
            if e[2] - low < TIE:
                depth = e[2] - TABLE_Z - CAP_R[L]
                alts.append((L, np.array([e[0], e[1], e[2] - CAP_R[L] - 0.5 * depth]), np.array([0, 0, 1.0]), depth))
        ok, opt = _margin_gate(alts[0][3], margin)
        if ok:
            slots[2 * FNS + a] = dict(alts=alts, optional=opt, branch="link-table:" + ("tie" if len(alts) > 1 else ("A" if A[L][2] <= B[L][2] else "B")))
    return slots


class FlyCase:
    __slots__ = ("state", "ob", "tag", "slots", "sensitive")

    def __init__(self, state, ob, tag):
        s = np.zeros(FLY_WORDS); s[:len(state)] = state
        self.state = f32(s); self.ob = ob; self.tag = tag
        self.slots = fly_reference(self.state, ob)
        # (a centre within 1e-5 of a capsule axis is present for certain -- the product drops a contact only at a distance <= 1e-9 -- but its
        #  normal is noise: sensitive, compared by depth and unit length)
        self.sensitive = any(s is not None and (s["optional"] or len(s["alts"]) > 1 or s["branch"].endswith(":axis")) for s in self.slots)


def _fly_state(q, opos, Ro):
    s = np.zeros(FLY_WORDS)
    s[F_Q:F_Q + 6] = q; s[F_TARGET:F_TARGET + 6] = q; s[F_OPOS:F_OPOS + 3] = opos; s[F_OQUAT:F_OQUAT + 4] = R_to_quat(Ro)
    return s


@functools.lru_cache(maxsize=None)
def fly_cases(ob):
    """sphere-to-capsule: cylinder side, beyond end A, beyond end B, at a joint (two capsules overlap), out of margin, a centre within 1e-6
    of a capsule axis; capsule-to-table: arm poses that dip towards the table, a horizontal link (A / B tie)"""
    from scipy.optimize import fsolve
    rng = np.random.default_rng(200 + ob)
    out = []
    kinds = ("side", "endA", "endB", "joint", "out", "axis")
    for k in range(40 * len(kinds)):
        kind = kinds[k % len(kinds)]
        q = rng.uniform(-np.pi, np.pi, 6)
        A, B = fly_capsules(f32(q))
        L = int(rng.integers(0, 6)); i = int(rng.integers(0, OBJ_NSPH[ob])); rs = OBJ_SPH_R[ob][i]
        ab = B[L] - A[L]; ln = np.linalg.norm(ab); e = ab / ln
        perp = np.cross(e, _unit(rng)); perp /= np.linalg.norm(perp)
        gap = rng.uniform(-0.015, FLY_MARGIN - 1e-3) if kind != "out" else FLY_MARGIN + rng.uniform(1e-3, 0.02)
        rad = CAP_R[L] + rs + gap
        if kind in ("side", "out"):
            x = A[L] + rng.uniform(0.05, 0.95) * ab + rad * perp
        elif kind in ("endA", "endB"):
            c = A[L] if kind == "endA" else B[L]; sg = -1 if kind == "endA" else 1
            th = rng.uniform(0, 1.4)
            x = c + rad * (np.cos(th) * sg * e + np.sin(th) * perp)
        elif kind == "joint":                                            # at the origin of link L + 1 (or L), where neighbouring capsules overlap
            R, o, _, _ = fk_ur5(f32(q)); x = o[min(L + 1, 5)] + _unit(rng) * rng.uniform(0.03, 0.09)
        else:
            x = A[L] + rng.uniform(0, 1) * ab + perp * rng.uniform(0, 1e-6)
        Ro = _rand_R(rng)
        out.append(FlyCase(_fly_state(q, x - Ro @ OBJ_SPH_C[ob][i], Ro), ob, "fly:" + kind))
    n = 0
    while n < 60:                                                        # arm poses whose capsule ends straddle the table's margin; the object on the table
        q = rng.uniform(-np.pi, np.pi, 6)
        A, B = fly_capsules(f32(q))
        dep = np.minimum(A[1:, 2], B[1:, 2]) - TABLE_Z - CAP_R[1:]
        if not (-0.05 < dep.min() < FLY_MARGIN + 0.01):
            continue
        Ro = _rand_R(rng); z = TABLE_Z + rng.uniform(0.0, 0.06)
        out.append(FlyCase(_fly_state(q, np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), z]), Ro), ob, "fly:table")); n += 1
    for k in range(12):                                                  # the forearm (link 2) horizontal and low: its two ends tie
        q = rng.uniform(-np.pi, np.pi, 6)

        def f(v):
            qq = q.copy(); qq[1:3] = v
            A, B = fly_capsules(qq)
            return [A[2][2] - B[2][2], A[2][2] - TABLE_Z - CAP_R[2] - 0.005]
        v, info, ier, _ = fsolve(f, [2.0, 1.0] if k % 2 else [1.2, -1.5], full_output=True)
        if ier == 1:
            q[1:3] = v
            out.append(FlyCase(_fly_state(q, np.array([2.0, 2.0, 1.0]), np.eye(3)), ob, "fly:level"))
    return tuple(out)


def fly_compare(case, cand, tol_p, tol_n, tol_d, lam_word_is_index=True):
    """cand [FNC, 10] = valid, link, p, n, depth, - of one env against the reference -> (error or None, maxima over the slots that are not sensitive)"""
    worst = np.zeros(3)
    for k in range(FNC):
        ref = case.slots[k]; r = cand[k]
        if ref is None or (ref["optional"] and r[0] == 0):
            if ref is None and r[0] != 0:
                return "slot %d valid, reference invalid" % k, None
            continue
        if r[0] == 0:
            return "slot %d (%s) invalid, reference valid" % (k, ref["branch"]), None
        best = None
        for L, p, n, d in ref["alts"]:
            if int(round(r[1])) == L:
                e = (np.abs(r[2:5] - p).max(), np.abs(r[5:8] - n).max(), abs(r[8] - d))
                best = e if best is None or max(e) < max(best) else best
        if best is None:
            return "slot %d (%s): link %d, reference %s" % (k, ref["branch"], r[1], [a[0] for a in ref["alts"]]), None
        if ref["branch"].endswith(":axis"):                              # the normal of a centre on the axis is noise: a unit vector, the depth
            best = (0.0, abs(np.linalg.norm(r[5:8]) - 1) * tol_n / 1e-5, best[2])
        if best[0] > tol_p or best[1] > tol_n or best[2] > tol_d:
            return "slot %d (%s): point %.3e normal %.3e depth %.3e off the reference" % (k, ref["branch"], *best), None
        if not ref["optional"] and len(ref["alts"]) == 1:
            worst = np.maximum(worst, best)
    return None, worst


def fly_branch_counts(cs):
    n = {}
    for c in cs:
        for s in c.slots:
            if s is not None:
                n[s["branch"]] = n.get(s["branch"], 0) + 1
    return n
