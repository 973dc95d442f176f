"""Lit camera images of both tasks (pih_render_lit, peg_in_hole_gym_amd/csrc/pih_lit.h), CPU part: the product's lit per-scene and
per-pixel code, compiled on the host in fp64 and fp32 (tests/emul/pih_lit_emul.cpp), against a numpy fp64 reference written here from
the model text of include/pih_render_light.h.  States, cameras, sizes, scene geometry, the ray functions of the primary ray and the normal
helpers come from tests/test_peg_view.py and tests/test_fly_render.py; the reference is anchored to those modules' reference_render
(specular 0, shadow factor 1: their shaded image within 1e-9) and to closed-form answers that do not go through a ray caster.  A shadow
ray starts at its pixel's hit point, and the modules' ray functions take one origin for all rays: the ray functions here are theirs
with an origin per ray, and test_ray_functions_are_the_modules checks them against the imported ones.  The GPU part is tests/test_gpu_render_lit.py, which takes reference, scenes and rules from here.

Shadow state of a pixel.  The reference evaluates the shadow -- s of the model: is ndl > 0 and the shadow ray occluded? -- three times: with
the scene as it is, and with every primitive grown and shrunk by DELTA = 1e-4 m (radii +- DELTA, box half-extents +- DELTA, the tube's outer
radius and half-length +- DELTA and its inner radius -+ DELTA).  The primitive the pixel's own ray hits is one of them: the normal is taken
where the ray hits the grown or shrunk primitive, so a pixel on a terminator (ndl = 0 within what DELTA does to the normal), where a light from below switches the
shadow on, is as undecided as a pixel on a shadow's edge.  So is a pixel with a second surface of another orientation within DELTA behind
its hit: the builds need not agree on which of the two the ray meets.  DELTA is 50 x the rounding of a position 3 m from the origin through about ten fp32 operations (3 x 6e-8 x 10 = 2e-6),
and 1/38 of the thinnest occluder, the hole's wall.  A pixel is DECIDED where the three agree; there every build has to give the
reference's state, without exception; at most UNDECIDED_CAP of an image may be undecided (asserted on the reference).  A build's state is
recovered from two images under a probe light of the same direction (ambient 0, diffuse 1, specular 0: a pixel is base x s x max(0, ndl))
with shadow factor 0.5 and 1: shadowed = they differ."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import test_fly_render as FR
from tests import test_peg_view as PV

ROOT = PV.ROOT
SIZES = PV.SIZES
assert SIZES == FR.SIZES == ((97, 61), (64, 64), (40, 30))
BIAS = 1e-4                     # PIH_SHADOW_BIAS
DELTA = 1e-4
CLASS_SHARE = PV.CLASS_SHARE
UNDECIDED_CAP = 0.003
SHADOW_SHARE = 0.005
SHADED_P99, SHADED_MEDIAN = 0.05, 1e-3          # the project's bar for shaded colours (tests/test_render.py), grey levels
_D = list(_lib.LIGHT_DEFAULT)
LIGHTS = {
    "default": _D,
    "low": [1.0, 0.3, 0.2] + _D[3:],                                    # 11 degrees above the table: long shadows
    "below": [-50.0, 30.0, -100.0] + _D[3:],                            # l.z < 0: the table occludes everything above it
    "shiny": _D[:3] + [1.0, 0.8, 0.6, 0.6, 0.35, 0.4, 32.0, 0.8],       # coloured, specular 0.4, shininess 32
}
LIGHT_NAMES = ("default", "low", "below", "shiny")
L_DIR, L_COL, L_AMB, L_DIF, L_SPEC, L_SHINE, L_SHADOW = 0, 3, 6, 7, 8, 9, 10


def colour_factor(light):
    """how much faster than the diffuse term the highlight moves with an error in the normal"""
    return 1.0 + light[L_SPEC] * light[L_SHINE] / light[L_DIF]


def probe_light(light, shadow):
    return list(light[:3]) + [1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 2.0, float(shadow)]


# ------------------------------------------------------------------------------------------------ ray functions, one origin per ray
def _dot(a, b):
    return (a * b).sum(-1)


def ray_sphere(o, d, c, r):
    oc = o - c
    b = _dot(oc, d); disc = b * b - (_dot(oc, oc) - r * r)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    return np.where((disc >= 0) & (t > 0), t, np.inf)


def ray_capsule(o, d, a, b, r):
    ba, oa = b - a, o - a
    baba, bard, baoa, rdoa, oaoa = ba @ ba, d @ ba, oa @ ba, _dot(d, oa), _dot(oa, oa)
    A = baba - bard * bard; B = baba * rdoa - baoa * bard; Cc = baba * oaoa - baoa * baoa - r * r * baba
    h = B * B - A * Cc
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (-B - np.sqrt(np.maximum(h, 0.0))) / A; y = baoa + t * bard
        best = np.where((h >= 0) & (A > 1e-18) & (y > 0) & (y < baba) & (t > 0), t, np.inf)
    return np.minimum(best, np.minimum(ray_sphere(o, d, a, r), ray_sphere(o, d, b, r)))


def ray_tube(o, d, grow=0.0):
    hl, ri, ro = float(PV._macro("PIH_HOLE_HALFLEN")) + grow, float(PV._macro("PIH_HOLE_RIN")) - grow, float(PV._macro("PIH_HOLE_ROUT")) + grow
    oc = o - PV.HOLE_POS
    a = d[..., 1] ** 2 + d[..., 2] ** 2; b = oc[..., 1] * d[..., 1] + oc[..., 2] * d[..., 2]; r2o = oc[..., 1] ** 2 + oc[..., 2] ** 2
    best = np.full(np.broadcast(a, b).shape, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for rr, sign in ((ro, -1.0), (ri, 1.0)):
            disc = b * b - a * (r2o - rr * rr)
            t = (-b + sign * np.sqrt(np.maximum(disc, 0.0))) / a
            ok = (a >= 1e-18) & (disc >= 0) & (t > 0) & (np.abs(oc[..., 0] + t * d[..., 0]) <= hl) & (t < best)
            best = np.where(ok, t, best)
        for end in (-hl, hl):
            t = (end - oc[..., 0]) / d[..., 0]
            r2 = (oc[..., 1] + t * d[..., 1]) ** 2 + (oc[..., 2] + t * d[..., 2]) ** 2
            ok = (np.abs(d[..., 0]) >= 1e-15) & (t > 0) & (t < best) & (r2 >= ri * ri) & (r2 <= ro * ro)
            best = np.where(ok, t, best)
    return best


def ray_box(o, d, R, c, h):
    ol = (o - c) @ R; dl = d @ R
    shape = np.broadcast(ol[..., 0], dl[..., 0]).shape
    tmin = np.full(shape, -np.inf); tmax = np.full(shape, np.inf); miss = np.zeros(shape, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            par = np.abs(dl[..., k]) < 1e-15
            miss = miss | (par & (np.abs(ol[..., k]) > h[k]))
            t1 = (-h[k] - ol[..., k]) / dl[..., k]; t2 = (h[k] - ol[..., k]) / dl[..., k]
            lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
            tmin = np.where(par, tmin, np.maximum(tmin, lo)); tmax = np.where(par, tmax, np.minimum(tmax, hi))
    return np.where(miss | (tmin > tmax) | (tmax <= 0) | (tmin <= 0), np.inf, tmin)


def _radial(ph, c):
    r = ph - c
    return r / np.maximum(np.linalg.norm(r, axis=-1, keepdims=True), 1e-12)


# ------------------------------------------------------------------------------------------------ scenes
class Prim:
    """one primitive: kind 'capsule' (a, b, r) | 'sphere' (c, r) | 'box' (R, c, h) | 'tube'; base = flat rgb; seg = the seg byte; cls = the
    class the comparison rule uses; arm = link index of a peg-in-hole arm capsule (the tie rule of pih_view.h), else None"""

    def __init__(self, kind, base, seg, cls, arm=None, **p):
        self.kind, self.base, self.seg, self.cls, self.arm, self.p = kind, np.full(3, base) if np.ndim(base) == 0 else np.asarray(base, float), seg, cls, arm, p

    def hit(self, o, d, grow=0.0):
        p = self.p
        if self.kind == "capsule":
            return ray_capsule(o, d, p["a"], p["b"], p["r"] + grow)
        if self.kind == "sphere":
            return ray_sphere(o, d, p["c"], p["r"] + grow)
        if self.kind == "box":
            return ray_box(o, d, p["R"], p["c"], p["h"] + grow)
        return ray_tube(o, d, grow)

    def primary(self, eye, d3, fly):
        """the primary ray's hit, by the ray functions of the task's module: d3 [H, W, 3], one origin -> t [H * W]"""
        p = self.p
        if fly and self.kind == "capsule":
            t = np.minimum(FR._ref_cylinder(eye, d3, p["a"], p["b"], p["r"]), np.minimum(FR._ref_sphere(eye, d3, p["a"], p["r"]), FR._ref_sphere(eye, d3, p["b"], p["r"])))
        elif fly:
            t = FR._ref_sphere(eye, d3, p["c"], p["r"])
        elif self.kind == "capsule":
            t = PV._ref_capsule(eye, d3, p["a"], p["b"], p["r"])
        elif self.kind == "sphere":
            t = PV._ref_sphere(eye - p["c"], d3, p["r"])
        elif self.kind == "box":
            t = PV._ref_box(eye, d3, p["R"], p["c"], p["h"])
        else:
            t = PV._ref_tube(eye, d3)
        return t.reshape(-1)

    def normal(self, ph, grow=0.0):
        p = self.p
        if self.kind == "capsule":
            return PV._capsule_normal(ph, p["a"], p["b"])
        if self.kind == "sphere":
            return _radial(ph, p["c"])
        if self.kind == "box":
            return PV._box_normal(ph, p["R"], p["c"], p["h"] + grow)
        return PV._tube_normal(ph) if grow == 0.0 else tube_normal(ph, grow)


class Scene:
    """prims in the order the modules' reference_render tests them; table: (base, seg, cls); none: (seg, cls); ee = (p, R) of the frame an
    eye-in-hand camera rides on"""


def peg_scene(O, rec):
    org, hand, boxes, vtx, (pe, Re) = PV.scene_geometry(O, rec)
    s = Scene(); s.task = "peg"; s.ee = (pe, Re); s.table_z = PV.TABLE_Z
    s.table = (PV.COL_TABLE, _lib.VIEW_SEG_TABLE, _lib.VIEW_SEG_TABLE); s.none = (_lib.SEG_NONE, _lib.SEG_NONE)
    pr = float(PV._macro("PIH_PIPE_RADIUS")); bh = PV._macro("PIH_FINGER_BOX_H"); radii = PV.arm_radii()
    s.prims = [Prim("capsule", PV.COL_PIPE, _lib.VIEW_SEG_PIPE0 + k, _lib.VIEW_SEG_PIPE0 + k, a=vtx[k], b=vtx[k + 1], r=pr) for k in range(24)]
    s.prims.append(Prim("tube", PV.COL_PIPE, _lib.VIEW_SEG_HOLE, _lib.VIEW_SEG_HOLE))
    s.prims += [Prim("box", PV.COL_HAND, PV.SEG_FINGER0 + k, PV.SEG_FINGER0 + k, R=R, c=c, h=bh) for k, (R, c) in enumerate(boxes)]
    s.prims += [Prim("sphere", PV.COL_HAND, PV.SEG_HAND, PV.SEG_HAND, c=c, r=r) for (c, r) in hand]
    s.prims += [Prim("capsule", PV.COL_ARM, L, L, arm=L, a=org[L], b=org[L + 1], r=radii[L]) for L in PV.ARM_ORDER]
    return s


def fly_scene(O, rec, obj):
    rec = np.asarray(rec, dtype=np.float64)
    q = rec[_lib.F_Q:_lib.F_Q + 6]; opos = rec[_lib.F_OPOS:_lib.F_OPOS + 3]; oquat = rec[_lib.F_OQUAT:_lib.F_OQUAT + 4]
    s = Scene(); s.task = "fly"; s.table_z = FR.TABLE_Z
    p, qt = O.fk_ur5(q, 6); s.ee = (p, FR._quat_matrix(qt))
    s.table = (153.0, _lib.SEG_TABLE, FR.TABLE); s.none = (_lib.SEG_NONE, FR.BG)
    A, B, Rr, rgb = FR._macro("PIH_UR5_CAP_A"), FR._macro("PIH_UR5_CAP_B"), FR._macro("PIH_UR5_CAP_R"), FR._macro("PIH_UR5_RGB")
    s.prims = []
    for L in range(6):
        p, qt = O.fk_ur5(q, L); R = FR._quat_matrix(qt)
        s.prims.append(Prim("capsule", 255.0 * rgb[L], L, FR.ARM, a=p + R @ A[L], b=p + R @ B[L], r=Rr[L]))
    Ro = FR._quat_matrix(oquat)
    SC, SR = FR._macro("PIH_FLY_OBJ_SPH_C")[obj], FR._macro("PIH_FLY_OBJ_SPH_R")[obj]
    for i in range(int(FR._macro("PIH_FLY_OBJ_NSPH")[obj])):
        s.prims.append(Prim("sphere", 255.0 * FR._macro("PIH_FLY_OBJ_RGB")[obj], _lib.SEG_OBJECT, FR.OBJECT, c=opos + Ro @ SC[i], r=SR[i]))
    return s


def camera_rays(scene, cam, W, H, frame):
    """-> eye, d [H * W, 3], d . f, near, far; cam: 13 words, used as the float32 numbers the C ABI takes; frame: "env", "ee", "ee_pos" """
    cam = np.asarray(cam, dtype=np.float32).astype(np.float64)
    eye, target, up = cam[0:3], cam[3:6], cam[6:9]
    fov, aspect, near, far = cam[9:13]
    pe, Re = scene.ee
    if frame == "ee":
        eye, target, up = pe + Re @ eye, pe + Re @ target, Re @ up
    elif frame == "ee_pos":
        eye, target = pe + eye, pe + target
    f = target - eye; f /= np.linalg.norm(f)
    s = np.cross(f, up); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    T = np.tan(np.radians(fov) / 2)
    xc = (2 * (np.arange(W) + 0.5) / W - 1) * T * aspect
    yc = (1 - 2 * (np.arange(H) + 0.5) / H) * T
    d = f + xc[None, :, None] * s + yc[:, None, None] * u
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d.reshape(-1, 3)
    return eye, d, d @ f, near, far


def occluded(scene, o, l, grow=0.0):
    """does the ray from o [N, 3] towards l hit an occluder at any t > 0?  Every primitive of the scene, no clip planes; the table for a light
    from below"""
    out = np.zeros(len(o), bool)
    if l[2] < 0:
        out |= (scene.table_z - o[:, 2]) / l[2] > 0
    for pr in scene.prims:
        out |= np.isfinite(pr.hit(o, l, grow))
    return out


def tube_normal(ph, grow=0.0):
    """PV._tube_normal for a tube grown by `grow`"""
    hl, ri, ro = float(PV._macro("PIH_HOLE_HALFLEN")) + grow, float(PV._macro("PIH_HOLE_RIN")) - grow, float(PV._macro("PIH_HOLE_ROUT")) + grow
    oc = ph - PV.HOLE_POS; rr = np.sqrt(oc[:, 1] ** 2 + oc[:, 2] ** 2)
    cap = np.abs(oc[:, 0]) >= hl - 1e-5
    k = np.where(rr > 0.5 * (ri + ro), 1.0, -1.0) / np.maximum(rr, 1e-12)
    n = np.stack([np.zeros_like(rr), oc[:, 1] * k, oc[:, 2] * k], -1)
    n[cap] = np.stack([np.where(oc[cap, 0] > 0, 1.0, -1.0), np.zeros(cap.sum()), np.zeros(cap.sum())], -1)
    return n


TABLE_HIT, NO_HIT = -2, -1


def trace(scene, eye, d, df, near, far, H, W, grow=None):
    """nearest hit of the primary rays -> (t [N], inf: none; idx [N]: index into scene.prims, TABLE_HIT or NO_HIT; normals [N, 3]; t and
    normal of the second-nearest hit, on another primitive), in the order and by the rules of the modules' reference_render.  grow=None: the scene as it is, by the modules' ray functions; a number: every
    primitive grown by it, by the ray functions above"""
    N = H * W; d3 = d.reshape(H, W, 3); fly = scene.task == "fly"; g = 0.0 if grow is None else grow
    best = np.full(N, np.inf); idx = np.full(N, NO_HIT); nrm = np.zeros((N, 3)); best2 = np.full(N, np.inf); nrm2 = np.zeros((N, 3))

    def hit_of(pr):
        t = pr.primary(eye, d3, fly) if grow is None else pr.hit(eye, d, g)
        z = t * df
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(t) & (t > 0) & (z >= near) & (z <= far), t, np.inf)

    def take(t, i, normal_of):
        m = t < best
        m2 = ~m & (t < best2)
        if m2.any():
            best2[m2] = t[m2]; nrm2[m2] = normal_of(eye + t[m2][:, None] * d[m2])
        if m.any():
            best2[m] = best[m]; nrm2[m] = nrm[m]
            best[m] = t[m]; idx[m] = i
            nrm[m] = normal_of(eye + t[m][:, None] * d[m])

    with np.errstate(divide="ignore", invalid="ignore"):
        t = (scene.table_z - eye[2]) / d[:, 2]
        z = t * df
        t = np.where(np.isfinite(t) & (t > 0) & (z >= near) & (z <= far), t, np.inf)
    take(t, TABLE_HIT, lambda ph: np.array([0.0, 0.0, 1.0]))
    for i, pr in enumerate(scene.prims):
        if pr.arm is None:
            take(hit_of(pr), i, lambda ph, pr=pr: pr.normal(ph, g))
    arm = [(i, pr) for i, pr in enumerate(scene.prims) if pr.arm is not None]
    if arm:            # the arm's own nearest hit first: sphere links first, a later link takes the pixel only if it is nearer by more than ARM_TIE
        abest = np.full(N, np.inf); alink = np.full(N, -1)
        for i, pr in arm:
            t = hit_of(pr)
            m = t < abest * (1 - PV.ARM_TIE)
            abest[m] = t[m]; alink[m] = pr.arm
        for i, pr in sorted(arm, key=lambda ip: ip[1].arm):
            take(np.where(alink == pr.arm, abest, np.inf), i, lambda ph, pr=pr: pr.normal(ph, g))
    return best, idx, nrm, best2, nrm2


def lit_reference(scene, cam, W, H, frame, light, light_exact=False):
    """the model of include/pih_render_light.h -> dict: img [H, W, 4] = depth value, r, g, b; seg, cls [H, W]; z [H, W] eye-space depth (inf:
    nothing hit); hit, table [H, W] bool; ndl, spec [H, W]; p [H, W, 3] hit points; d [H, W, 3] rays; shadow [H, W] = the pixel's shadow
    state: s of the model is the shadow factor (ndl > 0 and the shadow ray is occluded); decided [H, W]: the state is the same with every
    primitive of the scene grown and shrunk by DELTA, the one the pixel's ray hits included.  light: 11 words, used as the float32 numbers the C ABI takes (light_exact: as the doubles they are -- the modules'
    shaded images have ambient 0.6, not float32(0.6), which is 3e-6 grey levels on the table)"""
    light = np.asarray(light, dtype=np.float64) if light_exact else np.asarray(light, dtype=np.float32).astype(np.float64)
    eye, d, df, near, far = camera_rays(scene, cam, W, H, frame)
    N = H * W
    l = light[L_DIR:L_DIR + 3] / np.linalg.norm(light[L_DIR:L_DIR + 3])

    def state_of(best, idx, nrm, grow):
        hit = idx != NO_HIT
        cand = hit & (nrm @ l > 0)
        st = np.zeros(N, bool)
        p = eye + np.where(hit, best, 0.0)[:, None] * d
        st[cand] = occluded(scene, p[cand] + BIAS * nrm[cand], l, grow)
        return st

    def regrown(best, idx, nrm, grow):
        """hit parameter and normal of every pixel on the primitive it hits, that primitive grown by `grow` (the table stays).  A ray on the
        primitive's silhouette that misses the shrunk one keeps its hit: which primitive owns a pixel is the class rule's business"""
        b2, n2 = best.copy(), nrm.copy()
        for i, pr in enumerate(scene.prims):
            m = np.flatnonzero(idx == i)
            if len(m):
                t = pr.hit(eye, d[m], grow)
                m, t = m[np.isfinite(t)], t[np.isfinite(t)]
                b2[m] = t
                n = pr.normal(eye + t[:, None] * d[m], grow)
                # a normal that jumps is another FACE of the box or the tube (side, end, bore).  Which face a hit lies on is decided by
                # comparisons that fp32 gets right to 1e-7 of the primitive's size, not to DELTA: such a pixel keeps its normal
                same_face = _dot(n, nrm[m]) > 0.9
                n2[m[same_face]] = n[same_face]
        return b2, n2

    best, idx, nrm, best2, nrm2 = trace(scene, eye, d, df, near, far, H, W)
    shadow = state_of(best, idx, nrm, 0.0)
    # a second surface within DELTA behind the hit, facing another way (the seam of two overlapping spheres of an object, a pipe where it lies
    # on the table): which of the two the ray meets first is not decided, and with it the normal that ndl > 0 is asked of.  (Capsules that
    # share an end sphere give the same hit with the same normal: decided.)
    with np.errstate(invalid="ignore"):
        decided = ~((best2 - best < DELTA) & (_dot(nrm, nrm2) < 0.9))
    for grow in (DELTA, -DELTA):
        b2, n2 = regrown(best, idx, nrm, grow)
        decided &= state_of(best, idx, n2, grow) == shadow          # (the normal moves with the primitive; the shadow ray starts where it did)
    hit = idx != NO_HIT
    seg_of = np.array([pr.seg for pr in scene.prims] + [scene.table[1], scene.none[0]]); cls_of = np.array([pr.cls for pr in scene.prims] + [scene.table[2], scene.none[1]])
    base_of = np.array([pr.base for pr in scene.prims] + [np.full(3, scene.table[0]), np.full(3, PV.COL_BG)])
    seg, cls, base = seg_of[idx], cls_of[idx], base_of[idx]          # (TABLE_HIT = -2 and NO_HIT = -1 index the two rows appended last)
    z = best * df
    depth = np.ones(N)
    depth[hit] = far * (z[hit] - near) / (z[hit] * (far - near))
    ndl = nrm @ l
    r = 2 * ndl[:, None] * nrm - l
    x = np.maximum(0.0, -_dot(r, d))
    spec = np.where((ndl > 0) & (x > 0), np.exp2(light[L_SHINE] * np.log2(np.where(x > 0, x, 1.0))), 0.0)
    p = eye + np.where(hit, best, 0.0)[:, None] * d
    s = np.where(shadow, light[L_SHADOW], 1.0)
    direct = s * (light[L_DIF] * np.maximum(0.0, ndl) + light[L_SPEC] * spec)
    rgb = np.minimum(255.0, base * (light[L_AMB] + light[L_COL:L_COL + 3][None, :] * direct[:, None]))
    rgb = np.where(hit[:, None], rgb, base)
    img = np.concatenate([depth[:, None], rgb], -1).reshape(H, W, 4)
    return dict(img=img, seg=seg.reshape(H, W), cls=cls.reshape(H, W), z=np.where(hit, z, np.inf).reshape(H, W), hit=hit.reshape(H, W),
                table=(idx == TABLE_HIT).reshape(H, W), ndl=ndl.reshape(H, W), spec=spec.reshape(H, W), p=p.reshape(H, W, 3), d=d.reshape(H, W, 3),
                shadow=shadow.reshape(H, W), decided=decided.reshape(H, W), l=l)


def class_of_seg(task, seg):
    """the class the comparison rule of the task's module uses, from seg bytes: peg-in-hole: the seg byte; random-fly: BG, TABLE, ARM, OBJECT"""
    if task == "peg":
        return seg
    cls = np.full(seg.shape, FR.ARM)
    cls[seg == _lib.SEG_OBJECT] = FR.OBJECT; cls[seg == _lib.SEG_TABLE] = FR.TABLE; cls[seg == _lib.SEG_NONE] = FR.BG
    return cls


def check_image(ref, task, render, light, exact):
    """The comparison rules, for the host builds and the GPU.  render(light words) -> (float4 image [H, W, 4], seg bytes [H, W]).
    -> (colour errors on the compared pixels, share of pixels whose class differs).  Asserts the class rule and the shadow rule."""
    img, seg = render(light)
    img = np.asarray(img, dtype=np.float64)
    same = class_of_seg(task, seg) == ref["cls"]
    if exact:
        assert same.all(), "%d pixels differ in class" % (~same).sum()
    else:
        assert (~same).mean() <= CLASS_SHARE, "%.4f of the pixels differ in class" % (~same).mean()
    assert (img[..., 0][same & ~ref["hit"]] == 1.0).all()
    a, _ = render(probe_light(light, 0.5)); b, _ = render(probe_light(light, 1.0))
    state = (np.asarray(a)[..., 1:] != np.asarray(b)[..., 1:]).any(-1)
    use = same & ref["decided"]
    wrong = use & (state != ref["shadow"])
    if wrong.any():
        i, j = np.argwhere(wrong)[0]
        raise AssertionError("%d decided pixels have the wrong shadow state, the first at (%d, %d): seg %d, reference state %s with ndl %.3e, probe pixels %r and %r"
                             % (wrong.sum(), i, j, ref["seg"][i, j], ref["shadow"][i, j], ref["ndl"][i, j], np.asarray(a)[i, j].tolist(), np.asarray(b)[i, j].tolist()))
    return np.abs(img[..., 1:] - ref["img"][..., 1:])[use].reshape(-1), (~same).mean()


# ------------------------------------------------------------------------------------------------ host builds
@pytest.fixture(scope="module")
def host_builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("lit_emul")
    libs = {}
    dp, fp, bp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    for prec, real in (("f64", "double"), ("f32", "float")):
        so = str(d / ("libpih_lit_%s.so" % prec))
        subprocess.check_call(["g++"] + PV.CXXFLAGS + ["-DPIH_REAL=" + real, "-shared", "-o", so, os.path.join(ROOT, "tests", "emul", "pih_lit_emul.cpp")])
        L = C.CDLL(so)
        L.pihl_view_render.argtypes = [dp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, dp, bp, dp]
        L.pihl_fly_render.argtypes = [dp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, bp, dp]
        L.pihl_pack_byte.argtypes = [C.c_double]
        L.pihl_light_degenerate.argtypes = [fp, C.POINTER(C.c_char_p)]
        assert L.pihl_real_bytes() == (8 if prec == "f64" else 4)
        libs[prec] = L
    return libs


def host_render(L, case, light, lcull=True, expect=0, cam=None):
    """-> (float4 image [H, W, 4], rgba8 [H, W, 4] uint8, depth [H, W]) of the host build for a case of `cases`"""
    dp, fp, bp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    W, H = case["size"]
    rec = np.ascontiguousarray(case["rec"], dtype=np.float64); cam = np.ascontiguousarray(case["cam"] if cam is None else cam, dtype=np.float32)
    light = np.ascontiguousarray(light, dtype=np.float32)
    assert cam.shape == (_lib.CAM_WORDS,) and light.shape == (_lib.LIGHT_WORDS,)
    out = np.zeros((H, W, 4)); rgba = np.zeros((H, W, 4), dtype=np.uint8); depth = np.zeros((H, W))
    args = (W, H, case["flags"], int(lcull), out.ctypes.data_as(dp), rgba.ctypes.data_as(bp), depth.ctypes.data_as(dp))
    if case["task"] == "peg":
        rc = L.pihl_view_render(rec.ctypes.data_as(dp), cam.ctypes.data_as(fp), light.ctypes.data_as(fp), *args)
    else:
        rc = L.pihl_fly_render(rec.ctypes.data_as(dp), cam.ctypes.data_as(fp), light.ctypes.data_as(fp), case["obj"], *args)
    assert rc == expect, rc
    return out, rgba, depth


# The cap on undecided pixels is a condition on the scene.  The two cameras that ride on the hand miss it in the two states that bring
# the hand down to the table: one pixel covers 0.4 mm of it there, a shadow edge moves by DELTA / l.z = 0.12 mm (default light) to 0.5 mm
# (low light) between the grown and the shrunk occluders, so most pixels ALONG an edge are undecided -- measured on the reference: wrist
# preset, scripted state 4: 0.0083 of the 64 x 64 image (default light); wrist, state 5 (40 random steps): 0.0092 (low light); eye-in-hand,
# state 5: 0.0066 (low light).  The cap stays; for these three pairs the scene changes: they take one of two further reset states, 6 and 7
# (largest share there: 0.0017).  Every other camera sees all six states.
PEG_STATE_FOR = {("wrist", 4): 6, ("wrist", 5): 7, ("eye-in-hand", 5): 7}


def make_peg_states(O):
    """float32 [8, 256]: the six states of tests/test_peg_view.py and two more resets (PEG_STATE_FOR)"""
    six = PV.make_states(O)
    more = np.zeros((2, _lib.STATE_WORDS), dtype=np.float32)
    for i, seed in enumerate((14, 15)):
        more[i, :O.STATE_WORDS] = O.Oracle(1, seed=seed).get_state()[0]
    return np.concatenate([six, more])


def peg_cases(O, peg_states, names=PV.CAMERA_NAMES):
    """{key: case} of the peg-in-hole task: the six state slots x the cameras `names` x the three sizes.  case: task, rec, cam, frame, flags,
    size, obj, scene, name, env (the row of peg_states [8, 256] the slot takes, PEG_STATE_FOR)"""
    cases = {}
    scenes = {}
    for k in range(6):
        for name in names:
            env = PEG_STATE_FOR.get((name, k), k)
            if env not in scenes:
                scenes[env] = peg_scene(O, peg_states[env])
            for (W, H) in SIZES:
                cam, frame = PV.cameras(W, H)[name]
                cases[("peg", name, (W, H), k)] = dict(task="peg", rec=peg_states[env], cam=cam, frame=frame, flags=PV.FRAME_FLAG[frame], size=(W, H), obj=None, scene=scenes[env],
                                                       name=name, env=env)
    return cases


def fly_cases(O, obj, name, recs):
    """{key: case} of the random-fly task: the states recs [k, 48] of object `obj` under camera `name` x the three sizes"""
    cases = {}
    for k, rec in enumerate(recs):
        scene = fly_scene(O, rec, obj)
        for (W, H) in SIZES:
            cam, ee = FR.cameras(W, H)[name]
            cases[("fly%d" % obj, name, (W, H), k)] = dict(task="fly", rec=rec, cam=cam, frame="ee" if ee else "env", flags=_lib.RENDER_CAM_EE if ee else 0, size=(W, H),
                                                          obj=obj, scene=scene, name=name, env=k)
    return cases


def make_cases(O):
    """all cases of this module: peg_cases of make_peg_states, and two fly states per object and camera (the states of tests/test_fly_render.py)"""
    cases = peg_cases(O, make_peg_states(O))
    for obj in FR.OBJECTS:
        for ci, name in enumerate(FR.CAMERA_NAMES):
            cases.update(fly_cases(O, obj, name, FR.make_states(O, obj, 2, seed=100 + 10 * obj + ci, eye_in_hand=name == "eye-in-hand")))
    return cases


def case_reference(case, light, light_exact=False):
    W, H = case["size"]
    return lit_reference(case["scene"], case["cam"], W, H, case["frame"], light, light_exact)


@pytest.fixture(scope="module")
def cases(oracle_mod):
    return make_cases(oracle_mod)


@pytest.fixture(scope="module")
def references(cases):
    """{(case key, light name): reference}, computed once for the module"""
    return {(key, ln): case_reference(case, LIGHTS[ln]) for key, case in cases.items() for ln in LIGHT_NAMES}


# ------------------------------------------------------------------------------------------------ 1. the reference
def test_ray_functions_are_the_modules(oracle_mod, cases):
    """the per-ray-origin ray functions above == the ray functions of tests/test_peg_view.py, on the primary rays of the overview and the
    hole close-up: same hits, same ray parameters"""
    for name in ("overview", "hole close-up"):
        case = cases[("peg", name, (97, 61), 0)]
        W, H = case["size"]
        eye, d, _, _, _ = camera_rays(case["scene"], case["cam"], W, H, case["frame"])
        d3 = d.reshape(H, W, 3)
        for pr in case["scene"].prims:
            p = pr.p
            want = {"capsule": lambda: PV._ref_capsule(eye, d3, p["a"], p["b"], p["r"]), "sphere": lambda: PV._ref_sphere(eye - p["c"], d3, p["r"]),
                    "box": lambda: PV._ref_box(eye, d3, p["R"], p["c"], p["h"]), "tube": lambda: PV._ref_tube(eye, d3)}[pr.kind]()
            got = pr.hit(np.broadcast_to(eye, d.shape), d).reshape(H, W)
            assert np.array_equal(np.isfinite(got), np.isfinite(want)), (name, pr.kind)
            m = np.isfinite(want)
            assert not m.any() or np.abs(got[m] - want[m]).max() <= 1e-12, (name, pr.kind)


def test_reference_reproduces_the_shaded_images(oracle_mod, cases):
    """Anchor: with specular 0 and shadow factor 1 the lit reference is the shaded image of the two modules' reference_render within 1e-9,
    for every state, camera and size; classes and eye-space depths are theirs."""
    off = list(_lib.LIGHT_DEFAULT); off[L_SPEC] = 0.0; off[L_SHADOW] = 1.0
    for key, case in cases.items():
        W, H = case["size"]
        ref = case_reference(case, off, light_exact=True)
        if case["task"] == "peg":
            _, lit, seg, z = PV.reference_render(oracle_mod, case["rec"], case["cam"], W, H, case["frame"])
            assert np.array_equal(ref["seg"], seg), key
        else:
            _, lit, cls, z = FR.reference_render(oracle_mod, case["rec"], case["cam"], case["obj"], W, H, case["frame"] == "ee")
            assert np.array_equal(ref["cls"], cls), key
        assert np.abs(ref["img"] - lit).max() <= 1e-9, (key, np.abs(ref["img"] - lit).max())
        fin = np.isfinite(z)
        assert np.array_equal(np.isfinite(ref["z"]), fin) and np.abs(ref["z"][fin] - z[fin]).max(initial=0.0) <= 1e-9


def test_reference_scenes_are_worth_comparing(cases, references):
    """Conditions on the REFERENCE alone.  At most UNDECIDED_CAP of an image is undecided.  Every (camera, light) pair meant to show shadows
    has at least SHADOW_SHARE of the image shadowed -- SHADOWS names the pairs; a light from below shadows every lit surface above the
    table and leaves the table ambient only.  Under the wrist preset the arm owns no pixel and still shadows at least 1 % of the table."""
    worst = 0.0
    for (key, ln), ref in references.items():
        und = (~ref["decided"]).mean()
        worst = max(worst, und)
        assert und <= UNDECIDED_CAP, (key, ln, und)
        task, name, size, k = key
        if ln == "below":
            lit_side = ref["hit"] & (ref["ndl"] > 0)
            assert (ref["shadow"] == lit_side).all() and not (ref["table"] & lit_side).any()
            amb = float(np.float32(LIGHTS[ln][L_AMB])) * (PV.COL_TABLE if task == "peg" else 153.0)
            assert not ref["table"].any() or np.abs(ref["img"][..., 1:][ref["table"]] - amb).max() <= 1e-9
        elif ln in SHADOWS.get((task[:3], name), ()):
            assert ref["shadow"].mean() >= SHADOW_SHARE, (key, ln, ref["shadow"].mean())
        if task == "peg" and name == "wrist" and ln == "default":
            assert not (ref["seg"] <= 6).any()
            assert ref["table"].any() and (ref["shadow"] & ref["table"]).sum() >= 0.01 * ref["table"].sum(), (key, (ref["shadow"] & ref["table"]).sum(), ref["table"].sum())
    print("largest undecided share of an image: %.5f (cap %.3f)" % (worst, UNDECIDED_CAP))


# the (camera, light) pairs that are meant to show shadows.  Not among them: the low light with the wrist preset (its shadows fall outside the
# image) and with the two horizon cameras (the arm's long shadow leaves the table's near part); the fly task's eye-in-hand camera, which
# looks away from the arm at the object in mid-air
_ABOVE = ("default", "low", "shiny")
SHADOWS = {("peg", "overview"): _ABOVE, ("peg", "hole close-up"): _ABOVE, ("peg", "eye-in-hand"): _ABOVE, ("peg", "wrist"): ("default", "shiny"), ("peg", "horizon"): ("default", "shiny"),
           ("fly", "overview"): _ABOVE, ("fly", "close-up"): _ABOVE, ("fly", "horizon"): ("default", "shiny")}


# ------------------------------------------------------------------------------------------------ 2. known answers, no ray caster involved
def _straight_down(x, y, h, table_z, fov=50.0):
    return [x, y, table_z + h, x, y, table_z, 0, 1, 0, fov, 1, 0.01, 100]


@pytest.mark.parametrize("prec", ["ref", "f64"])
def test_highlight_on_the_table_in_closed_form(oracle_mod, host_builds, prec):
    """Light (0, 0, 1), a camera looking straight down at the table: the mirrored light is (0, 0, 1), so spec of a table pixel is
    cos(angle of its ray to the vertical) ** shininess.  With ambient 0, diffuse 0, specular 1, colour 1 and no shadows the pixel is
    table colour x that."""
    rec = FR.make_states(oracle_mod, 0, 1, seed=100)[0]
    shine = 8.0
    light = [0, 0, 1, 1, 1, 1, 0, 0, 1, shine, 1]
    W, H = 40, 30
    cam = _straight_down(0.3, -0.9, 1.0, FR.TABLE_Z)
    case = dict(task="fly", rec=rec, cam=cam, frame="env", flags=0, size=(W, H), obj=0, scene=fly_scene(oracle_mod, rec, 0))
    ref = case_reference(case, light)
    assert ref["table"].mean() > 0.5
    T = np.tan(np.radians(cam[9]) / 2)
    xc = (2 * (np.arange(W) + 0.5) / W - 1) * T; yc = (1 - 2 * (np.arange(H) + 0.5) / H) * T
    cos = 1.0 / np.sqrt(1 + xc[None, :] ** 2 + yc[:, None] ** 2)
    want = 153.0 * cos ** shine
    assert want.min() < 0.5 * want.max()                     # the highlight falls off across the image
    if prec == "ref":
        img, table = ref["img"], ref["table"]
    else:
        out, rgba, _ = host_render(host_builds[prec], case, light)
        img, table = out, rgba[..., 3] == _lib.SEG_TABLE
        assert np.array_equal(table, ref["table"])
    for c in (1, 2, 3):
        assert np.abs(img[..., c] - want)[table].max() <= 1e-9


def _object_above_the_table(O, obj=0):
    rec = FR.make_states(O, obj, 1, seed=100)[0].astype(np.float64)
    rec[_lib.F_OPOS:_lib.F_OPOS + 3] = [0.45, -0.55, 0.3]          # held above the table, clear of the arm's footprint
    return rec.astype(np.float32)


@pytest.mark.parametrize("prec", ["ref", "f64"])
def test_object_shadow_on_the_table_in_closed_form(oracle_mod, host_builds, prec):
    """Light (0, 0, 1), shadow factor 0.5: a table pixel is shadowed exactly when its hit point's (x, y) lies within r_i of some object
    sphere's centre or inside an arm capsule's footprint (within r of the projected segment) -- every sphere and capsule lies above the
    table.  Tested on the pixels farther than 1e-4 m from those outlines; both kinds of pixel exist."""
    obj = 0
    rec = _object_above_the_table(oracle_mod, obj)
    scene = fly_scene(oracle_mod, rec, obj)
    light = [0, 0, 1, 1, 1, 1, 0.6, 0.35, 0.0, 2, 0.5]
    W, H = 97, 61
    cam = [1.4, -1.2, 1.6, 0.3, -0.3, 0.0, 0, 0, 1, 45, W / H, 0.01, 100]
    case = dict(task="fly", rec=rec, cam=cam, frame="env", flags=0, size=(W, H), obj=obj, scene=scene)
    ref = case_reference(case, light)
    # the hit point of a table pixel in closed form: the ray scaled to the table's height
    eye, d, _, _, _ = camera_rays(scene, cam, W, H, "env")
    t = (FR.TABLE_Z - eye[2]) / d[:, 2]
    xy = (eye + t[:, None] * d)[:, :2].reshape(H, W, 2)
    margin = np.full((H, W), np.inf)              # signed distance to the nearest outline: < 0 inside a footprint
    for pr in scene.prims:
        if pr.kind == "sphere":
            assert pr.p["c"][2] - pr.p["r"] > FR.TABLE_Z
            dist = np.linalg.norm(xy - pr.p["c"][:2], axis=-1) - pr.p["r"]
        else:
            a, b = pr.p["a"], pr.p["b"]
            assert min(a[2], b[2]) - pr.p["r"] > FR.TABLE_Z
            ab = b[:2] - a[:2]
            q = np.clip(((xy - a[:2]) @ ab) / max(ab @ ab, 1e-30), 0, 1)
            dist = np.linalg.norm(xy - (a[:2] + q[..., None] * ab), axis=-1) - pr.p["r"]
        margin = np.minimum(margin, dist)
    if prec == "ref":
        table, state = ref["table"], ref["shadow"]
    else:
        L = host_builds[prec]
        a, rgba, _ = host_render(L, case, light); b, _, _ = host_render(L, case, light[:10] + [1.0])
        table, state = rgba[..., 3] == _lib.SEG_TABLE, (a[..., 1:] != b[..., 1:]).any(-1)
        assert np.array_equal(table, ref["table"])
    clear = table & (np.abs(margin) > 1e-4)
    want = margin < 0
    assert (want & clear).sum() >= 20 and (~want & clear).sum() >= 1000, ((want & clear).sum(), (~want & clear).sum())
    assert np.array_equal(state[clear], want[clear])
    # and the object's own shadow is among them
    near_obj = np.linalg.norm(xy - rec[_lib.F_OPOS:_lib.F_OPOS + 2].astype(np.float64), axis=-1) < 0.02
    assert (near_obj & clear & state).any()


# ------------------------------------------------------------------------------------------------ 3. host builds against the reference
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_host_build_matches_the_reference(host_builds, cases, references, prec):
    """All six peg states and the fly states of both objects, every camera of the two modules, the three sizes, the four lights.  Class rule
    of the modules; shadow state equal on every decided pixel; images with and without the light-space cull bit-identical in all three
    formats; colour on the decided pixels: fp64 <= 1e-6, fp32 the project's bar for shaded colours times 1 + specular shininess / diffuse
    of the light.  The fp32 maxima are printed: they are the yardstick of the GPU test."""
    L = host_builds[prec]
    worst_share = 0.0
    for ln in LIGHT_NAMES:
        light = LIGHTS[ln]; errs = []
        for key, case in cases.items():
            ref = references[(key, ln)]
            full = host_render(L, case, light, lcull=False)
            culled = host_render(L, case, light, lcull=True)
            for a, b in zip(full, culled):
                assert np.array_equal(a, b), (key, ln, int((a != b).sum()))
            err, share = check_image(ref, case["task"], lambda lw: (lambda r: (r[0], r[1][..., 3]))(host_render(L, case, lw)), light, exact=prec == "f64")
            errs.append(err); worst_share = max(worst_share, share)
        errs = np.concatenate(errs); f = colour_factor(light)
        print("%s host build, light %-8s: colour error max %.3e, p99 %.3e, median %.3e (bounds x %.2f); worst class share %.4f"
              % (prec, ln, errs.max(), np.percentile(errs, 99), np.median(errs), f, worst_share))
        if prec == "f64":
            assert errs.max() <= 1e-6
        else:
            assert np.percentile(errs, 99) < SHADED_P99 * f and np.median(errs) < SHADED_MEDIAN * f


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_packed_formats_of_the_host_build(host_builds, cases, references, prec):
    """rgba8 bytes == pack_byte of the float4 colours; the seg byte == the unlit call's (the reference's, in fp64); depth-only == channel 0
    and does not depend on the light"""
    L = host_builds[prec]
    real = np.float64 if prec == "f64" else np.float32
    for v, want in ((178.5, 179), (0.0, 0), (0.49, 0), (254.5, 255), (255.0, 255), (300.0, 255)):
        assert L.pihl_pack_byte(v) == want
    for key, case in cases.items():
        if case["size"] != (97, 61) or key[3] != 0:
            continue
        depths = []
        for ln in LIGHT_NAMES:
            img, rgba, depth = host_render(L, case, LIGHTS[ln])
            want = np.minimum(255, (img[..., 1:].astype(real) + real(0.5)).astype(np.int64))
            assert np.array_equal(rgba[..., :3], want.astype(np.uint8)), (key, ln)
            assert np.array_equal(depth, img[..., 0])
            depths.append(depth)
            if prec == "f64":
                assert np.array_equal(rgba[..., 3], references[(key, ln)]["seg"]), (key, ln)
        assert all(np.array_equal(depths[0], d) for d in depths[1:])
    # a bright light saturates: min(255, .)
    case = cases[("peg", "overview", (40, 30), 0)]
    img, rgba, _ = host_render(L, case, [0, 0, 1, 3, 3, 3, 0.6, 1.0, 0.0, 2, 1])
    assert img[..., 1:].max() == 255.0 and (img[..., 1:] == 255.0).mean() > 0.3


BAD_LIGHTS = (
    ("direction", 0, [0.0, 0.0, 0.0] + _D[3:]), ("direction", 1, _D[:1] + [float("inf")] + _D[2:]),
    ("colour", 4, _D[:4] + [-0.1] + _D[5:]), ("ambient", 6, _D[:6] + [-1.0] + _D[7:]), ("diffuse", 7, _D[:7] + [float("nan")] + _D[8:]),
    ("specular", 8, _D[:8] + [-0.5] + _D[9:]), ("shininess", 9, _D[:9] + [0.0] + _D[10:]), ("shadow factor", 10, _D[:10] + [1.5]), ("shadow factor", 10, _D[:10] + [-0.1]),
)


def test_degenerate_lights(host_builds, cases):
    """each field in turn: the validity function names it, and a light the kernel tests itself (a device row) gives the background in every
    format; the default and the four test lights are valid"""
    L = host_builds["f32"]
    fp = C.POINTER(C.c_float)
    for ln in LIGHT_NAMES:
        assert L.pihl_light_degenerate(np.array(LIGHTS[ln], dtype=np.float32).ctypes.data_as(fp), None) == 0
    codes = set()
    for field, _, words in BAD_LIGHTS:
        what = C.c_char_p()
        code = L.pihl_light_degenerate(np.array(words, dtype=np.float32).ctypes.data_as(fp), C.byref(what))
        assert code > 0 and what.value.decode().startswith(field), (field, code, what.value)
        codes.add(code)
        for key in (("peg", "overview", (40, 30), 0), ("fly0", "overview", (40, 30), 0)):
            img, rgba, depth = host_render(L, cases[key], words, expect=16 * code)
            assert (img[..., 0] == 1).all() and (img[..., 1:] == 255).all() and (depth == 1).all()
            assert (rgba[..., :3] == 255).all() and (rgba[..., 3] == _lib.SEG_NONE).all()
    assert codes == set(range(1, 8))


def test_light_validity_survives_fast_math(tmp_path):
    """The library compiles light_degenerate with clang -O3 -ffast-math, on the host too, where a bit test on a float VALUE is folded to
    "finite" and `!(x >= 0)` to `x < 0`: a NaN coefficient once passed the host's test.  The same file under those flags: a NaN or an
    infinity in each of the 11 words is refused, under the field's code."""
    import __graft_entry__  # noqa: F401  (the compiler of the library)
    from peg_in_hole_gym_amd.csrc import build as B
    so = str(tmp_path / "libpih_lit_fast.so")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", "-O3", "-ffast-math", "-std=c++17", "-fPIC", "-shared", "-w", "-DPIH_REAL=float", "-o", so,
                           os.path.join(ROOT, "tests", "emul", "pih_lit_emul.cpp")])
    assert "-ffast-math" in B.FLAGS and "-O3" in B.FLAGS
    L = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    L.pihl_light_degenerate.argtypes = [fp, C.POINTER(C.c_char_p)]
    want = [1, 1, 1, 2, 2, 2, 3, 4, 5, 6, 7]
    for i in range(_lib.LIGHT_WORDS):
        for v in (float("nan"), float("inf"), -float("inf")):
            w = list(_D); w[i] = v
            assert L.pihl_light_degenerate(np.array(w, dtype=np.float32).ctypes.data_as(fp), None) == want[i], (i, v)
    assert L.pihl_light_degenerate(np.array(_D, dtype=np.float32).ctypes.data_as(fp), None) == 0
    for field, _, words in BAD_LIGHTS:
        what = C.c_char_p()
        assert L.pihl_light_degenerate(np.array(words, dtype=np.float32).ctypes.data_as(fp), C.byref(what)) > 0 and what.value.decode().startswith(field)


# ------------------------------------------------------------------------------------------------ 4. header, constants, plumbing
def test_light_constants_match_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "pih.h"\nint main(void) {\n  static const float d[] = PIH_LIGHT_DEFAULT;\n'
                   '  printf("%d %d %d %d %.9g\\n", PIH_ABI_VERSION, PIH_LIGHT_WORDS, PIH_RENDER_LIGHT_DEVICE, (int)(sizeof d / sizeof d[0]), (double)PIH_SHADOW_BIAS);\n'
                   '  for (int i = 0; i < PIH_LIGHT_WORDS; i++) printf("%.9g\\n", d[i]);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    abi, words, dev, count = [int(x) for x in lines[0].split()[:4]]
    assert abi == _lib.ABI_VERSION == 4 and words == count == _lib.LIGHT_WORDS == 11 and dev == _lib.RENDER_LIGHT_DEVICE == 64
    assert float(lines[0].split()[4]) == BIAS
    vals = np.array([float(x) for x in lines[1:12]])
    assert isinstance(_lib.LIGHT_DEFAULT, tuple) and np.array_equal(vals.astype(np.float32), np.array(_lib.LIGHT_DEFAULT, dtype=np.float32))
    assert _lib.LIGHT_DEFAULT == (-50, 30, 100, 1, 1, 1, 0.6, 0.35, 0.05, 2, 0.8)
    # the direction and the two coefficients are those of the fixed light of PIH_RENDER_SHADED
    assert np.allclose(np.array(_lib.LIGHT_DEFAULT[:3]) / np.linalg.norm(_lib.LIGHT_DEFAULT[:3]), PV.LIGHT, atol=1e-15) and _lib.LIGHT_DEFAULT[6:8] == (PV.AMBIENT, PV.DIFFUSE)
    names = sorted(set(re.findall(r"\b(pih_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "pih_render_light.h")).read())))
    assert names == sorted(_lib.LIGHT_EXPORTS) == ["pih_render_lit"] and not set(names) & set(_lib.EXPORTS) and not set(names) & set(_lib.VIEW_EXPORTS)
    assert '#include "pih_render_light.h"' in open(os.path.join(ROOT, "include", "pih.h")).read()
    bits = [_lib.RENDER_SHADED, _lib.RENDER_CAM_EE, _lib.RENDER_OUT_RGBA8, _lib.RENDER_OUT_DEPTH, _lib.RENDER_CAM_DEVICE, _lib.RENDER_CAM_EE_POS, _lib.RENDER_LIGHT_DEVICE]
    assert sorted(bits) == [1, 2, 4, 8, 16, 32, 64]


def test_library_exports_the_lit_camera():
    import __graft_entry__ as ge
    ge.build()
    L = C.CDLL(os.path.join(ROOT, "peg_in_hole_gym_amd", "csrc", "libpih_hip.so"))
    assert hasattr(L, "pih_render_lit")


class _FakeLib:
    """records the C calls PihVecEnv.render / render_view make"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _vec_env(task_id):
    """a PihVecEnv that never touches a GPU: the attributes render() and render_view() use, a recording library"""
    import torch
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    g = PihVecEnv.__new__(PihVecEnv)
    g.n, g.task_id, g.device, g.h, g.L = 4, task_id, torch.device("cpu"), None, _FakeLib()
    g._stream = lambda: None
    g._chk = lambda rc, what: None
    return g


def test_light_none_takes_todays_calls_and_a_wrong_length_raises(monkeypatch):
    import contextlib
    import torch
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())      # (no GPU here: the calls go to the recording library)
    peg, fly = _vec_env(_lib.TASK_PEG_IN_HOLE), _vec_env(_lib.TASK_RANDOM_FLY)
    peg.render_view(8, 6, shaded=True, frame="ee", fmt="rgba8", light=None); peg.render_view(8, 6, shaded=True, frame="ee", fmt="rgba8")
    fly.render(8, 6, shaded=True, ee_frame=True, light=None); fly.render(8, 6, shaded=True, ee_frame=True)
    for g, name, nargs in ((peg, "pih_render_view", 9), (fly, "pih_render_cam", 9)):
        (n0, a0), (n1, a1) = g.L.calls
        assert n0 == n1 == name and len(a0) == len(a1) == nargs and a0[2:] == a1[2:]
    assert peg.L.calls[0][1][2:] == (None, 8, 6, 0, 4, _lib.RENDER_SHADED | _lib.RENDER_CAM_EE | _lib.RENDER_OUT_RGBA8, None)
    assert fly.L.calls[0][1][2:] == (None, 8, 6, 0, 4, _lib.RENDER_SHADED | _lib.RENDER_CAM_EE, None)
    # a light takes the new entry point: "default" passes NULL, 11 numbers a host array, [count, 11] a device address with the flag
    peg.L.calls.clear()
    peg.render_view(8, 6, light="default"); peg.render_view(8, 6, light=list(LIGHTS["shiny"])); peg.render_view(8, 6, env_begin=1, env_count=2, light=np.tile(LIGHTS["low"], (2, 1)))
    assert [c[0] for c in peg.L.calls] == ["pih_render_lit"] * 3
    (_, a), (_, b), (_, c) = peg.L.calls
    assert a[3] is None and a[8] == _lib.RENDER_SHADED and list(b[3]) == [np.float32(x) for x in LIGHTS["shiny"]] and b[8] == _lib.RENDER_SHADED
    assert c[3].value == peg._light_keep.data_ptr() and c[8] == _lib.RENDER_SHADED | _lib.RENDER_LIGHT_DEVICE and c[4:8] == (8, 6, 1, 2) and tuple(peg._light_keep.shape) == (2, 11)
    fly.L.calls.clear()
    fly.render(8, 6, light="default", fmt="depth")
    assert fly.L.calls[0][0] == "pih_render_lit" and fly.L.calls[0][1][8] == _lib.RENDER_SHADED | _lib.RENDER_OUT_DEPTH
    for g, f in ((peg, peg.render_view), (fly, fly.render)):
        with pytest.raises(ValueError):
            f(8, 6, light=[0, 0, 1, 1, 1, 1, 0.6, 0.35, 0.05, 2])               # 10 numbers
        with pytest.raises(ValueError):
            f(8, 6, light=np.zeros((4, 10)))
        with pytest.raises(ValueError):
            f(8, 6, light=np.tile(_D, (3, 1)))                                   # 3 rows for 4 envs
        with pytest.raises(ValueError):
            f(8, 6, light="bright")
    with pytest.raises(ValueError):
        peg.render(8, 6, light="default")                                        # the wrist camera of render() takes none


class _FakeBackend:
    def __init__(self, n, offsets, **cfg):
        self.n, self.cfg, self.calls = n, cfg, []

    def reset(self, mask=None, hard_reset=False):
        pass

    def render(self, width=300, height=300, **kw):
        self.calls.append(dict(width=width, height=height, **kw))
        return np.full((self.n, height, width, 4), 7.0, dtype=np.float32)

    def render_view(self, **kw):
        self.calls.append(kw)
        return "image"


def test_facades_forward_the_light():
    from peg_in_hole_gym_amd.envs.peg_in_hole import PegInHole, RandomFly
    t = RandomFly(args=["Banana", 1 / 120.], backend_factory=_FakeBackend)
    t.render()
    assert t._backend.calls[-1] == dict(width=300, height=300, shaded=True, camera=None, ee_frame=False)          # today's call, no new keyword
    t.render(light="default")
    assert t._backend.calls[-1] == dict(width=300, height=300, shaded=True, camera=None, ee_frame=False, light="default")
    p = PegInHole(backend_factory=_FakeBackend)
    assert p.render_view(light=list(LIGHTS["low"]), fmt="rgba8") == "image" and p._backend.calls == [dict(light=list(LIGHTS["low"]), fmt="rgba8")]


def test_random_lights_on_the_host():
    """the draw itself is plain torch: valid rows, unit directions inside the elevation range, reproducible with a generator"""
    import torch
    from peg_in_hole_gym_amd.vec_env import random_lights
    gen = torch.Generator().manual_seed(3)
    a = random_lights(64, "cpu", gen, (20, 80)).numpy()
    b = random_lights(64, "cpu", torch.Generator().manual_seed(3), (20, 80)).numpy()
    assert a.shape == (64, 11) and a.dtype == np.float32 and np.array_equal(a, b)
    assert np.allclose(np.linalg.norm(a[:, :3], axis=1), 1, atol=1e-6) and np.array_equal(a[:, 3:], np.tile(np.array(_lib.LIGHT_DEFAULT[3:], dtype=np.float32), (64, 1)))
    el = np.degrees(np.arcsin(a[:, 2]))
    assert el.min() >= 20 - 1e-3 and el.max() <= 80 + 1e-3 and el.max() - el.min() > 30 and np.ptp(np.arctan2(a[:, 1], a[:, 0])) > 4
    with pytest.raises(ValueError):
        random_lights(4, "cpu", None, (80, 20))
