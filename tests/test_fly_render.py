"""Free camera of the 'random-fly' task (pih_render_cam, peg_in_hole_gym_amd/csrc/pih_fly_render.h), CPU part: the product's per-scene
and per-pixel code, compiled on the host in fp64 and fp32 (tests/emul/pih_fly_render_emul.cpp), against a numpy fp64 ray caster
written here from the camera and image semantics of include/pih.h; the constants of the ABI, the model table and the facade.
The GPU part is tests/test_gpu_fly_render.py, which takes the reference, the scenes and the comparison rules from this module."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REST = np.array([0, -np.pi / 2, np.pi / 2, -np.pi / 2, -np.pi / 2, 0])
P0 = np.array([0.45, 0.1, 0.55])
TABLE_Z = -0.05
SIZES = ((97, 61), (64, 64), (40, 30))          # (W, H): two tile columns, the second partial, rows no multiple of 16 | one tile column | narrower than a wave
OBJECTS = (0, 1)                                # Banana (5 spheres), Amicelli (2)
LIGHT = np.array([-50.0, 30.0, 100.0]) / np.linalg.norm([-50.0, 30.0, 100.0])
AMBIENT, DIFFUSE = 0.6, 0.35
BG, TABLE, ARM, OBJECT = 0, 1, 2, 3             # pixel classes
CLASS_SHARE = 0.003                             # share of an image's pixels that may differ in class (silhouette rays in fp32; tests/test_render.py)


def cameras(W, H):
    """name -> (13 camera words, ee_frame)"""
    return {
        "overview": (list(_lib.FLY_CAM_DEFAULT), False),
        "close-up": (list(P0 + [0.25, 0.15, 0.2]) + list(P0) + [0, 0, 1, 60, 1, 0.01, 100], False),
        "horizon": ([1.6, 0, 0.5, 0, 0, 0.5, 0, 0, 1, 60, W / H, 0.01, 100], False),
        "eye-in-hand": ([0.05, 0, 0, 1.05, 0, 0, 0, 1, 0, 60, 1, 0.01, 100], True),
    }


CAMERA_NAMES = ("overview", "close-up", "horizon", "eye-in-hand")


# ------------------------------------------------------------------------------------------------ model tables, from the header
def _macro(name):
    hdr = open(os.path.join(ROOT, "include", "pih_model.h")).read()
    return np.array(eval(re.search(r"#define %s (.*)" % name, hdr).group(1).split("/*")[0].replace("{", "[").replace("}", "]")), dtype=float)


def _quat_matrix(q):
    qx, qy, qz, qw = q
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                     [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                     [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])


# ------------------------------------------------------------------------------------------------ scenes
def make_states(O, obj, n, seed, eye_in_hand=False):
    """float32 [n, 48] records: q = REST + U(-0.6, 0.6) per joint, a random unit object quaternion, the object at P0 -- or, for the
    eye-in-hand camera, 0.35 m in front of the ee frame.  Rounded to float32 here, so every build and the reference see the same numbers."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, _lib.FLY_STATE_WORDS))
    for e in range(n):
        q = (REST + rng.uniform(-0.6, 0.6, 6)).astype(np.float32).astype(np.float64)
        oq = rng.normal(size=4); oq /= np.linalg.norm(oq)
        s[e, _lib.F_Q:_lib.F_Q + 6] = q; s[e, _lib.F_TARGET:_lib.F_TARGET + 6] = q
        s[e, _lib.F_OQUAT:_lib.F_OQUAT + 4] = oq
        pos = P0
        if eye_in_hand:
            p, qt = O.fk_ur5(q, 6)
            pos = p + _quat_matrix(qt) @ np.array([0.35, 0.0, 0.0])
        s[e, _lib.F_OPOS:_lib.F_OPOS + 3] = pos
    return s.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the reference
def _ref_sphere(o, d, c, r):
    oc = o - c
    b = d @ oc; disc = b * b - (oc @ oc - r * r)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    return np.where((disc >= 0) & (t > 0), t, np.inf)


def _ref_cylinder(o, d, a, b, r):
    """entry point of the ray on the side of the cylinder of radius r around the segment a..b (not its caps)"""
    length = np.linalg.norm(b - a); ax = (b - a) / length
    oa = o - a
    dp = d - (d @ ax)[..., None] * ax; op = oa - (oa @ ax) * ax         # parts perpendicular to the axis
    A = (dp * dp).sum(-1); B = dp @ op; Cc = op @ op - r * r
    disc = B * B - A * Cc
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (-B - np.sqrt(np.maximum(disc, 0.0))) / A
        y = (oa + t[..., None] * d) @ ax
        ok = (disc >= 0) & (A > 1e-30) & (t > 0) & (y > 0) & (y < length)
    return np.where(ok, t, np.inf)


def reference_render(O, rec, cam, obj, W, H, ee_frame=False):
    """-> (flat image, shaded image: float64 [H, W, 4] = depth value, r, g, b; class [H, W]; eye-space depth z [H, W], inf where nothing
    was hit).  rec: one env's state record; cam: 13 words (used as the float32 numbers the C ABI takes)."""
    rec = np.asarray(rec, dtype=np.float64); cam = np.asarray(cam, dtype=np.float32).astype(np.float64)
    q = rec[_lib.F_Q:_lib.F_Q + 6]; opos = rec[_lib.F_OPOS:_lib.F_OPOS + 3]; oquat = rec[_lib.F_OQUAT:_lib.F_OQUAT + 4]
    eye, target, up = cam[0:3], cam[3:6], cam[6:9]
    fov, aspect, near, far = cam[9:13]
    if ee_frame:
        p, qt = O.fk_ur5(q, 6); R = _quat_matrix(qt)
        eye, target, up = p + R @ eye, p + R @ target, R @ up
    f = target - eye; f /= np.linalg.norm(f)
    s = np.cross(f, up); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    T = np.tan(np.radians(fov) / 2)
    xc = (2 * (np.arange(W) + 0.5) / W - 1) * T * aspect
    yc = (1 - 2 * (np.arange(H) + 0.5) / H) * T
    d = f + xc[None, :, None] * s + yc[:, None, None] * u
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    df = d @ f
    best = np.full((H, W), np.inf); cls = np.full((H, W), BG); rgb = np.full((H, W, 3), 255.0); nrm = np.zeros((H, W, 3))

    def take(t, c, colour, normal_of):
        z = t * df
        m = np.isfinite(t) & (t > 0) & (z >= near) & (z <= far) & (t < best)
        if m.any():
            best[m] = t[m]; cls[m] = c; rgb[m] = colour
            nrm[m] = normal_of(eye + t[m][:, None] * d[m], m)

    with np.errstate(divide="ignore", invalid="ignore"):
        t = (TABLE_Z - eye[2]) / d[..., 2]
    take(np.where(np.isfinite(t), t, np.inf), TABLE, 153.0, lambda ph, m: np.array([0.0, 0.0, 1.0]))
    A, B, Rr, link_rgb = _macro("PIH_UR5_CAP_A"), _macro("PIH_UR5_CAP_B"), _macro("PIH_UR5_CAP_R"), _macro("PIH_UR5_RGB")
    for L in range(6):
        p, qt = O.fk_ur5(q, L); R = _quat_matrix(qt)
        a, b, r = p + R @ A[L], p + R @ B[L], Rr[L]
        ax = (b - a) / np.linalg.norm(b - a)
        take(_ref_cylinder(eye, d, a, b, r), ARM, 255.0 * link_rgb[L], lambda ph, m: ((ph - a) - ((ph - a) @ ax)[:, None] * ax) / r)
        for c in (a, b):
            take(_ref_sphere(eye, d, c, r), ARM, 255.0 * link_rgb[L], lambda ph, m, c=c: (ph - c) / r)
    Ro = _quat_matrix(oquat)
    nsph = int(_macro("PIH_FLY_OBJ_NSPH")[obj]); SC, SR = _macro("PIH_FLY_OBJ_SPH_C")[obj], _macro("PIH_FLY_OBJ_SPH_R")[obj]
    for i in range(nsph):
        c = opos + Ro @ SC[i]
        take(_ref_sphere(eye, d, c, SR[i]), OBJECT, 255.0 * _macro("PIH_FLY_OBJ_RGB")[obj], lambda ph, m, c=c, r=SR[i]: (ph - c) / r)
    z = best * df
    hit = np.isfinite(best)
    depth = np.ones((H, W))
    depth[hit] = far * (z[hit] - near) / (z[hit] * (far - near))
    lit = AMBIENT + DIFFUSE * np.maximum(nrm @ LIGHT, 0.0)
    lit_rgb = np.where(hit[..., None], rgb * lit[..., None], rgb)
    return np.concatenate([depth[..., None], rgb], -1), np.concatenate([depth[..., None], lit_rgb], -1), cls, np.where(hit, z, np.inf)


def classify(flat_img, obj):
    """pixel classes of a FLAT image, from its colours"""
    colours = {BG: np.full(3, 255.0), TABLE: np.full(3, 153.0), ARM: 255.0 * _macro("PIH_UR5_RGB")[0], OBJECT: 255.0 * _macro("PIH_FLY_OBJ_RGB")[obj]}
    cls = np.full(flat_img.shape[:2], -1)
    for k, c in colours.items():
        cls[np.abs(flat_img[..., 1:] - c).max(-1) < 1e-3] = k
    assert (cls >= 0).all(), "a flat image holds a colour of no class"
    return cls


def linear_depth(depth_value, cam):
    near, far = [float(x) for x in np.asarray(cam, dtype=np.float32)[11:13]]
    return near * far / (far - np.asarray(depth_value, dtype=np.float64) * (far - near))


def check_reference_scene(name, W, H, cls, obj):
    """What makes a scene worth comparing, asserted on the REFERENCE image.
    Eye-in-hand, 64 x 64: the object is 0.30 m in front of the eye, one pixel is 2 tan(30 deg) / 64 = 0.018 of the camera plane.  The Banana's
    five spheres cover 186 .. 251 pixels: at least 90.  The Amicelli's cover is two overlapping spheres of r = 21.9 mm: each a disc of
    pi (0.0219 / 0.30 / 0.018)^2 = 51 pixels, 61 .. 94 together depending on the direction its axis is seen from -- it cannot reach 90 in
    every pose; it has to show at least 40 pixels, the number the close-up asks of the object."""
    if name == "close-up" and (W, H) == (97, 61):
        assert (cls == TABLE).sum() >= 2000 and (cls == ARM).sum() >= 200 and (cls == OBJECT).sum() >= 40, [(cls == k).sum() for k in range(4)]
    if name == "eye-in-hand" and (W, H) == (64, 64):
        assert (cls == OBJECT).sum() >= (90 if obj == 0 else 40), (cls == OBJECT).sum()
    if name == "horizon":
        assert (cls == BG).mean() >= 0.25, (cls == BG).mean()


def compare(img, flat_img, ref_img, ref_cls, ref_z, cam, obj, exact_class):
    """-> (max relative error of the eye-space depth, max absolute error of the depth-buffer value, array of absolute colour errors) over
    the pixels whose class agrees; asserts the class rule: identical everywhere (exact_class) or at most CLASS_SHARE of the image different"""
    cls = classify(flat_img, obj)
    same = cls == ref_cls
    if exact_class:
        assert same.all(), "%d pixels differ in class" % (~same).sum()
    else:
        assert (~same).mean() <= CLASS_SHARE, "%.4f of the pixels differ in class" % (~same).mean()
    hit = same & (ref_cls != BG)
    assert (img[..., 0][same & (ref_cls == BG)] == 1.0).all()
    z = linear_depth(img[..., 0], cam)
    zerr = (np.abs(z - ref_z)[hit] / ref_z[hit]).max() if hit.any() else 0.0
    derr = np.abs(img[..., 0] - ref_img[..., 0])[hit].max() if hit.any() else 0.0
    return zerr, derr, np.abs(img[..., 1:] - ref_img[..., 1:])[same].reshape(-1)


# ------------------------------------------------------------------------------------------------ 1. host build against the reference
# the flags of tests/emul/Makefile
CXXFLAGS = "-O2 -fPIC -Wl,-Bsymbolic -fno-gnu-unique -fvisibility-inlines-hidden -std=c++17 -Wall -Wno-unused-variable -Wno-unused-but-set-variable -Wno-unknown-pragmas -fno-fast-math".split()


@pytest.fixture(scope="module")
def host_builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("fly_render_emul")
    libs = {}
    for prec, real in (("f64", "double"), ("f32", "float")):
        so = str(d / ("libpih_fly_render_%s.so" % prec))
        subprocess.check_call(["g++"] + CXXFLAGS + ["-DPIH_REAL=" + real, "-shared", "-o", so, os.path.join(ROOT, "tests", "emul", "pih_fly_render_emul.cpp")])
        L = C.CDLL(so)
        L.pihfr_render.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        assert L.pihfr_real_bytes() == (8 if prec == "f64" else 4)
        libs[prec] = L
    return libs


def host_render(L, rec, cam, obj, W, H, shaded, ee_frame, cull):
    rec = np.ascontiguousarray(rec, dtype=np.float64); cam = np.ascontiguousarray(cam, dtype=np.float32)
    out = np.zeros((H, W, 4))
    flags = (_lib.RENDER_SHADED if shaded else 0) | (_lib.RENDER_CAM_EE if ee_frame else 0)
    rc = L.pihfr_render(rec.ctypes.data_as(C.POINTER(C.c_double)), cam.ctypes.data_as(C.POINTER(C.c_float)), obj, W, H, flags, int(cull),
                        out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def reference_images(oracle_mod):
    """{(obj, camera, (W, H), shaded): (record, camera words, ee_frame, reference image, class, z)}: two arm poses per object and camera,
    computed once for the module"""
    out = {}
    for obj in OBJECTS:
        for ci, name in enumerate(CAMERA_NAMES):
            recs = make_states(oracle_mod, obj, 2, seed=100 + 10 * obj + ci, eye_in_hand=name == "eye-in-hand")
            for (W, H) in SIZES:
                cam, ee = cameras(W, H)[name]
                for k, rec in enumerate(recs):
                    flat, lit, cls, z = reference_render(oracle_mod, rec, cam, obj, W, H, ee)
                    check_reference_scene(name, W, H, cls, obj)
                    for shaded in (False, True):
                        out[(obj, name, (W, H), k, shaded)] = (rec, cam, ee, lit if shaded else flat, cls, z)
    return out


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_host_build_matches_the_reference(host_builds, reference_images, prec):
    """All four cameras, both objects, the three sizes, flat and shaded.  fp64: class identical on every pixel, relative depth error
    <= 1e-9, colour error <= 1e-6.  fp32: the class share rule; the maximum errors are printed -- they are the yardstick of the GPU
    tolerance (tests/test_gpu_fly_render.py), which the host build itself has to meet.  Both: the image rendered with the tile lists of
    the product's screen-bound test equals the one rendered with every primitive on for every tile, bit for bit."""
    L = host_builds[prec]
    zmax, dmax, cmax_flat, cmax_shaded = 0.0, 0.0, 0.0, 0.0
    for (obj, name, (W, H), k, shaded), (rec, cam, ee, rimg, rcls, rz) in reference_images.items():
        full = host_render(L, rec, cam, obj, W, H, shaded, ee, cull=False)
        culled = host_render(L, rec, cam, obj, W, H, shaded, ee, cull=True)
        assert np.array_equal(full, culled), (obj, name, W, H, k, shaded, int((full != culled).any(-1).sum()))
        flat = culled if not shaded else host_render(L, rec, cam, obj, W, H, False, ee, cull=True)
        assert np.array_equal(flat[..., 0], culled[..., 0])             # shading does not touch the depth buffer
        zerr, derr, cerr = compare(culled, flat, rimg, rcls, rz, cam, obj, exact_class=prec == "f64")
        zmax = max(zmax, zerr); dmax = max(dmax, derr)
        if shaded:
            cmax_shaded = max(cmax_shaded, cerr.max())
        else:
            cmax_flat = max(cmax_flat, cerr.max())
    print("%s host build: max relative depth error %.3e, max depth-buffer value error %.3e, max colour error flat %.3e shaded %.3e" % (prec, zmax, dmax, cmax_flat, cmax_shaded))
    if prec == "f64":
        assert zmax <= 1e-9 and max(cmax_flat, cmax_shaded) <= 1e-6
    else:
        from tests import test_gpu_fly_render as G
        assert zmax <= G.DEPTH_REL_TOL and dmax <= G.DEPTH_VALUE_TOL and cmax_flat <= G.COLOUR_TOL


# ------------------------------------------------------------------------------------------------ 2. constants
def test_camera_constants_match_the_header(tmp_path):
    from peg_in_hole_gym_amd.envs.peg_in_hole import RandomFly
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "pih.h"\nint main(void) {\n  static const float d[] = PIH_FLY_CAM_DEFAULT;\n'
                   '  printf("%d %d %d %d\\n", PIH_CAM_WORDS, (int)(sizeof d / sizeof d[0]), PIH_RENDER_CAM_EE, PIH_RENDER_SHADED);\n'
                   '  for (int i = 0; i < (int)(sizeof d / sizeof d[0]); i++) printf("%.9g\\n", d[i]);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    words, count, ee_flag, shaded_flag = [int(x) for x in lines[0].split()]
    assert words == count == _lib.CAM_WORDS == 13 and ee_flag == _lib.RENDER_CAM_EE and shaded_flag == _lib.RENDER_SHADED
    vals = np.array([float(x) for x in lines[1:1 + count]])
    assert len(_lib.FLY_CAM_DEFAULT) == 13 and isinstance(_lib.FLY_CAM_DEFAULT, tuple)
    assert np.array_equal(vals.astype(np.float32), np.array(_lib.FLY_CAM_DEFAULT, dtype=np.float32))
    assert tuple(RandomFly.CAMERA) == _lib.FLY_CAM_DEFAULT
    assert "pih_render_cam" in _lib.EXPORTS and len(_lib.EXPORTS) == 22


# ------------------------------------------------------------------------------------------------ 3. model table
def test_ur5_link_colours_come_from_the_urdf():
    import xml.etree.ElementTree as ET
    root = ET.parse(os.path.join(ROOT, "tests", "golden", "model_assets", "peg_in_hole_gym", "envs", "assets", "urdf", "ur5.urdf")).getroot()
    links = {l.get("name"): l for l in root.findall("link")}
    names = ["shoulder_link", "upper_arm_link", "forearm_link", "wrist_1_link", "wrist_2_link", "wrist_3_link"]      # children of the six revolute joints
    want = [[float(x) for x in links[n].find("visual").find("material").find("color").get("rgba").split()[:3]] for n in names]
    got = _macro("PIH_UR5_RGB")
    assert got.shape == (6, 3) and np.array_equal(got, np.array(want))


# ------------------------------------------------------------------------------------------------ 4. facade forwarding
class _FakeBackend:
    def __init__(self, n, offsets, **cfg):
        self.n, self.cfg, self.calls = n, cfg, []

    def reset(self, mask=None, hard_reset=False):
        pass

    def render(self, width=300, height=300, shaded=False, camera=None, ee_frame=False):
        self.calls.append(dict(width=width, height=height, shaded=shaded, camera=camera, ee_frame=ee_frame))
        return np.full((self.n, height, width, 4), 7.0, dtype=np.float32)


def test_random_fly_render_forwards_the_camera():
    from peg_in_hole_gym_amd.envs.peg_in_hole import RandomFly
    t = RandomFly(args=["Banana", 1 / 120.], backend_factory=_FakeBackend)
    img = t.render()
    assert img.shape == (300, 300, 4) and img.dtype == np.float64 and (img == 7.0).all()
    assert t._backend.calls[-1] == dict(width=300, height=300, shaded=True, camera=None, ee_frame=False)
    cam = [0.05, 0, 0, 1.05, 0, 0, 0, 1, 0, 60, 1, 0.01, 100]
    t.render("rgb_array", camera=cam, ee_frame=True)
    assert t._backend.calls[-1] == dict(width=300, height=300, shaded=True, camera=cam, ee_frame=True)
    assert t._backend.cfg["task_id"] == 1 and t._backend.cfg["object_id"] == 0
