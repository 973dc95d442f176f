"""Output formats and per-env cameras of the random-fly camera (pih_render_cam: PIH_RENDER_OUT_RGBA8, PIH_RENDER_OUT_DEPTH,
PIH_RENDER_CAM_DEVICE), CPU part: the product's per-pixel, pack, seg and camera-test code compiled on the host in fp64 and fp32
(tests/emul/pih_fly_image_emul.cpp) against the numpy fp64 ray caster of tests/test_fly_render.py (`T`: same scenes, cameras, sizes),
the constants of the ABI, and tracking_cameras.  The GPU part is tests/test_gpu_fly_image.py; it takes the comparison rules and the
(state, camera) pairs of its per-env-camera tests from this module, where the fp32 host build has to meet the same caps first.

Comparison rules (no tolerance of its own: the caps are T.CLASS_SHARE and the DEPTH_* / COLOUR_TOL numbers of tests/test_gpu_fly_render.py):
  class   seg 0..5 -> ARM, 6 -> OBJECT, 7 -> TABLE, 255 -> BG; against the reference's class: identical on every pixel in fp64, at most
          CLASS_SHARE of an image different in fp32 and on the GPU
  link    a pixel with seg = L < 6 and agreeing class: the reference's hit point eye + z_ref d / (d . f) lies on link L's capsule,
          |dist(point, segment L) - r_L| <= 1e-6 m; in fp32 / on the GPU the pixels where it does not count towards the same share
          (capsules overlap at the joints)
  depth   on class-agreeing pixels the depth-buffer value and the eye-space depth recovered from it; background exactly 1
  colour  on class-agreeing pixels excess = max(0, |byte - reference colour| - 0.5): what exceeds the unavoidable half step"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import test_fly_render as T
from tests import test_gpu_fly_render as G

SIZES = T.SIZES + ((5, 3),)                      # + narrower than a 16-byte vector, H W odd
LINK_TOL = 1e-6                                 # [m]


# ------------------------------------------------------------------------------------------------ comparison rules (shared with the GPU part)
def seg_classes(seg):
    cls = np.full(seg.shape, -1)
    cls[seg < 6] = T.ARM; cls[seg == _lib.SEG_OBJECT] = T.OBJECT; cls[seg == _lib.SEG_TABLE] = T.TABLE; cls[seg == _lib.SEG_NONE] = T.BG
    assert (cls >= 0).all(), "seg values outside 0..7, 255: %s" % np.unique(seg[cls < 0])
    return cls


def _camera_rays(O, rec, cam, W, H, ee_frame):
    """eye, unit ray directions [H, W, 3] and d . f of the reference's camera (the expressions of T.reference_render)"""
    rec = np.asarray(rec, dtype=np.float64); cam = np.asarray(cam, dtype=np.float32).astype(np.float64)
    eye, target, up = cam[0:3], cam[3:6], cam[6:9]
    if ee_frame:
        p, qt = O.fk_ur5(rec[_lib.F_Q:_lib.F_Q + 6], 6); R = T._quat_matrix(qt)
        eye, target, up = p + R @ eye, p + R @ target, R @ up
    f = target - eye; f /= np.linalg.norm(f)
    s = np.cross(f, up); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    tan = np.tan(np.radians(cam[9]) / 2)
    xc = (2 * (np.arange(W) + 0.5) / W - 1) * tan * cam[10]
    yc = (1 - 2 * (np.arange(H) + 0.5) / H) * tan
    d = f + xc[None, :, None] * s + yc[:, None, None] * u
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return eye, d, d @ f


def link_failures(O, seg, same, rec, cam, ee_frame, ref_z):
    """number of class-agreeing ARM pixels whose reference hit point does not lie on the capsule of the link the seg byte names"""
    H, W = seg.shape
    rec = np.asarray(rec, dtype=np.float64)
    eye, d, df = _camera_rays(O, rec, cam, W, H, ee_frame)
    A, B, Rr = T._macro("PIH_UR5_CAP_A"), T._macro("PIH_UR5_CAP_B"), T._macro("PIH_UR5_CAP_R")
    bad = 0
    for L in range(6):
        m = same & (seg == L)
        if not m.any():
            continue
        p, qt = O.fk_ur5(rec[_lib.F_Q:_lib.F_Q + 6], L); R = T._quat_matrix(qt)
        a, b = p + R @ A[L], p + R @ B[L]
        ph = eye + (ref_z[m] / df[m])[:, None] * d[m]
        q = np.clip(((ph - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
        dist = np.linalg.norm(ph - (a + q[:, None] * (b - a)), axis=-1)
        bad += int((np.abs(dist - Rr[L]) > LINK_TOL).sum())
    return bad


def check_seg(O, seg, rec, cam, ee_frame, ref, exact):
    """asserts the class and link rules on one image; -> mask of the class-agreeing pixels"""
    rflat, rlit, rcls, rz = ref
    same = seg_classes(seg) == rcls
    nlink = link_failures(O, seg, same, rec, cam, ee_frame, rz)
    if exact:
        assert same.all() and nlink == 0, "%d pixels differ in class, %d name the wrong link" % ((~same).sum(), nlink)
    else:
        share = ((~same).sum() + nlink) / same.size
        assert share <= T.CLASS_SHARE, "%.4f of the pixels differ in class or link (%d class, %d link)" % (share, (~same).sum(), nlink)
    return same


def depth_errors(depth, same, ref, cam):
    """-> (max relative error of the eye-space depth, max absolute error of the depth-buffer value) over the class-agreeing hit pixels;
    asserts that the class-agreeing background is exactly 1"""
    rflat, rlit, rcls, rz = ref
    depth = np.asarray(depth, dtype=np.float64)
    assert np.isfinite(depth).all()
    assert (depth[same & (rcls == T.BG)] == 1.0).all()
    hit = same & (rcls != T.BG)
    if not hit.any():
        return 0.0, 0.0
    z = T.linear_depth(depth, cam)
    return (np.abs(z - rz)[hit] / rz[hit]).max(), np.abs(depth - rflat[..., 0])[hit].max()


def colour_excess(rgb, same, ref_img):
    """what |byte - reference colour| exceeds the half step by, over the class-agreeing pixels (flat array)"""
    return np.maximum(0.0, np.abs(rgb.astype(np.float64) - ref_img[..., 1:]) - 0.5)[same].reshape(-1)


class Figures:
    """running maxima / samples over many images; limits() asserts the fp32 / GPU caps of tests/test_gpu_fly_render.py"""
    def __init__(self):
        self.z = self.d = self.flat = 0.0; self.shaded = []

    def add_depth(self, zd):
        self.z = max(self.z, zd[0]); self.d = max(self.d, zd[1])

    def add_colour(self, excess, shaded):
        if shaded:
            self.shaded.append(excess)
        elif excess.size:
            self.flat = max(self.flat, excess.max())

    def text(self):
        sh = np.concatenate(self.shaded) if self.shaded else np.zeros(1)
        return ("max relative depth error %.3e (bound %.3e), depth-buffer value %.3e (%.3e), flat colour excess %.3e (%.3e), shaded colour excess p99 %.3e median %.3e max %.3e"
                % (self.z, G.DEPTH_REL_TOL, self.d, G.DEPTH_VALUE_TOL, self.flat, G.COLOUR_TOL, np.percentile(sh, 99), np.median(sh), sh.max()))

    def limits(self):
        assert self.z <= G.DEPTH_REL_TOL and self.d <= G.DEPTH_VALUE_TOL and self.flat <= G.COLOUR_TOL
        if self.shaded:
            sh = np.concatenate(self.shaded)
            assert np.percentile(sh, 99) < 0.05 and np.median(sh) < 1e-3


# ------------------------------------------------------------------------------------------------ the per-env-camera cases of the GPU part
def per_env_cases(O):
    """name -> dict(obj, states float32 [n, 48], cams float32 [n, 13], ee, size (W, H), checked envs, degenerate rows).  The GPU tests of
    PIH_RENDER_CAM_DEVICE render exactly these; test_per_env_cases_meet_the_caps_on_the_host puts every checked env through the fp32
    host build first."""
    W, H = 97, 61
    three = [np.array(T.cameras(W, H)[k][0], dtype=np.float32) for k in ("overview", "close-up", "horizon")]
    cases = {"cycle": dict(obj=0, states=T.make_states(O, 0, 70, seed=300), cams=np.stack([three[e % 3] for e in range(70)]), ee=False, size=(W, H),
                           checked=(0, 3, 4, 5, 6, 7, 63, 64, 69), degenerate=())}
    hand = np.tile(np.array(T.cameras(64, 64)["eye-in-hand"][0], dtype=np.float32), (6, 1))
    hand[:, 9] = np.linspace(50.0, 70.0, 6)
    cases["eye-in-hand"] = dict(obj=0, states=T.make_states(O, 0, 6, seed=G.SCENE_SEED[(0, "eye-in-hand")], eye_in_hand=True), cams=hand, ee=True,
                                size=(64, 64), checked=tuple(range(6)), degenerate=())
    deg = np.stack([three[e % 3] for e in range(6)])
    deg[2, 0:3] = deg[2, 3:6]                   # eye == target
    deg[4, 9] = np.nan                          # fov = NaN
    cases["degenerate"] = dict(obj=1, states=T.make_states(O, 1, 6, seed=G.SCENE_SEED[(1, "close-up")]), cams=deg, ee=False, size=(40, 30),
                               checked=(0, 1, 3, 5), degenerate=(2, 4))
    return cases


# ------------------------------------------------------------------------------------------------ host build
@pytest.fixture(scope="module")
def image_builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("fly_image_emul")
    libs = {}
    for prec, real in (("f64", "double"), ("f32", "float")):
        so = str(d / ("libpih_fly_image_%s.so" % prec))
        subprocess.check_call(["g++"] + T.CXXFLAGS + ["-DPIH_REAL=" + real, "-shared", "-o", so, os.path.join(T.ROOT, "tests", "emul", "pih_fly_image_emul.cpp")])
        L = C.CDLL(so)
        L.pihfi_render.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.pihfi_pack_byte.argtypes = [C.c_double]
        L.pihfi_cam_degenerate.argtypes = [C.POINTER(C.c_float)]
        assert L.pihfi_real_bytes() == (8 if prec == "f64" else 4)
        libs[prec] = L
    return libs


def host_image(L, rec, cam, obj, W, H, shaded, ee_frame, cull):
    """-> (uint8 [H, W, 4] = r, g, b, seg; float64 [H, W] depth; code of the camera test)"""
    rec = np.ascontiguousarray(rec, dtype=np.float64); cam = np.ascontiguousarray(cam, dtype=np.float32)
    rgba = np.full((H, W, 4), 0xA5, dtype=np.uint8); depth = np.full((H, W), np.nan)
    flags = (_lib.RENDER_SHADED if shaded else 0) | (_lib.RENDER_CAM_EE if ee_frame else 0)
    rc = L.pihfi_render(rec.ctypes.data_as(C.POINTER(C.c_double)), cam.ctypes.data_as(C.POINTER(C.c_float)), obj, W, H, flags, int(cull),
                        rgba.ctypes.data, depth.ctypes.data)
    assert rc >= 0
    return rgba, depth, rc


def cam_code(L, cam):
    cam = np.ascontiguousarray(cam, dtype=np.float32)
    return L.pihfi_cam_degenerate(cam.ctypes.data_as(C.POINTER(C.c_float)))


@pytest.fixture(scope="module")
def reference_scenes(oracle_mod):
    """[(obj, camera name, (W, H), record, camera words, ee_frame, reference)]: T's scenes (two arm poses per object and camera) at SIZES"""
    out = []
    for obj in T.OBJECTS:
        for ci, name in enumerate(T.CAMERA_NAMES):
            recs = T.make_states(oracle_mod, obj, 2, seed=100 + 10 * obj + ci, eye_in_hand=name == "eye-in-hand")
            for (W, H) in SIZES:
                cam, ee = T.cameras(W, H)[name]
                for rec in recs:
                    ref = T.reference_render(oracle_mod, rec, cam, obj, W, H, ee)
                    T.check_reference_scene(name, W, H, ref[2], obj)
                    out.append((obj, name, (W, H), rec, cam, ee, ref))
    return out


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_host_build_of_the_packed_formats(image_builds, reference_scenes, oracle_mod, prec):
    """rgba8 flat and shaded, and depth, on all of T's scenes at T.SIZES plus (5, 3).  fp64: class and link exact, relative depth error
    <= 1e-9, colour excess <= 1e-6 (the bars of T's fp64 build).  fp32: the share rule and the caps of the GPU tests.  Both: with the
    tile lists and without, bit-identical; the depth plane does not depend on shading."""
    L = image_builds[prec]
    fig = Figures()
    for obj, name, (W, H), rec, cam, ee, ref in reference_scenes:
        flat, depth, code = host_image(L, rec, cam, obj, W, H, False, ee, cull=True)
        lit, depth2, _ = host_image(L, rec, cam, obj, W, H, True, ee, cull=True)
        assert code == 0 and np.array_equal(depth, depth2) and np.array_equal(flat[..., 3], lit[..., 3])
        for shaded, img in ((False, flat), (True, lit)):
            full, fdepth, _ = host_image(L, rec, cam, obj, W, H, shaded, ee, cull=False)
            assert np.array_equal(full, img) and np.array_equal(fdepth, depth), (obj, name, W, H, shaded)
        same = check_seg(oracle_mod, flat[..., 3], rec, cam, ee, ref, exact=prec == "f64")
        fig.add_depth(depth_errors(depth, same, ref, cam))
        fig.add_colour(colour_excess(flat[..., :3], same, ref[0]), False)
        fig.add_colour(colour_excess(lit[..., :3], same, ref[1]), True)
    print("%s host build: %s" % (prec, fig.text()))
    if prec == "f64":
        assert fig.z <= 1e-9 and fig.flat <= 1e-6 and np.concatenate(fig.shaded).max() <= 1e-6
    else:
        fig.limits()


def test_pack_and_seg_known_answers(image_builds):
    """the rounding rule min(255, (int)(v + 0.5f)): 255 x 0.7f is 178.5 exactly in fp32 and becomes 179"""
    assert np.float32(255) * np.float32(0.7) == np.float32(178.5)
    for L in image_builds.values():
        assert [L.pihfi_pack_byte(v) for v in (178.5, 0.49, 254.5, 300.0, 0.0, 0.5, 255.0)] == [179, 0, 255, 255, 0, 1, 255]
        assert L.pihfi_seg_of_kind(L.pihfi_kind(2)) == 255 == _lib.SEG_NONE
        assert L.pihfi_seg_of_kind(L.pihfi_kind(1)) == 7 == _lib.SEG_TABLE
        assert L.pihfi_seg_of_kind(L.pihfi_kind(0)) == 6 == _lib.SEG_OBJECT
        assert [L.pihfi_seg_of_kind(k) for k in range(6)] == list(range(6))


# the degenerate cameras of tests/test_gpu_fly_render.py::test_errors_and_untouched_paths and the field its message has to name
# (codes of fly::cam_degenerate: 1 eye / target, 2 up, 3 fov, 4 aspect, 5 near, 6 far)
DEGENERATE = ((dict(eye=list(_lib.FLY_CAM_DEFAULT[3:6])), 1), (dict(up=[1.6, 0.0, 1.0]), 2), (dict(up=[0.0, 0.0, 0.0]), 2), (dict(fov=0.0), 3), (dict(fov=180.0), 3),
              (dict(aspect=0.0), 4), (dict(aspect=-1.0), 4), (dict(near=0.0), 5), (dict(far=0.01), 6), (dict(far=0.005), 6))


def camera_with(**kw):
    c = list(_lib.FLY_CAM_DEFAULT)
    for k, v in kw.items():
        i = {"eye": 0, "target": 3, "up": 6, "fov": 9, "aspect": 10, "near": 11, "far": 12}[k]
        c[i:i + (3 if i < 9 else 1)] = v if i < 9 else [v]
    return c


def test_camera_test_names_the_field(image_builds):
    for L in image_builds.values():
        for kw, code in DEGENERATE:
            assert cam_code(L, camera_with(**kw)) == code, kw
        assert cam_code(L, _lib.FLY_CAM_DEFAULT) == 0
        for W, H in SIZES:
            for name in T.CAMERA_NAMES:
                assert cam_code(L, T.cameras(W, H)[name][0]) == 0
        for i in range(_lib.CAM_WORDS):
            for v in (np.nan, np.inf, -np.inf):
                c = list(_lib.FLY_CAM_DEFAULT); c[i] = v
                assert cam_code(L, c) != 0, (i, v)


def test_degenerate_camera_gives_the_background(image_builds, oracle_mod):
    rec = T.make_states(oracle_mod, 0, 1, seed=100)[0]
    for L in image_builds.values():
        for cam in (camera_with(eye=list(_lib.FLY_CAM_DEFAULT[3:6])), camera_with(fov=np.nan)):
            for shaded in (False, True):
                rgba, depth, code = host_image(L, rec, cam, 0, 40, 30, shaded, False, cull=True)
                assert code != 0 and (depth == 1.0).all() and (rgba == 255).all()


def test_format_constants_match_the_header(tmp_path):
    names = ("RENDER_OUT_RGBA8", "RENDER_OUT_DEPTH", "RENDER_CAM_DEVICE", "SEG_OBJECT", "SEG_TABLE", "SEG_NONE")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "pih.h"\n#include "pih_model.h"\nint main(void) {\n  printf("%s %%d %%d\\n", %s, PIH_UR5_NJ, PIH_ABI_VERSION);\n  return 0;\n}\n'
                   % (" ".join(["%d"] * len(names)), ", ".join("PIH_" + n for n in names)))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(T.ROOT, "include"), "-o", str(exe), str(src)])
    vals = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert vals[:6] == [getattr(_lib, n) for n in names] == [4, 8, 16, 6, 7, 255]
    assert vals[6] == _lib.SEG_OBJECT and vals[7] == _lib.ABI_VERSION == 4
    flags = (_lib.RENDER_SHADED, _lib.RENDER_CAM_EE, _lib.RENDER_OUT_RGBA8, _lib.RENDER_OUT_DEPTH, _lib.RENDER_CAM_DEVICE)
    assert sum(flags) == 31 and all(f & (f - 1) == 0 for f in flags)                      # five distinct bits


def test_tracking_cameras_on_cpu_tensors():
    import torch
    from peg_in_hole_gym_amd.vec_env import tracking_cameras
    opos = torch.tensor([[0.45, 0.1, 0.55], [0.3, -0.2, 0.4], [0.0, 0.0, 0.1]])
    cam = tracking_cameras(opos, eye=(1.2, 0.6, 0.9))
    assert cam.shape == (3, _lib.CAM_WORDS) and cam.dtype == torch.float32 and cam.device == opos.device
    assert torch.equal(cam[:, 3:6], opos)
    want = torch.tensor([1.2, 0.6, 0.9, 0, 0, 0, 0, 0, 1, 60, 1, 0.01, 100])
    for i in list(range(3)) + list(range(6, 13)):
        assert (cam[:, i] == want[i]).all(), i
    cam = tracking_cameras(opos.double(), eye=opos + 1.0, up=(0, 1, 0), fov=45, aspect=1.5, near=0.1, far=10)
    assert cam.dtype == torch.float32 and torch.equal(cam[:, 0:3], opos + 1.0) and torch.equal(cam[:, 3:6], opos)
    assert torch.equal(cam[0, 6:], torch.tensor([0, 1, 0, 45, 1.5, 0.1, 10]))
    with pytest.raises(ValueError):
        tracking_cameras(torch.zeros(3, 4), eye=(1, 1, 1))


def test_per_env_cases_meet_the_caps_on_the_host(image_builds, oracle_mod):
    """every (state, camera) pair the GPU tests of PIH_RENDER_CAM_DEVICE check goes through the fp32 host build under the same caps"""
    L = image_builds["f32"]
    for name, case in per_env_cases(oracle_mod).items():
        fig = Figures()
        (W, H), obj, ee = case["size"], case["obj"], case["ee"]
        for e in case["checked"]:
            rec, cam = case["states"][e], case["cams"][e]
            assert cam_code(L, cam) == 0
            ref = T.reference_render(oracle_mod, rec, cam, obj, W, H, ee)
            flat, depth, _ = host_image(L, rec, cam, obj, W, H, False, ee, cull=True)
            same = check_seg(oracle_mod, flat[..., 3], rec, cam, ee, ref, exact=False)
            fig.add_depth(depth_errors(depth, same, ref, cam))
            fig.add_colour(colour_excess(flat[..., :3], same, ref[0]), False)
        for e in case["degenerate"]:
            assert cam_code(L, case["cams"][e]) != 0
        print("%s: %s" % (name, fig.text()))
        fig.limits()
