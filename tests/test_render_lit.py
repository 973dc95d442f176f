"""Lit camera images of both tasks (pih_render_lit, peg_in_hole_gym_amd/csrc/pih_lit.h), CPU part: the product's lit per-scene and
per-pixel code, compiled on the host in fp64 and fp32 (tests/emul/pih_lit_emul.cpp, bound in tests/emul/render_emul.py), against
lit_reference of tests/render_ref.py, the numpy fp64 reference written from the model text of include/pih_render_light.h (its docstring
says what the shadow state of a pixel and a DECIDED pixel are).  The reference is anchored here to its own plain images (specular 0, shadow
factor 1: the shaded image within 1e-9; tests/test_peg_view.py anchors those to the oracle) and to closed-form answers that do not go
through a ray caster.  States, cameras, lights, cases, rules and caps are those of tests/render_cases.py, which the GPU part,
tests/test_gpu_render_lit.py, shares."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import render_cases as RC
from tests import render_ref as R
from tests.emul import render_emul
from tests.emul.render_emul import lit_render as host_render
from tests.oracle_backend import RecordingBackend
from tests.render_cases import BAD_LIGHTS, LIGHT_NAMES, LIGHTS, case_reference
from tests.render_ref import L_AMB, L_SHADOW, L_SPEC, TABLE_Z, camera_rays, fly_scene

ROOT = R.ROOT
_D = list(_lib.LIGHT_DEFAULT)


@pytest.fixture(scope="module")
def host_builds(tmp_path_factory):
    return render_emul.libs(tmp_path_factory.mktemp("lit_emul"), "lit")


@pytest.fixture(scope="module")
def cases(oracle_mod):
    return RC.make_cases(oracle_mod)


@pytest.fixture(scope="module")
def references(cases):
    """{(case key, light name): reference}, computed once for the module"""
    return {(key, ln): case_reference(case, LIGHTS[ln]) for key, case in cases.items() for ln in LIGHT_NAMES}


# ------------------------------------------------------------------------------------------------ 1. the reference
def test_reference_reproduces_the_shaded_images(cases):
    """Anchor: with specular 0 and shadow factor 1 (the light as the doubles it is) the lit reference, shadow passes and all, is the shaded
    image of plain_reference within 1e-9, for every state, camera and size; classes are identical and eye-space depths within 1e-9."""
    off = list(_lib.LIGHT_DEFAULT); off[L_SPEC] = 0.0; off[L_SHADOW] = 1.0
    for key, case in cases.items():
        W, H = case["size"]
        ref = case_reference(case, off, light_exact=True)
        _, lit, cls, z = R.plain_reference(case["scene"], case["cam"], W, H, case["frame"])
        assert np.array_equal(ref["cls"], cls) and np.array_equal(R.class_of_seg(case["task"], ref["seg"]), cls), key
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
        assert und <= RC.UNDECIDED_CAP, (key, ln, und)
        task, name, size, k = key
        if ln == "below":
            lit_side = ref["hit"] & (ref["ndl"] > 0)
            assert (ref["shadow"] == lit_side).all() and not (ref["table"] & lit_side).any()
            amb = float(np.float32(LIGHTS[ln][L_AMB])) * R.COL_TABLE
            assert not ref["table"].any() or np.abs(ref["img"][..., 1:][ref["table"]] - amb).max() <= 1e-9
        elif ln in SHADOWS.get((task[:3], name), ()):
            assert ref["shadow"].mean() >= RC.SHADOW_SHARE, (key, ln, ref["shadow"].mean())
        if task == "peg" and name == "wrist" and ln == "default":
            assert not (ref["seg"] <= 6).any()
            assert ref["table"].any() and (ref["shadow"] & ref["table"]).sum() >= 0.01 * ref["table"].sum(), (key, (ref["shadow"] & ref["table"]).sum(), ref["table"].sum())
    print("largest undecided share of an image: %.5f (cap %.3f)" % (worst, RC.UNDECIDED_CAP))


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
    rec = RC.make_fly_states(oracle_mod, 0, 1, seed=100)[0]
    shine = 8.0
    light = [0, 0, 1, 1, 1, 1, 0, 0, 1, shine, 1]
    W, H = 40, 30
    cam = _straight_down(0.3, -0.9, 1.0, TABLE_Z)
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
    rec = RC.make_fly_states(O, obj, 1, seed=100)[0].astype(np.float64)
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
    t = (TABLE_Z - eye[2]) / d[:, 2]
    xy = (eye + t[:, None] * d)[:, :2].reshape(H, W, 2)
    margin = np.full((H, W), np.inf)              # signed distance to the nearest outline: < 0 inside a footprint
    for pr in scene.prims:
        if pr.kind == "sphere":
            assert pr.p["c"][2] - pr.p["r"] > TABLE_Z
            dist = np.linalg.norm(xy - pr.p["c"][:2], axis=-1) - pr.p["r"]
        else:
            a, b = pr.p["a"], pr.p["b"]
            assert min(a[2], b[2]) - pr.p["r"] > TABLE_Z
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
    """All six peg states and the fly states of both objects, every camera of both tasks, the three sizes, the four lights.  Class rule
    of the task; shadow state equal on every decided pixel; images with and without the light-space cull bit-identical in all three
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
            err, share = RC.check_image(ref, case["task"], lambda lw: (lambda r: (r[0], r[1][..., 3]))(host_render(L, case, lw)), light, exact=prec == "f64")
            errs.append(err); worst_share = max(worst_share, share)
        errs = np.concatenate(errs); f = RC.colour_factor(light)
        print("%s host build, light %-8s: colour error max %.3e, p99 %.3e, median %.3e (bounds x %.2f); worst class share %.4f"
              % (prec, ln, errs.max(), np.percentile(errs, 99), np.median(errs), f, worst_share))
        if prec == "f64":
            assert errs.max() <= 1e-6
        else:
            assert np.percentile(errs, 99) < RC.SHADED_P99 * f and np.median(errs) < RC.SHADED_MEDIAN * f


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
    assert float(lines[0].split()[4]) == R.BIAS
    vals = np.array([float(x) for x in lines[1:12]])
    assert isinstance(_lib.LIGHT_DEFAULT, tuple) and np.array_equal(vals.astype(np.float32), np.array(_lib.LIGHT_DEFAULT, dtype=np.float32))
    assert _lib.LIGHT_DEFAULT == (-50, 30, 100, 1, 1, 1, 0.6, 0.35, 0.05, 2, 0.8)
    # the direction and the two coefficients are those of the fixed light of PIH_RENDER_SHADED
    assert _lib.LIGHT_DEFAULT[:8] == tuple(R.PLAIN_LIGHT[:8]) and R.PLAIN_LIGHT[R.L_AMB:R.L_DIF + 1] == [0.6, 0.35]
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


def test_facades_forward_the_light():
    from peg_in_hole_gym_amd.envs.peg_in_hole import PegInHole, RandomFly
    t = RandomFly(args=["Banana", 1 / 120.], backend_factory=RecordingBackend)
    t.render()
    assert t._backend.calls[-1] == dict(width=300, height=300, shaded=True, camera=None, ee_frame=False)          # today's call, no new keyword
    t.render(light="default")
    assert t._backend.calls[-1] == dict(width=300, height=300, shaded=True, camera=None, ee_frame=False, light="default")
    p = PegInHole(backend_factory=RecordingBackend)
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
