"""Free camera of the peg-in-hole task (pih_render_view, peg_in_hole_gym_amd/csrc/pih_view.h), CPU part: the product's per-scene and
per-pixel code, compiled on the host in fp64 and fp32 (tests/emul/pih_view_emul.cpp, bound in tests/emul/render_emul.py), against the
numpy fp64 ray caster of tests/render_ref.py.  The ray caster itself is anchored to the fp64 oracle here: for the wrist preset it has to
reproduce Oracle.render.  States, cameras, comparison rules and tolerances are those of tests/render_cases.py, which the GPU part,
tests/test_gpu_peg_view.py, shares."""
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
from tests.emul.render_emul import view_render as host_render
from tests.oracle_backend import RecordingBackend
from tests.render_ref import COL_ARM, SEG_FINGER0

ROOT = R.ROOT


# ------------------------------------------------------------------------------------------------ host builds and references
@pytest.fixture(scope="module")
def host_builds(tmp_path_factory):
    return render_emul.libs(tmp_path_factory.mktemp("peg_view_emul"), "view")


@pytest.fixture(scope="module")
def states(oracle_mod):
    return RC.make_view_states(oracle_mod)


@pytest.fixture(scope="module")
def scenes(oracle_mod, states):
    return [R.peg_scene(oracle_mod, rec) for rec in states]


@pytest.fixture(scope="module")
def reference_images(states, scenes):
    """{(camera, (W, H), state index): (record, camera words, frame, flat reference, shaded reference, seg, z)}, computed once for the module.
    Every (state, camera) pair met its scene condition with the first choice of seeds: none had to be replaced."""
    out = {}
    for name in RC.PEG_CAMERA_NAMES:
        for (W, H) in RC.SIZES:
            cam, frame = RC.peg_cameras(W, H)[name]
            for k, rec in enumerate(states):
                flat, lit, seg, z = R.plain_reference(scenes[k], cam, W, H, frame)
                RC.peg_check_reference_scene(name, W, H, seg, cam)
                out[(name, (W, H), k)] = (rec, cam, frame, flat, lit, seg, z)
    return out


# ------------------------------------------------------------------------------------------------ 1. the reference against the oracle
def test_reference_reproduces_the_oracle_wrist_camera(oracle_mod, states, scenes, reference_images):
    """The wrist preset of the numpy ray caster == Oracle.render, flat and shaded, on all six states: colour class identical (which also
    says that the wrist camera never sees the arm), depth value <= 1e-9, colour <= 1e-6.  This anchors pipe, finger, tube and table
    geometry of the new reference to the fp64 oracle."""
    O = oracle_mod
    assert len(states) == 6
    for k, rec in enumerate(states):
        o = O.Oracle(1); o.set_state(rec[:O.STATE_WORDS].astype(np.float64)[None])
        for (W, H) in ((97, 61), (40, 30)):
            flat, lit, seg, _ = R.plain_reference(scenes[k], _lib.VIEW_CAM_WRIST, W, H, "ee_pos", cam_exact=True)
            assert np.array_equal(seg, reference_images[("wrist", (W, H), k)][5])
            a, b = o.render(W, H)[0], o.render(W, H, shaded=True)[0]
            assert np.array_equal(a[..., 1:], flat[..., 1:]), (k, W, H, int((a[..., 1] != flat[..., 1]).sum()))
            assert np.abs(a[..., 0] - flat[..., 0]).max() <= 1e-9 and np.abs(b[..., 0] - lit[..., 0]).max() <= 1e-9
            assert np.abs(b[..., 1:] - lit[..., 1:]).max() <= 1e-6
            assert (seg > 6).all()
    # the near-plane case is among them: in the scripted state the closed pads touch the eye and none of their t ~ 0 hits is drawn
    assert (reference_images[("wrist", (64, 64), 4)][3][..., 0] > 0.9).all()


# ------------------------------------------------------------------------------------------------ 3, 4, 5. host builds against the reference
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_host_build_matches_the_reference(host_builds, reference_images, prec):
    """All five cameras, six states, three sizes, flat and shaded.  fp64: class identical on every pixel, relative depth error and depth
    value error <= 1e-9, colour error <= 1e-6.  fp32: at most CLASS_SHARE of an image's pixels differ in class; the maximum errors are
    printed -- they are the yardstick of the GPU tolerances (RC.PEG_*_TOL), which the host build itself has to meet.  Both:
    the image rendered with the tile lists of the product's screen-bound test equals the one rendered with every primitive on for every
    tile, bit for bit, in all three formats."""
    L = host_builds[prec]
    zmax, dmax, cmax_flat, cmax_shaded, worst_share = 0.0, 0.0, 0.0, 0.0, 0.0
    shaded_err = []
    for (name, (W, H), k), (rec, cam, frame, rflat, rlit, rseg, rz) in reference_images.items():
        for shaded in (False, True):
            full = host_render(L, rec, cam, W, H, shaded, frame, cull=False)
            culled = host_render(L, rec, cam, W, H, shaded, frame, cull=True)
            for a, b in zip(full, culled):
                assert np.array_equal(a, b), (name, W, H, k, shaded, int((a != b).sum()))
            img, rgba, _ = culled
            worst_share = max(worst_share, (rgba[..., 3] != rseg).mean())
            zerr, derr, cerr = RC.compare(img, rgba[..., 3], rlit if shaded else rflat, rseg, rz, cam, _lib.SEG_NONE, exact_class=prec == "f64")
            zmax = max(zmax, zerr); dmax = max(dmax, derr)
            if shaded:
                cmax_shaded = max(cmax_shaded, cerr.max()); shaded_err.append(cerr)
            else:
                cmax_flat = max(cmax_flat, cerr.max())
    shaded_err = np.concatenate(shaded_err)
    print("%s host build: max relative depth error %.3e, max depth-buffer value error %.3e, max colour error flat %.3e shaded %.3e (p99 %.3e, median %.3e), worst class share %.4f"
          % (prec, zmax, dmax, cmax_flat, cmax_shaded, np.percentile(shaded_err, 99), np.median(shaded_err), worst_share))
    if prec == "f64":
        assert zmax <= 1e-9 and dmax <= 1e-9 and max(cmax_flat, cmax_shaded) <= 1e-6
    else:
        assert zmax <= RC.PEG_DEPTH_REL_TOL and dmax <= RC.PEG_DEPTH_VALUE_TOL and cmax_flat <= RC.PEG_COLOUR_TOL
        assert np.percentile(shaded_err, 99) < RC.SHADED_P99 and np.median(shaded_err) < RC.SHADED_MEDIAN


# ------------------------------------------------------------------------------------------------ 6. formats
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_packed_formats_of_the_host_build(host_builds, reference_images, prec):
    """rgba8 bytes == pack_byte of the float4 colours (rounded half up in the build's precision, capped at 255); the seg byte == the
    reference's class -- pipe capsule indices and which finger included -- everywhere in fp64; depth == channel 0 bit for bit."""
    L = host_builds[prec]
    real = np.float64 if prec == "f64" else np.float32
    for v, want in ((178.5, 179), (0.0, 0), (0.49, 0), (254.5, 255), (255.0, 255), (300.0, 255)):
        assert L.pihv_pack_byte(v) == want
    seen = set()
    for (name, (W, H), k), (rec, cam, frame, rflat, rlit, rseg, rz) in reference_images.items():
        if (W, H) != (97, 61):
            continue
        for shaded in (False, True):
            img, rgba, depth = host_render(L, rec, cam, W, H, shaded, frame, cull=True)
            want = np.minimum(255, (img[..., 1:].astype(real) + real(0.5)).astype(np.int64))
            assert np.array_equal(rgba[..., :3], want.astype(np.uint8)), (name, k, shaded)
            assert np.array_equal(depth, img[..., 0])
            if prec == "f64":
                assert np.array_equal(rgba[..., 3], rseg), (name, k)
            seen |= set(np.unique(rgba[..., 3]).tolist())
    pipes = {s for s in seen if _lib.VIEW_SEG_PIPE0 <= s < _lib.VIEW_SEG_PIPE0 + 24}
    assert {0, 1, 2, 3, 4, 6, SEG_FINGER0, SEG_FINGER0 + 1, _lib.VIEW_SEG_HOLE, _lib.VIEW_SEG_TABLE, _lib.SEG_NONE} <= seen and len(pipes) >= 12 and 5 not in seen, sorted(seen)


def test_degenerate_camera_gives_the_background(host_builds, states):
    """what the kernel does with a per-env camera it cannot use (cam_degenerate): the background in every format, whatever the scene"""
    L = host_builds["f32"]
    for bad, code in (([1, 1, 1, 1, 1, 1, 0, 0, 1, 60, 1, 0.01, 100], 1), ([1, 0, 1, 0, 0, 0, 0, 0, 1, float("nan"), 1, 0.01, 100], 3)):
        img, rgba, depth = host_render(L, states[0], bad, 40, 30, True, "env", cull=True, expect=code)
        assert (img[..., 0] == 1).all() and (img[..., 1:] == 255).all() and (depth == 1).all()
        assert (rgba[..., :3] == 255).all() and (rgba[..., 3] == _lib.SEG_NONE).all()


# ------------------------------------------------------------------------------------------------ 7. coincident link origins
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_links_whose_origins_coincide_render_as_spheres(oracle_mod, host_builds, states, scenes, prec):
    """Link 1's origin is link 0's (PIH_LINK_TFIX[1] = 0): its capsule is the sphere of radius 0.06 around the shoulder.  Known answer: the
    ray through the shoulder centre (the centre pixel of an odd-sized image aimed at it) hits at |eye - centre| - 0.06, on link 1 -- links 0
    and 2 end in the same sphere, and the rule of pih_view.h gives it to the sphere link."""
    org = R.scene_geometry(oracle_mod, states[0])[0]
    centre = org[1]
    assert np.array_equal(org[1], org[2]) and np.array_equal(org[5], org[6]) and np.allclose(centre, [0, 0, 0.333])
    # eyes level with the shoulder, where link 0's cylinder (below) is not in the way, and on the side link 2's cylinder leans away from or
    # square to it, where that one is not either
    lean = org[3] - org[2]; h = np.array([lean[0], lean[1], 0.0]) / np.hypot(lean[0], lean[1]); side = np.array([-h[1], h[0], 0.0])
    for eye in (centre - 1.5 * h, centre + 1.2 * side, centre - 0.8 * side - 0.8 * h):
        cam = list(eye) + list(centre) + [0, 0, 1, 20, 1, 0.01, 100]
        img, rgba, _ = host_render(host_builds[prec], states[0], cam, 5, 5, False, "env", cull=True)
        dist = np.linalg.norm(np.array(cam[:3], dtype=np.float32).astype(np.float64) - np.array(cam[3:6], dtype=np.float32).astype(np.float64))
        assert rgba[2, 2, 3] == 1 and img[2, 2, 1] == COL_ARM
        # fp32: the depth-buffer value near 1 has a quantum of 2^-24, which is z^2 / near times that in z (near = 0.01); four of them
        tol = 1e-12 * dist if prec == "f64" else 4 * dist ** 2 / 0.01 * 2.0 ** -24
        assert abs(RC.linear_depth(img[2, 2, 0], cam) - (dist - 0.06)) <= tol, (RC.linear_depth(img[2, 2, 0], cam), dist - 0.06)
        ref = R.plain_reference(scenes[0], cam, 5, 5)
        assert ref[2][2, 2] == 1 and abs(ref[3][2, 2] - (dist - 0.06)) <= 1e-12


# ------------------------------------------------------------------------------------------------ 8. header and bindings
def test_view_constants_match_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "pih.h"\nint main(void) {\n  static const float w[] = PIH_VIEW_CAM_WRIST, o[] = PIH_VIEW_CAM_OVERVIEW;\n'
                   '  printf("%d %d %d %d %d %d %d %d\\n", PIH_ABI_VERSION, PIH_RENDER_CAM_EE_POS, PIH_VIEW_SEG_HOLE, PIH_VIEW_SEG_TABLE, PIH_VIEW_SEG_PIPE0, PIH_SEG_NONE,\n'
                   '         (int)(sizeof w / sizeof w[0]), (int)(sizeof o / sizeof o[0]));\n'
                   '  for (int i = 0; i < PIH_CAM_WORDS; i++) printf("%.9g %.9g\\n", w[i], o[i]);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    abi, ee_pos, hole, table, pipe0, none, nw, no = [int(x) for x in lines[0].split()]
    assert abi == _lib.ABI_VERSION == 4 and nw == no == _lib.CAM_WORDS == 13
    assert (ee_pos, hole, table, pipe0, none) == (_lib.RENDER_CAM_EE_POS, _lib.VIEW_SEG_HOLE, _lib.VIEW_SEG_TABLE, _lib.VIEW_SEG_PIPE0, _lib.SEG_NONE) == (32, 9, 10, 32, 255)
    vals = np.array([[float(x) for x in ln.split()] for ln in lines[1:14]])
    assert isinstance(_lib.VIEW_CAM_WRIST, tuple) and isinstance(_lib.VIEW_CAM_OVERVIEW, tuple)
    assert np.array_equal(vals[:, 0].astype(np.float32), np.array(_lib.VIEW_CAM_WRIST, dtype=np.float32))
    assert np.array_equal(vals[:, 1].astype(np.float32), np.array(_lib.VIEW_CAM_OVERVIEW, dtype=np.float32))
    assert _lib.VIEW_CAM_WRIST == (0, 0, 0, 0, 0, -10, 0, 1, 0, 60, 1, 0.001, 1000)
    # the symbols of include/pih_render_view.h, which pih.h includes, are _lib.VIEW_EXPORTS
    names = sorted(set(re.findall(r"\b(pih_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "pih_render_view.h")).read())))
    assert names == sorted(_lib.VIEW_EXPORTS) == ["pih_render_view"] and not set(names) & set(_lib.EXPORTS)
    assert '#include "pih_render_view.h"' in open(os.path.join(ROOT, "include", "pih.h")).read()
    # the frame flag is a bit of its own next to the flags it combines with
    bits = [_lib.RENDER_SHADED, _lib.RENDER_CAM_EE, _lib.RENDER_OUT_RGBA8, _lib.RENDER_OUT_DEPTH, _lib.RENDER_CAM_DEVICE, _lib.RENDER_CAM_EE_POS]
    assert sorted(bits) == [1, 2, 4, 8, 16, 32]


def test_library_exports_the_view_camera():
    import __graft_entry__ as ge
    ge.build()
    L = C.CDLL(os.path.join(ROOT, "peg_in_hole_gym_amd", "csrc", "libpih_hip.so"))
    assert hasattr(L, "pih_render_view")


def test_peg_in_hole_render_view_delegates_to_the_backend():
    from peg_in_hole_gym_amd.envs.peg_in_hole import PegInHole
    t = PegInHole(backend_factory=RecordingBackend)
    assert t.render_view(camera=list(_lib.VIEW_CAM_OVERVIEW), fmt="rgba8", width=64, height=48) == "image"
    assert t._backend.calls == [dict(camera=list(_lib.VIEW_CAM_OVERVIEW), fmt="rgba8", width=64, height=48)] and t._backend.cfg["task_id"] == 0
