"""Output formats and per-env cameras of the random-fly camera (pih_render_cam: PIH_RENDER_OUT_RGBA8, PIH_RENDER_OUT_DEPTH,
PIH_RENDER_CAM_DEVICE), CPU part: the product's per-pixel, pack, seg and camera-test code compiled on the host in fp64 and fp32
(tests/emul/pih_fly_image_emul.cpp, bound in tests/emul/render_emul.py) against the numpy fp64 ray caster of tests/render_ref.py, the
constants of the ABI, and tracking_cameras.  Scenes, cameras, comparison rules (class, link, depth, colour excess), caps and the
(state, camera) pairs of the per-env-camera tests are those of tests/render_cases.py; the GPU part, tests/test_gpu_fly_image.py, shares
them, and the fp32 host build has to meet the same caps here first."""
import os
import subprocess

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import render_cases as RC
from tests import render_ref as R
from tests.emul import render_emul
from tests.emul.render_emul import cam_code, fly_image as host_image
from tests.render_cases import DEGENERATE, Figures, camera_with, check_seg, colour_excess, depth_errors

SIZES = RC.IMAGE_SIZES


# ------------------------------------------------------------------------------------------------ host build
@pytest.fixture(scope="module")
def image_builds(tmp_path_factory):
    return render_emul.libs(tmp_path_factory.mktemp("fly_image_emul"), "fly_image")


@pytest.fixture(scope="module")
def reference_scenes(oracle_mod):
    """RC.fly_reference_scenes (two arm poses per object and camera) at SIZES"""
    return RC.fly_reference_scenes(oracle_mod, SIZES)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_host_build_of_the_packed_formats(image_builds, reference_scenes, oracle_mod, prec):
    """rgba8 flat and shaded, and depth, on all of RC.fly_reference_scenes at RC.SIZES plus (5, 3).  fp64: class and link exact, relative depth error
    <= 1e-9, colour excess <= 1e-6 (the bars of the fp64 build of tests/test_fly_render.py).  fp32: the share rule and the caps of the GPU tests.  Both: with the
    tile lists and without, bit-identical; the depth plane does not depend on shading."""
    L = image_builds[prec]
    fig = Figures()
    for obj, name, (W, H), _, rec, cam, frame, scene, ref in reference_scenes:
        flat, depth, code = host_image(L, rec, cam, obj, W, H, False, frame, cull=True)
        lit, depth2, _ = host_image(L, rec, cam, obj, W, H, True, frame, cull=True)
        assert code == 0 and np.array_equal(depth, depth2) and np.array_equal(flat[..., 3], lit[..., 3])
        for shaded, img in ((False, flat), (True, lit)):
            full, fdepth, _ = host_image(L, rec, cam, obj, W, H, shaded, frame, cull=False)
            assert np.array_equal(full, img) and np.array_equal(fdepth, depth), (obj, name, W, H, shaded)
        same = check_seg(scene, flat[..., 3], cam, frame, ref, exact=prec == "f64")
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


def test_camera_test_names_the_field(image_builds):
    for L in image_builds.values():
        for kw, code in DEGENERATE:
            assert cam_code(L, camera_with(**kw)) == code, kw
        assert cam_code(L, _lib.FLY_CAM_DEFAULT) == 0
        for W, H in SIZES:
            for name in RC.FLY_CAMERA_NAMES:
                assert cam_code(L, RC.fly_cameras(W, H)[name][0]) == 0
        for i in range(_lib.CAM_WORDS):
            for v in (np.nan, np.inf, -np.inf):
                c = list(_lib.FLY_CAM_DEFAULT); c[i] = v
                assert cam_code(L, c) != 0, (i, v)


def test_degenerate_camera_gives_the_background(image_builds, oracle_mod):
    rec = RC.make_fly_states(oracle_mod, 0, 1, seed=100)[0]
    for L in image_builds.values():
        for cam in (camera_with(eye=list(_lib.FLY_CAM_DEFAULT[3:6])), camera_with(fov=np.nan)):
            for shaded in (False, True):
                rgba, depth, code = host_image(L, rec, cam, 0, 40, 30, shaded, "env", cull=True)
                assert code != 0 and (depth == 1.0).all() and (rgba == 255).all()


def test_format_constants_match_the_header(tmp_path):
    names = ("RENDER_OUT_RGBA8", "RENDER_OUT_DEPTH", "RENDER_CAM_DEVICE", "SEG_OBJECT", "SEG_TABLE", "SEG_NONE")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "pih.h"\n#include "pih_model.h"\nint main(void) {\n  printf("%s %%d %%d\\n", %s, PIH_UR5_NJ, PIH_ABI_VERSION);\n  return 0;\n}\n'
                   % (" ".join(["%d"] * len(names)), ", ".join("PIH_" + n for n in names)))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(R.ROOT, "include"), "-o", str(exe), str(src)])
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
    for name, case in RC.per_env_cases(oracle_mod).items():
        fig = Figures()
        (W, H), obj, frame = case["size"], case["obj"], case["frame"]
        for e in case["checked"]:
            rec, cam = case["states"][e], case["cams"][e]
            assert cam_code(L, cam) == 0
            scene = R.fly_scene(oracle_mod, rec, obj)
            ref = R.plain_reference(scene, cam, W, H, frame)
            flat, depth, _ = host_image(L, rec, cam, obj, W, H, False, frame, cull=True)
            same = check_seg(scene, flat[..., 3], cam, frame, ref, exact=False)
            fig.add_depth(depth_errors(depth, same, ref, cam))
            fig.add_colour(colour_excess(flat[..., :3], same, ref[0]), False)
        for e in case["degenerate"]:
            assert cam_code(L, case["cams"][e]) != 0
        print("%s: %s" % (name, fig.text()))
        fig.limits()
