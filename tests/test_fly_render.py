"""Free camera of the 'random-fly' task (pih_render_cam, peg_in_hole_gym_amd/csrc/pih_fly_render.h), CPU part: the product's per-scene
and per-pixel code, compiled on the host in fp64 and fp32 (tests/emul/pih_fly_render_emul.cpp, bound in tests/emul/render_emul.py),
against the numpy fp64 ray caster of tests/render_ref.py; the constants of the ABI, the model table and the facade.  Scenes, cameras,
comparison rules and tolerances are those of tests/render_cases.py, which the GPU part, tests/test_gpu_fly_render.py, shares."""
import os
import subprocess

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import render_cases as RC
from tests import render_ref as R
from tests.emul import render_emul
from tests.oracle_backend import RecordingBackend

ROOT = R.ROOT


# ------------------------------------------------------------------------------------------------ 1. host build against the reference
@pytest.fixture(scope="module")
def host_builds(tmp_path_factory):
    return render_emul.libs(tmp_path_factory.mktemp("fly_render_emul"), "fly_render")


@pytest.fixture(scope="module")
def reference_images(oracle_mod):
    """RC.fly_reference_scenes at RC.SIZES: two arm poses per object and camera, computed once for the module"""
    return RC.fly_reference_scenes(oracle_mod, RC.SIZES)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_host_build_matches_the_reference(host_builds, reference_images, prec):
    """All four cameras, both objects, the three sizes, flat and shaded.  fp64: class identical on every pixel, relative depth error
    <= 1e-9, colour error <= 1e-6.  fp32: the class share rule; the maximum errors are printed -- they are the yardstick of the GPU
    tolerance (RC.FLY_*_TOL), which the host build itself has to meet.  Both: the image rendered with the tile lists of
    the product's screen-bound test equals the one rendered with every primitive on for every tile, bit for bit."""
    L = host_builds[prec]
    zmax, dmax, cmax_flat, cmax_shaded = 0.0, 0.0, 0.0, 0.0
    for obj, name, (W, H), k, rec, cam, frame, _, (rflat, rlit, rcls, rz) in reference_images:
        flat = render_emul.fly_render(L, rec, cam, obj, W, H, False, frame, cull=True)
        for shaded in (False, True):
            full = render_emul.fly_render(L, rec, cam, obj, W, H, shaded, frame, cull=False)
            culled = flat if not shaded else render_emul.fly_render(L, rec, cam, obj, W, H, True, frame, cull=True)
            assert np.array_equal(full, culled), (obj, name, W, H, k, shaded, int((full != culled).any(-1).sum()))
            assert np.array_equal(flat[..., 0], culled[..., 0])             # shading does not touch the depth buffer
            zerr, derr, cerr = RC.compare(culled, R.classify(flat, obj), rlit if shaded else rflat, rcls, rz, cam, R.BG, exact_class=prec == "f64")
            zmax = max(zmax, zerr); dmax = max(dmax, derr)
            if shaded:
                cmax_shaded = max(cmax_shaded, cerr.max())
            else:
                cmax_flat = max(cmax_flat, cerr.max())
    print("%s host build: max relative depth error %.3e, max depth-buffer value error %.3e, max colour error flat %.3e shaded %.3e" % (prec, zmax, dmax, cmax_flat, cmax_shaded))
    if prec == "f64":
        assert zmax <= 1e-9 and max(cmax_flat, cmax_shaded) <= 1e-6
    else:
        assert zmax <= RC.FLY_DEPTH_REL_TOL and dmax <= RC.FLY_DEPTH_VALUE_TOL and cmax_flat <= RC.FLY_COLOUR_TOL


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
    got = R.macro("PIH_UR5_RGB")
    assert got.shape == (6, 3) and np.array_equal(got, np.array(want))


# ------------------------------------------------------------------------------------------------ 4. facade forwarding
def test_random_fly_render_forwards_the_camera():
    from peg_in_hole_gym_amd.envs.peg_in_hole import RandomFly
    t = RandomFly(args=["Banana", 1 / 120.], backend_factory=RecordingBackend)
    img = t.render()
    assert img.shape == (300, 300, 4) and img.dtype == np.float64 and (img == 7.0).all()
    assert t._backend.calls[-1] == dict(width=300, height=300, shaded=True, camera=None, ee_frame=False)
    cam = [0.05, 0, 0, 1.05, 0, 0, 0, 1, 0, 60, 1, 0.01, 100]
    t.render("rgb_array", camera=cam, ee_frame=True)
    assert t._backend.calls[-1] == dict(width=300, height=300, shaded=True, camera=cam, ee_frame=True)
    assert t._backend.cfg["task_id"] == 1 and t._backend.cfg["object_id"] == 0
