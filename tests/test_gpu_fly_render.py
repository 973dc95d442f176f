"""Free camera of the 'random-fly' task on the GPU: pih_render_cam / PihVecEnv.render / RandomFly.render / BaseEnv.render against the
numpy fp64 ray caster of tests/render_ref.py, with the scenes, cameras, sizes, comparison rules and tolerances (RC.FLY_*_TOL, derived
there from the fp32 host build) of tests/render_cases.py, which tests/test_fly_render.py shares."""
import ctypes as C

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import render_cases as RC
from tests import render_ref as R
from tests.render_cases import FLY_COLOUR_TOL as COLOUR_TOL, FLY_DEPTH_REL_TOL as DEPTH_REL_TOL, FLY_DEPTH_VALUE_TOL as DEPTH_VALUE_TOL


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


def _check(O, img, flat, rec, cam, frame, obj, shaded, name=None):
    """one env's image against the reference under the class share, depth and colour rules; prints the figures before it asserts"""
    H, W = img.shape[:2]
    rflat, rlit, rcls, rz = R.plain_reference(R.fly_scene(O, rec, obj), cam, W, H, frame)
    if name is not None:
        RC.fly_check_reference_scene(name, W, H, rcls, obj)
    return RC.compare(img.astype(np.float64), R.classify(flat.astype(np.float64), obj), rlit if shaded else rflat, rcls, rz, cam, R.BG, exact_class=False)


@pytest.mark.gpu
@pytest.mark.parametrize("obj", [0, 1])
def test_parity_all_cameras_sizes_flat_and_shaded(torch_mod, oracle_mod, obj):
    """N = 6: the four cameras, the three sizes, flat and shaded, every env against the reference fed with the handle's own state()"""
    n = 6
    g = RC.fly_handle(n, object_id=obj)
    zmax = dmax = cmax = 0.0; shaded_err = []
    for name in RC.FLY_CAMERA_NAMES:
        g.set_state(torch_mod.tensor(RC.make_fly_states(oracle_mod, obj, n, seed=RC.SCENE_SEED[(obj, name)], eye_in_hand=name == "eye-in-hand")))
        st = g.state().cpu().numpy()
        for (W, H) in RC.SIZES:
            cam, frame = RC.fly_cameras(W, H)[name]
            flat = g.render(W, H, camera=cam, ee_frame=frame == "ee").cpu().numpy()
            lit = g.render(W, H, camera=cam, ee_frame=frame == "ee", shaded=True).cpu().numpy()
            assert flat.shape == (n, H, W, 4) and np.array_equal(flat[..., 0], lit[..., 0])          # shading does not touch the depth buffer
            for e in range(n):
                z, d, c = _check(oracle_mod, flat[e], flat[e], st[e], cam, frame, obj, False, name)
                zmax = max(zmax, z); dmax = max(dmax, d); cmax = max(cmax, c.max())
                z, d, c = _check(oracle_mod, lit[e], flat[e], st[e], cam, frame, obj, True)
                shaded_err.append(c)
    shaded_err = np.concatenate(shaded_err)
    print("object %d: max relative depth error %.3e (bound %.3e), depth-buffer value %.3e (%.3e), flat colour %.3e (%.3e), shaded colour p99 %.3e median %.3e max %.3e"
          % (obj, zmax, DEPTH_REL_TOL, dmax, DEPTH_VALUE_TOL, cmax, COLOUR_TOL, np.percentile(shaded_err, 99), np.median(shaded_err), shaded_err.max()))
    assert zmax <= DEPTH_REL_TOL and dmax <= DEPTH_VALUE_TOL and cmax <= COLOUR_TOL
    assert np.percentile(shaded_err, 99) < 0.05 and np.median(shaded_err) < 1e-3


@pytest.mark.gpu
def test_soa_indexing_and_sub_ranges(torch_mod, oracle_mod):
    """N = 70 (not a multiple of the wave): word w of env e is state[w * n + e]; a sub-range renders the same pixels"""
    n, obj, (W, H) = 70, 0, (97, 61)
    g = RC.fly_handle(n, object_id=obj)
    g.set_state(torch_mod.tensor(RC.make_fly_states(oracle_mod, obj, n, seed=300)))
    st = g.state().cpu().numpy()
    cam, frame = RC.fly_cameras(W, H)["close-up"]
    full = g.render(W, H, camera=cam).cpu().numpy()
    part = g.render(W, H, env_begin=3, env_count=5, camera=cam).cpu().numpy()
    assert part.shape == (5, H, W, 4) and np.array_equal(part, full[3:8])
    for e in (0, 63, 64, 69):
        z, d, c = _check(oracle_mod, full[e], full[e], st[e], cam, frame, obj, False, "close-up")
        print("env %d: max relative depth error %.3e, depth-buffer value %.3e, colour %.3e" % (e, z, d, c.max()))
        assert z <= DEPTH_REL_TOL and d <= DEPTH_VALUE_TOL and c.max() <= COLOUR_TOL


@pytest.mark.gpu
def test_live_state_and_default_camera(torch_mod, oracle_mod):
    """after reset and 40 steps the image is the reference's for state() of the same handle; camera=None is PIH_FLY_CAM_DEFAULT"""
    n, obj, (W, H) = 6, 0, (97, 61)
    g = RC.fly_handle(n, object_id=obj, auto_reset=0)
    g.reset(seed=11)
    rng = np.random.default_rng(11)
    for _ in range(40):
        g.step(torch_mod.tensor(rng.uniform(-1, 1, (n, 6)), dtype=torch_mod.float32))
    st = g.state().cpu().numpy()
    img = g.render(W, H).cpu().numpy()
    assert np.array_equal(img, g.render(W, H, camera=_lib.FLY_CAM_DEFAULT).cpu().numpy())
    assert np.abs(st[:, _lib.F_Q:_lib.F_Q + 6] - RC.REST).max() > 1e-3                     # the arms have moved
    for e in range(n):
        z, d, c = _check(oracle_mod, img[e], img[e], st[e], _lib.FLY_CAM_DEFAULT, "env", obj, False)
        print("env %d: max relative depth error %.3e, depth-buffer value %.3e, colour %.3e" % (e, z, d, c.max()))
        assert z <= DEPTH_REL_TOL and d <= DEPTH_VALUE_TOL and c.max() <= COLOUR_TOL


@pytest.mark.gpu
def test_errors_and_untouched_paths(torch_mod):
    from oracle import oracle as O
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    torch = torch_mod
    L = _lib.load()
    peg = PihVecEnv(3, seed=7)
    with pytest.raises(ValueError):
        peg.render(64, 48, camera=_lib.FLY_CAM_DEFAULT)
    with pytest.raises(ValueError):
        peg.render(64, 48, ee_frame=True)
    out = torch.empty(3, 48, 64, 4, device="cuda")
    assert L.pih_render_cam(peg.h, out.data_ptr(), None, 64, 48, 0, 3, 0, None) == -2
    assert b"random-fly" in L.pih_last_error(peg.h)
    fly = RC.fly_handle(3)
    assert L.pih_render_ex(fly.h, out.data_ptr(), 64, 48, 0, 3, 0, None) == -2
    assert b"peg-in-hole" in L.pih_last_error(fly.h)
    assert L.pih_render(fly.h, out.data_ptr(), 64, 48, 0, 3, None) == -2
    good = list(_lib.FLY_CAM_DEFAULT)
    def cam_with(**kw):
        c = list(good)
        for k, v in kw.items():
            i = {"eye": 0, "target": 3, "up": 6, "fov": 9, "aspect": 10, "near": 11, "far": 12}[k]
            c[i:i + (3 if i < 9 else 1)] = v if i < 9 else [v]
        return (C.c_float * _lib.CAM_WORDS)(*c)
    assert L.pih_render_cam(fly.h, out.data_ptr(), cam_with(), 64, 48, 0, 3, 0, None) == 0
    for kw, word in ((dict(eye=good[3:6]), b"eye"), (dict(up=[1.6, 0.0, 1.0]), b"up"), (dict(up=[0.0, 0.0, 0.0]), b"up"), (dict(fov=0.0), b"fov"), (dict(fov=180.0), b"fov"),
                     (dict(aspect=0.0), b"aspect"), (dict(aspect=-1.0), b"aspect"), (dict(near=0.0), b"near"), (dict(far=0.01), b"far"), (dict(far=0.005), b"far")):
        for flags in (0, _lib.RENDER_CAM_EE):
            assert L.pih_render_cam(fly.h, out.data_ptr(), cam_with(**kw), 64, 48, 0, 3, flags, None) == -2, kw
            msg = L.pih_last_error(fly.h)
            assert b"degenerate camera" in msg and word in msg, (kw, msg)
    with pytest.raises(ValueError):
        fly.render(64, 48, camera=good[:12])
    # the peg-in-hole wrist camera is what it was: against the oracle as tests/test_render.py does, rest pose, 3 envs
    o0 = O.Oracle(3, seed=7)
    o0.set_state(peg.state().cpu().numpy()[:, :O.STATE_WORDS].astype(np.float64))
    a0 = peg.render(64, 48).cpu().numpy(); b0 = o0.render(64, 48)
    assert (a0[..., 0] > 0.9).all() and (a0[..., 0] <= 1.0).all()
    assert (a0[..., 1] == b0[..., 1]).mean() > 0.997 and np.abs(a0[..., 0] - b0[..., 0])[a0[..., 1] == b0[..., 1]].max() < 2e-6


@pytest.mark.gpu
def test_base_env_renders_random_fly(torch_mod, oracle_mod):
    """BaseEnv.render fills `images` for task='random-fly'; every agent's image is the reference's for its own state, so the env offset
    does not enter an env-local camera"""
    from peg_in_hole_gym_amd.envs import BaseEnv
    env = BaseEnv(task="random-fly", task_num=2, offset=[2., 3., 0.], args=["Banana", 1 / 120.])
    env.reset()
    assert env.render() is None
    assert len(env.images) == 2
    st = env._backend.state().cpu().numpy()
    assert np.abs(st[1, _lib.F_OFFSET:_lib.F_OFFSET + 3] - st[0, _lib.F_OFFSET:_lib.F_OFFSET + 3]).max() >= 2.0           # the agents stand apart
    flat = env._backend.render(300, 300).cpu().numpy()
    shaded_err = []
    for e in range(2):
        img = env.images[e]
        assert img.shape == (300, 300, 4) and img.dtype == np.float64
        z, d, c = _check(oracle_mod, img, flat[e].astype(np.float64), st[e], _lib.FLY_CAM_DEFAULT, "env", 0, True)
        print("agent %d: max relative depth error %.3e, depth-buffer value %.3e, shaded colour p99 %.3e median %.3e" % (e, z, d, np.percentile(c, 99), np.median(c)))
        assert z <= DEPTH_REL_TOL and d <= DEPTH_VALUE_TOL
        shaded_err.append(c)
    shaded_err = np.concatenate(shaded_err)
    assert np.percentile(shaded_err, 99) < 0.05 and np.median(shaded_err) < 1e-3
    env.close()
