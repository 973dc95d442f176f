"""Output formats and per-env cameras of the random-fly camera on the GPU: pih_render_cam with PIH_RENDER_OUT_RGBA8, PIH_RENDER_OUT_DEPTH
and PIH_RENDER_CAM_DEVICE through PihVecEnv.render(fmt=..., camera=[count, 13]) and PihVecEnv.tracking_cameras, against the numpy fp64
ray caster of tests/render_ref.py.  Rules, caps and the per-env-camera cases come from tests/render_cases.py; the fp32 host build of the
same per-pixel code meets them first in tests/test_fly_image.py."""
import ctypes as C

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import render_cases as RC
from tests import render_ref as R

GUARD = 4096


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


class Guarded:
    """a tensor of the given shape and dtype inside a larger buffer of 0xA5 bytes, GUARD bytes before and after it"""
    def __init__(self, torch, shape, dtype):
        self.torch = torch
        self.nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((2 * GUARD + self.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.nbytes:] == 0xA5).all())


def _render_guarded(torch, g, W, H, fmt, count=None, **kw):
    count = g.n if count is None else count
    shape, dtype = {"rgba8": ((count, H, W, 4), torch.uint8), "depth": ((count, H, W), torch.float32), "float4": ((count, H, W, 4), torch.float32)}[fmt]
    box = Guarded(torch, shape, dtype)
    out = g.render(W, H, out=box.view, fmt=fmt, env_count=count, **kw)
    assert out.data_ptr() == box.view.data_ptr() and out.shape == shape and out.dtype == dtype
    res = out.cpu().numpy()
    assert box.intact(), "bytes outside the image were written (%s, %dx%d)" % (fmt, W, H)
    assert not (fmt == "rgba8" and W * H > 64 and (res == 0xA5).all()), "the image was not written"
    return res


def _check_packed(scene, fig, rgba_flat, rgba_lit, depth, cam, frame, ref):
    """one env's three images against the reference, into the running figures"""
    assert np.array_equal(rgba_flat[..., 3], rgba_lit[..., 3])                             # shading does not touch the segmentation
    same = RC.check_seg(scene, rgba_flat[..., 3], cam, frame, ref, exact=False)
    fig.add_depth(RC.depth_errors(depth, same, ref, cam))
    fig.add_colour(RC.colour_excess(rgba_flat[..., :3], same, ref[0]), False)
    fig.add_colour(RC.colour_excess(rgba_lit[..., :3], same, ref[1]), True)


@pytest.mark.gpu
@pytest.mark.parametrize("obj", [0, 1])
def test_formats_all_cameras_and_sizes(torch_mod, oracle_mod, obj):
    """N = 6, the four cameras, RC.SIZES plus (5, 3): rgba8 flat and shaded, and depth, every env against the reference fed with the handle's
    own state(); every call writes into a guarded view"""
    n = 6
    g = RC.fly_handle(n, object_id=obj)
    fig = RC.Figures()
    for name in RC.FLY_CAMERA_NAMES:
        g.set_state(torch_mod.tensor(RC.make_fly_states(oracle_mod, obj, n, seed=RC.SCENE_SEED[(obj, name)], eye_in_hand=name == "eye-in-hand")))
        st = g.state().cpu().numpy()
        for (W, H) in RC.IMAGE_SIZES:
            cam, frame = RC.fly_cameras(W, H)[name]
            flat = _render_guarded(torch_mod, g, W, H, "rgba8", camera=cam, ee_frame=frame == "ee")
            lit = _render_guarded(torch_mod, g, W, H, "rgba8", camera=cam, ee_frame=frame == "ee", shaded=True)
            depth = _render_guarded(torch_mod, g, W, H, "depth", camera=cam, ee_frame=frame == "ee")
            assert np.array_equal(depth, _render_guarded(torch_mod, g, W, H, "depth", camera=cam, ee_frame=frame == "ee", shaded=True))
            for e in range(n):
                scene = R.fly_scene(oracle_mod, st[e], obj)
                ref = R.plain_reference(scene, cam, W, H, frame)
                RC.fly_check_reference_scene(name, W, H, ref[2], obj)
                _check_packed(scene, fig, flat[e], lit[e], depth[e], cam, frame, ref)
    print("object %d: %s" % (obj, fig.text()))
    fig.limits()


@pytest.mark.gpu
def test_depth_plane_is_the_float4_depth(torch_mod, oracle_mod):
    n, obj = 6, 0
    g = RC.fly_handle(n, object_id=obj)
    g.set_state(torch_mod.tensor(RC.make_fly_states(oracle_mod, obj, n, seed=RC.SCENE_SEED[(obj, "close-up")])))
    worst = 0.0
    for (W, H) in RC.IMAGE_SIZES:
        cam, frame = RC.fly_cameras(W, H)["close-up"]
        depth = g.render(W, H, camera=cam, fmt="depth").cpu().numpy()
        img = g.render(W, H, camera=cam).cpu().numpy()
        assert depth.shape == (n, H, W) and depth.dtype == np.float32
        worst = max(worst, float(np.abs(depth - img[..., 0]).max()))
    print("max |depth plane - float4 channel 0| = %.3e (0 expected)" % worst)
    assert worst <= RC.FLY_DEPTH_VALUE_TOL


def _case_handle(torch, case):
    g = RC.fly_handle(len(case["states"]), object_id=case["obj"])
    g.set_state(torch.tensor(case["states"]))
    return g, g.state().cpu().numpy(), torch.tensor(case["cams"], device="cuda")


@pytest.mark.gpu
def test_per_env_cameras(torch_mod, oracle_mod):
    """N = 70: the camera of env e is row e of a device tensor (three cameras in turn); the full range and env_begin = 3, env_count = 5,
    where row e belongs to env 3 + e.  The envs of RC.per_env_cases against the reference rendered with their own row, and bit for bit
    against a call with that row as the one host camera: both calls run the same kernel instance."""
    case = RC.per_env_cases(oracle_mod)["cycle"]
    (W, H), obj, cams = case["size"], case["obj"], case["cams"]
    g, st, cams_dev = _case_handle(torch_mod, case)
    f4 = _render_guarded(torch_mod, g, W, H, "float4", camera=cams_dev)
    u8 = _render_guarded(torch_mod, g, W, H, "rgba8", camera=cams_dev)
    dp = _render_guarded(torch_mod, g, W, H, "depth", camera=cams_dev)
    sub = cams_dev[3:8].contiguous()
    assert np.array_equal(_render_guarded(torch_mod, g, W, H, "float4", count=5, env_begin=3, camera=sub), f4[3:8])
    assert np.array_equal(_render_guarded(torch_mod, g, W, H, "rgba8", count=5, env_begin=3, camera=sub), u8[3:8])
    assert np.array_equal(g.render(W, H, camera=cams[3:8].tolist(), env_begin=3, env_count=5, fmt="rgba8").cpu().numpy(), u8[3:8])      # converted and uploaded
    fig = RC.Figures(); zmax = dmax = cmax = 0.0
    for e in case["checked"]:
        scene = R.fly_scene(oracle_mod, st[e], obj)
        ref = R.plain_reference(scene, cams[e], W, H)
        same = RC.check_seg(scene, u8[e][..., 3], cams[e], "env", ref, exact=False)
        fig.add_depth(RC.depth_errors(dp[e], same, ref, cams[e]))
        fig.add_colour(RC.colour_excess(u8[e][..., :3], same, ref[0]), False)
        z, d, c = RC.compare(f4[e].astype(np.float64), R.classify(f4[e].astype(np.float64), obj), ref[0], ref[2], ref[3], cams[e], R.BG, exact_class=False)
        zmax = max(zmax, z); dmax = max(dmax, d); cmax = max(cmax, c.max())
        # the same env with its row as the single host camera
        one4 = g.render(W, H, camera=cams[e].tolist(), env_begin=e, env_count=1).cpu().numpy()[0]
        one8 = g.render(W, H, camera=cams[e].tolist(), env_begin=e, env_count=1, fmt="rgba8").cpu().numpy()[0]
        assert np.array_equal(one4, f4[e]) and np.array_equal(one8, u8[e]), "env %d: the per-env call and the single-camera call differ" % e
    print("per-env cameras: %s; float4: max relative depth error %.3e, depth-buffer value %.3e, colour %.3e; bit-identical to the single-camera calls"
          % (fig.text(), zmax, dmax, cmax))
    fig.limits()
    assert zmax <= RC.FLY_DEPTH_REL_TOL and dmax <= RC.FLY_DEPTH_VALUE_TOL and cmax <= RC.FLY_COLOUR_TOL


@pytest.mark.gpu
def test_per_env_eye_in_hand_cameras(torch_mod, oracle_mod):
    """N = 6: rows that differ in fov (50 .. 70 degrees), given in each env's ee_link frame"""
    case = RC.per_env_cases(oracle_mod)["eye-in-hand"]
    (W, H), obj, cams = case["size"], case["obj"], case["cams"]
    g, st, cams_dev = _case_handle(torch_mod, case)
    flat = _render_guarded(torch_mod, g, W, H, "rgba8", camera=cams_dev, ee_frame=True)
    lit = _render_guarded(torch_mod, g, W, H, "rgba8", camera=cams_dev, ee_frame=True, shaded=True)
    depth = _render_guarded(torch_mod, g, W, H, "depth", camera=cams_dev, ee_frame=True)
    fig = RC.Figures()
    for e in case["checked"]:
        scene = R.fly_scene(oracle_mod, st[e], obj)
        ref = R.plain_reference(scene, cams[e], W, H, "ee")
        RC.fly_check_reference_scene("eye-in-hand", W, H, ref[2], obj)
        _check_packed(scene, fig, flat[e], lit[e], depth[e], cams[e], "ee", ref)
    print("per-env eye-in-hand: %s" % fig.text())
    fig.limits()


@pytest.mark.gpu
def test_degenerate_rows_give_the_background(torch_mod, oracle_mod):
    """N = 6: row 2 has eye == target, row 4 fov = NaN: those two images are background and finite, the other four are what they were"""
    case = RC.per_env_cases(oracle_mod)["degenerate"]
    (W, H), obj, cams = case["size"], case["obj"], case["cams"]
    assert case["degenerate"] == (2, 4)
    g, st, cams_dev = _case_handle(torch_mod, case)
    u8 = _render_guarded(torch_mod, g, W, H, "rgba8", camera=cams_dev)
    lit = _render_guarded(torch_mod, g, W, H, "rgba8", camera=cams_dev, shaded=True)
    dp = _render_guarded(torch_mod, g, W, H, "depth", camera=cams_dev)
    f4 = _render_guarded(torch_mod, g, W, H, "float4", camera=cams_dev, shaded=True)
    assert np.isfinite(dp).all() and np.isfinite(f4).all()
    for e in case["degenerate"]:
        assert (dp[e] == 1.0).all() and (u8[e] == 255).all() and (lit[e] == 255).all()
        assert (f4[e][..., 0] == 1.0).all() and (f4[e][..., 1:] == 255.0).all()
    fig = RC.Figures()
    for e in case["checked"]:
        scene = R.fly_scene(oracle_mod, st[e], obj)
        ref = R.plain_reference(scene, cams[e], W, H)
        _check_packed(scene, fig, u8[e], lit[e], dp[e], cams[e], "env", ref)
        assert np.abs(f4[e][..., 0] - dp[e]).max() <= RC.FLY_DEPTH_VALUE_TOL
    print("rows next to degenerate ones: %s" % fig.text())
    fig.limits()


@pytest.mark.gpu
def test_tracking_cameras_follow_the_object(torch_mod, oracle_mod):
    """after reset and 40 steps every env is seen from (1.2, 0.6, 0.9) looking at its own object, cameras built on the device"""
    n, obj, (W, H) = 6, 0, (61, 61)
    g = RC.fly_handle(n, object_id=obj, auto_reset=0)
    g.reset(seed=11)
    rng = np.random.default_rng(11)
    for _ in range(40):
        g.step(torch_mod.tensor(rng.uniform(-1, 1, (n, 6)), dtype=torch_mod.float32))
    cams_dev = g.tracking_cameras(eye=(1.2, 0.6, 0.9))
    assert cams_dev.shape == (n, _lib.CAM_WORDS) and cams_dev.is_cuda and cams_dev.dtype == torch_mod.float32
    u8 = g.render(W, H, camera=cams_dev, fmt="rgba8").cpu().numpy()
    dp = g.render(W, H, camera=cams_dev, fmt="depth").cpu().numpy()
    st = g.state().cpu().numpy(); cams = cams_dev.cpu().numpy()
    assert np.array_equal(cams[:, 3:6], st[:, _lib.F_OPOS:_lib.F_OPOS + 3])
    fig = RC.Figures(); centred = 0
    for e in range(n):
        scene = R.fly_scene(oracle_mod, st[e], obj)
        ref = R.plain_reference(scene, cams[e], W, H)
        same = RC.check_seg(scene, u8[e][..., 3], cams[e], "env", ref, exact=False)
        fig.add_depth(RC.depth_errors(dp[e], same, ref, cams[e]))
        fig.add_colour(RC.colour_excess(u8[e][..., :3], same, ref[0]), False)
        if ref[2][H // 2, W // 2] == R.OBJECT:
            centred += 1
            assert u8[e][H // 2, W // 2, 3] == _lib.SEG_OBJECT
    print("tracking cameras: the object is on the centre pixel of %d of %d reference images; %s" % (centred, n, fig.text()))
    fig.limits()


@pytest.mark.gpu
def test_errors(torch_mod):
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    torch = torch_mod
    L = _lib.load()
    fly = RC.fly_handle(3)
    out = torch.empty(3, 48, 64, 4, device="cuda")
    cams = torch.tensor([_lib.FLY_CAM_DEFAULT] * 3, device="cuda")
    both = _lib.RENDER_OUT_RGBA8 | _lib.RENDER_OUT_DEPTH
    assert L.pih_render_cam(fly.h, out.data_ptr(), None, 64, 48, 0, 3, both, None) == -2
    assert L.pih_render_cam(fly.h, out.data_ptr(), None, 64, 48, 0, 3, _lib.RENDER_CAM_DEVICE, None) == -2
    assert b"PIH_RENDER_CAM_DEVICE" in L.pih_last_error(fly.h)
    assert L.pih_render_cam(fly.h, out.data_ptr(), None, 64, 48, 0, 3, 32, None) == -2                         # a bit nobody defined
    assert L.pih_render_cam(fly.h, out.data_ptr(), C.c_void_p(cams.data_ptr()), 64, 48, 0, 3, _lib.RENDER_CAM_DEVICE, None) == 0
    peg = PihVecEnv(3, seed=7)
    assert L.pih_render_ex(peg.h, out.data_ptr(), 64, 48, 0, 3, _lib.RENDER_OUT_RGBA8, None) == -2
    assert b"flag" in L.pih_last_error(peg.h)
    assert L.pih_render_ex(peg.h, out.data_ptr(), 64, 48, 0, 3, _lib.RENDER_SHADED, None) == 0
    with pytest.raises(ValueError):
        peg.render(64, 48, fmt="rgba8")
    with pytest.raises(ValueError):
        fly.render(64, 48, fmt="rgb")
    with pytest.raises(ValueError):
        fly.render(64, 48, fmt="rgba8", out=out)                                                               # float32 where uint8 is due
    with pytest.raises(ValueError):
        fly.render(64, 48, fmt="depth", out=torch.empty(3, 48, 64, 4, device="cuda"))                          # the shape of another format
    with pytest.raises(ValueError):
        fly.render(64, 48, fmt="rgba8", out=torch.empty(3, 48, 64, 4, dtype=torch.uint8))                      # on the host
    with pytest.raises(ValueError):
        fly.render(64, 48, camera=torch.zeros(3, 12, device="cuda"))
    with pytest.raises(ValueError):
        fly.render(64, 48, camera=cams[:2].contiguous())
    with pytest.raises(ValueError):
        fly.render(64, 48, camera=cams, env_begin=1, env_count=2)
    img = fly.render(64, 48)
    assert img.shape == (3, 48, 64, 4) and img.dtype == torch.float32 and bool(torch.isfinite(img).all())
    assert fly.render(64, 48, fmt="rgba8").dtype == torch.uint8
