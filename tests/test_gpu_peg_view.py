"""Free camera of the peg-in-hole task on the GPU: pih_render_view / PihVecEnv.render_view against the numpy fp64 ray caster of
tests/render_ref.py, with the states, cameras, sizes, comparison rules and tolerances (RC.PEG_*_TOL, derived there from the fp32 host
build) of tests/render_cases.py, which tests/test_peg_view.py shares."""
import ctypes as C

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import render_cases as RC
from tests import render_ref as R
from tests.render_cases import (PEG_COLOUR_TOL as COLOUR_TOL, PEG_DEPTH_REL_TOL as DEPTH_REL_TOL, PEG_DEPTH_VALUE_TOL as DEPTH_VALUE_TOL, SHADED_MEDIAN,
                                SHADED_P99)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.fixture(scope="module")
def states(oracle_mod):
    return RC.make_view_states(oracle_mod)


def _peg(n, **kw):
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    return PihVecEnv(n, **kw)


def _tile(states, n):
    """n records: the six states of RC.make_view_states, repeated"""
    return np.ascontiguousarray(states[np.arange(n) % len(states)])


def _check(O, img, seg, rec, cam, frame, shaded, name=None, cache=None):
    """one env's float4 image and seg bytes against the reference under the class share, depth and colour rules"""
    H, W = img.shape[:2]
    key = (rec.tobytes(), tuple(cam), frame, W, H)
    if cache is None or key not in cache:
        ref = R.plain_reference(R.peg_scene(O, rec), cam, W, H, frame)
        if cache is not None:
            cache[key] = ref
    else:
        ref = cache[key]
    rflat, rlit, rseg, rz = ref
    if name is not None:
        RC.peg_check_reference_scene(name, W, H, rseg, cam)
    return RC.compare(img.astype(np.float64), seg, rlit if shaded else rflat, rseg, rz, cam, _lib.SEG_NONE, exact_class=False)


@pytest.mark.gpu
def test_parity_all_cameras_sizes_flat_and_shaded(torch_mod, oracle_mod, states):
    """N = 6: the five cameras, the three sizes, flat and shaded, every env against the reference fed with the handle's own state().  The
    class of a pixel is its seg byte (rgba8 of the same call arguments)."""
    n = 6
    g = _peg(n)
    g.set_state(torch_mod.tensor(states))
    st = g.state().cpu().numpy()
    zmax = dmax = cmax = 0.0; shaded_err = []; cache = {}
    for name in RC.PEG_CAMERA_NAMES:
        for (W, H) in RC.SIZES:
            cam, frame = RC.peg_cameras(W, H)[name]
            flat = g.render_view(W, H, camera=cam, frame=frame).cpu().numpy()
            lit = g.render_view(W, H, camera=cam, frame=frame, shaded=True).cpu().numpy()
            seg = g.render_view(W, H, camera=cam, frame=frame, fmt="rgba8").cpu().numpy()[..., 3]
            assert flat.shape == (n, H, W, 4) and np.array_equal(flat[..., 0], lit[..., 0])          # shading does not touch the depth channel
            for e in range(n):
                z, d, c = _check(oracle_mod, flat[e], seg[e], st[e], cam, frame, False, name, cache)
                zmax = max(zmax, z); dmax = max(dmax, d); cmax = max(cmax, c.max())
                z, d, c = _check(oracle_mod, lit[e], seg[e], st[e], cam, frame, True, None, cache)
                shaded_err.append(c)
    shaded_err = np.concatenate(shaded_err)
    print("max relative depth error %.3e (bound %.3e), depth-buffer value %.3e (%.3e), flat colour %.3e (%.3e), shaded colour p99 %.3e median %.3e max %.3e"
          % (zmax, DEPTH_REL_TOL, dmax, DEPTH_VALUE_TOL, cmax, COLOUR_TOL, np.percentile(shaded_err, 99), np.median(shaded_err), shaded_err.max()))
    assert zmax <= DEPTH_REL_TOL and dmax <= DEPTH_VALUE_TOL and cmax <= COLOUR_TOL
    assert np.percentile(shaded_err, 99) < SHADED_P99 and np.median(shaded_err) < SHADED_MEDIAN
    # no camera means the wrist preset, whatever the frame says
    W, H = 97, 61
    a = g.render_view(W, H).cpu().numpy()
    assert np.array_equal(a, g.render_view(W, H, camera=_lib.VIEW_CAM_WRIST, frame="ee_pos").cpu().numpy())
    assert np.array_equal(a, g.render_view(W, H, frame="ee").cpu().numpy())


NEAR_EYE = 4            # near-plane distances: closer to the eye than this, a hit is one of the pad faces the eye lies on
NEAR_EYE_PIXELS = 2     # per image


@pytest.mark.gpu
def test_wrist_preset_against_pih_render(torch_mod, states):
    """The wrist preset and pih_render of the same handle are two fp32 images of one fp64 truth: class (flat colour) agreement > 0.997,
    depth value on the agreeing pixels within twice the depth-value bound; flat and shaded.
    One kind of agreeing pixel is exempt, counted and capped.  With closed fingers the eye lies ON the faces of the pads (the near-plane
    case of pih_render.h); in fp64 their hits at t ~ 0 are clipped, in fp32 the eye is a rounding error off the face and a grazing ray
    can meet it a millimetre or two out, past the near plane.  Measured on the MI355X: at one pixel of the 97 x 61 rest-pose image both
    kernels draw a pad 2.2 mm from the eye (depth values 0.5366 and 0.5396, 3.0e-3 apart) where the reference sees the table; the hit's
    distance is rounding noise over a grazing angle and no two fp32 evaluations agree on it.  So: an agreeing pixel that either image
    puts closer to the eye than NEAR_EYE near-plane distances (4 mm; nothing else in a scene is that close) is exempt from the depth
    bound, and an image may hold at most NEAR_EYE_PIXELS of them.  Every other agreeing pixel takes the bound."""
    near, far = _lib.VIEW_CAM_WRIST[11], _lib.VIEW_CAM_WRIST[12]
    n = 6
    g = _peg(n)
    g.set_state(torch_mod.tensor(states))
    for (W, H) in ((97, 61), (64, 64)):
        a, b = g.render_view(W, H).cpu().numpy(), g.render(W, H).cpu().numpy()
        same = a[..., 1] == b[..., 1]
        z = near * far / (far - np.minimum(a[..., 0], b[..., 0]).astype(np.float64) * (far - near))      # the nearer of the two eye-space depths
        exempt = same & (z < NEAR_EYE * near)
        bound = same & ~exempt
        print("%dx%d: class agreement %.5f, exempt pixels per image %s, max depth value difference %.3e (bound %.3e; over the exempt ones %.3e)"
              % (W, H, same.mean(), exempt.sum((1, 2)).tolist(), np.abs(a[..., 0] - b[..., 0])[bound].max(), 2 * DEPTH_VALUE_TOL,
                 np.abs(a[..., 0] - b[..., 0])[exempt].max() if exempt.any() else 0.0))
        assert same.mean() > 0.997
        assert (exempt.sum((1, 2)) <= NEAR_EYE_PIXELS).all()
        assert np.abs(a[..., 0] - b[..., 0])[bound].max() <= 2 * DEPTH_VALUE_TOL
        al, bl = g.render_view(W, H, shaded=True).cpu().numpy(), g.render(W, H, shaded=True).cpu().numpy()
        d = np.abs(al[..., 1:] - bl[..., 1:])[bound]
        assert np.percentile(d, 99) < SHADED_P99 and np.median(d) < SHADED_MEDIAN


@pytest.mark.gpu
def test_sub_ranges(torch_mod, oracle_mod, states):
    """N = 70 (not a multiple of the wave): a sub-range renders the same pixels; envs 0, 63, 64 and 69 against the reference"""
    n, (W, H) = 70, (97, 61)
    g = _peg(n)
    g.set_state(torch_mod.tensor(_tile(states, n)))
    st = g.state().cpu().numpy()
    cam, frame = RC.peg_cameras(W, H)["overview"]
    full = g.render_view(W, H, camera=cam).cpu().numpy()
    part = g.render_view(W, H, env_begin=3, env_count=5, camera=cam).cpu().numpy()
    assert part.shape == (5, H, W, 4) and np.array_equal(part, full[3:8])
    seg = g.render_view(W, H, camera=cam, fmt="rgba8").cpu().numpy()[..., 3]
    for e in (0, 63, 64, 69):
        z, d, c = _check(oracle_mod, full[e], seg[e], st[e], cam, frame, False, "overview")
        print("env %d: max relative depth error %.3e, depth-buffer value %.3e, colour %.3e" % (e, z, d, c.max()))
        assert z <= DEPTH_REL_TOL and d <= DEPTH_VALUE_TOL and c.max() <= COLOUR_TOL


def _pack(rgb):
    return np.minimum(255, (rgb + np.float32(0.5)).astype(np.int64)).astype(np.uint8)


@pytest.mark.gpu
def test_packed_formats(torch_mod, states):
    """rgba8 == the pack of the float4 image, bytewise; depth == channel 0, bitwise; flat and shaded, every camera; out= is written in place"""
    torch = torch_mod
    n, (W, H) = 6, (97, 61)
    g = _peg(n)
    g.set_state(torch.tensor(states))
    segs = set()
    for name in RC.PEG_CAMERA_NAMES:
        cam, frame = RC.peg_cameras(W, H)[name]
        for shaded in (False, True):
            f4 = g.render_view(W, H, camera=cam, frame=frame, shaded=shaded).cpu().numpy()
            r8 = g.render_view(W, H, camera=cam, frame=frame, shaded=shaded, fmt="rgba8")
            assert r8.dtype == torch.uint8 and tuple(r8.shape) == (n, H, W, 4)
            r8 = r8.cpu().numpy()
            assert np.array_equal(r8[..., :3], _pack(f4[..., 1:])), (name, shaded)
            dp = g.render_view(W, H, camera=cam, frame=frame, shaded=shaded, fmt="depth")
            assert dp.dtype == torch.float32 and tuple(dp.shape) == (n, H, W)
            assert np.array_equal(dp.cpu().numpy().view(np.uint32), f4[..., 0].view(np.uint32)), (name, shaded)
            segs |= set(np.unique(r8[..., 3]).tolist())
    assert {0, 1, 2, 3, 4, 6, 7, 8, _lib.VIEW_SEG_HOLE, _lib.VIEW_SEG_TABLE, _lib.SEG_NONE} <= segs and 5 not in segs, sorted(segs)
    out = torch.zeros(n, H, W, 4, dtype=torch.uint8, device="cuda")
    assert g.render_view(W, H, out=out, fmt="rgba8") is out and (out[..., 3] != 0).any()
    with pytest.raises(ValueError):
        g.render_view(W, H, out=torch.zeros(n, H, W, 4, device="cuda"), fmt="rgba8")
    with pytest.raises(ValueError):
        g.render_view(W, H, fmt="rgb")
    with pytest.raises(ValueError):
        g.render_view(W, H, frame="world")


@pytest.mark.gpu
def test_per_env_device_cameras(torch_mod, states):
    """Row e of a [count, 13] camera tensor == the single host camera call for that env, bitwise, in all three formats; a degenerate row and
    a NaN row give the background and leave their neighbours alone"""
    torch = torch_mod
    n, (W, H) = 6, (97, 61)
    g = _peg(n)
    g.set_state(torch.tensor(states))
    names = ("overview", "hole close-up", "horizon", "overview", "hole close-up", "horizon")
    rows = [RC.peg_cameras(W, H)[nm][0] for nm in names]
    rows[3] = list(rows[3]); rows[3][0] += 0.2                                     # (not twice the same camera)
    cams = torch.tensor(rows, dtype=torch.float32, device="cuda")
    for frame in ("env", "ee_pos"):
        for fmt in ("float4", "rgba8", "depth"):
            for shaded in (False, True):
                per_env = g.render_view(W, H, camera=cams, frame=frame, fmt=fmt, shaded=shaded).cpu().numpy()
                for e in range(n):
                    one = g.render_view(W, H, env_begin=e, env_count=1, camera=rows[e], frame=frame, fmt=fmt, shaded=shaded).cpu().numpy()
                    assert np.array_equal(per_env[e].view(np.uint8), one[0].view(np.uint8)), (frame, fmt, shaded, e)
    # a sub-range takes its own rows
    part = g.render_view(W, H, env_begin=2, env_count=3, camera=cams[2:5].contiguous(), fmt="rgba8").cpu().numpy()
    assert np.array_equal(part, g.render_view(W, H, camera=cams, fmt="rgba8").cpu().numpy()[2:5])
    good = g.render_view(W, H, camera=cams, fmt="rgba8").cpu().numpy()
    bad = cams.clone()
    bad[1, 3:6] = bad[1, 0:3]                                                      # eye == target
    bad[4, 9] = float("nan")
    for fmt in ("float4", "rgba8", "depth"):
        img = g.render_view(W, H, camera=bad, fmt=fmt, shaded=True).cpu().numpy()
        ref = g.render_view(W, H, camera=cams, fmt=fmt, shaded=True).cpu().numpy()
        for e in (1, 4):
            if fmt == "float4":
                assert (img[e, ..., 0] == 1).all() and (img[e, ..., 1:] == 255).all()
            elif fmt == "rgba8":
                assert (img[e, ..., :3] == 255).all() and (img[e, ..., 3] == _lib.SEG_NONE).all()
            else:
                assert (img[e] == 1).all()
        for e in (0, 2, 3, 5):
            assert np.array_equal(img[e].view(np.uint8), ref[e].view(np.uint8))
    assert (good[1, ..., 3] != _lib.SEG_NONE).any()
    with pytest.raises(ValueError):
        g.render_view(W, H, camera=cams[:4])


@pytest.mark.gpu
def test_tracking_the_peg_tip(torch_mod):
    """tracking_cameras(tip_pose()[:, :3], eye) -> render_view(camera=...): after 40 random steps every env's camera has the pipe capsule
    that carries the peg tip within the central third of its image, without a host round trip; the render calls change no state"""
    from peg_in_hole_gym_amd.vec_env import tracking_cameras
    torch = torch_mod
    n, (W, H) = 6, (96, 96)
    g = _peg(n, seed=31)
    rng = np.random.default_rng(31)
    for _ in range(40):
        g.step(torch.tensor(rng.uniform(-1, 1, (n, 4)), dtype=torch.float32))
    before = g.state().clone()
    tip = g.tip_pose()
    cams = tracking_cameras(tip[:, :3], (0.9, -1.1, 0.7), fov=25.0)
    assert cams.is_cuda and tuple(cams.shape) == (n, _lib.CAM_WORDS)
    seg = g.render_view(W, H, camera=cams, fmt="rgba8")[..., 3].cpu().numpy()
    g.render_view(W, H, camera=cams); g.render_view(W, H, camera=cams, fmt="depth", shaded=True); g.render_view(W, H)
    assert torch.equal(before, g.state())
    grasp = before[:, _lib.S_GRASP].cpu().numpy()
    for e in range(n):
        tip_capsule = _lib.VIEW_SEG_PIPE0 + (0 if grasp[e] == 0 else 23)           # the tip rides on the pipe's first or last link
        rows, cols = np.nonzero(seg[e] == tip_capsule)
        assert len(rows) > 0, (e, sorted(np.unique(seg[e]).tolist()))
        third = ((rows >= H // 3) & (rows < 2 * H // 3) & (cols >= W // 3) & (cols < 2 * W // 3))
        print("env %d: capsule %d owns %d pixels, %d of them in the central third" % (e, tip_capsule, len(rows), third.sum()))
        assert third.all()


@pytest.mark.gpu
def test_errors(torch_mod):
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    torch = torch_mod
    L = _lib.load()
    peg = _peg(3, seed=7)
    fly = PihVecEnv(3, task_id=1, max_episode_steps=480, contact_margin=0.02, dt=1.0 / 120.0)
    out = torch.empty(3, 48, 64, 4, device="cuda")
    view = lambda h, cam, flags, ptr=None: L.pih_render_view(h, out.data_ptr() if ptr is None else ptr, cam, 64, 48, 0, 3, flags, None)
    assert view(peg.h, None, 0) == 0
    assert view(fly.h, None, 0) == -2 and b"peg-in-hole" in L.pih_last_error(fly.h)
    with pytest.raises(ValueError):
        fly.render_view(64, 48)
    assert view(peg.h, None, _lib.RENDER_OUT_RGBA8 | _lib.RENDER_OUT_DEPTH) == -2 and b"exclude" in L.pih_last_error(peg.h)
    assert view(peg.h, None, _lib.RENDER_CAM_EE | _lib.RENDER_CAM_EE_POS) == -2 and b"exclude" in L.pih_last_error(peg.h)
    assert view(peg.h, None, _lib.RENDER_CAM_DEVICE) == -2 and b"PIH_RENDER_CAM_DEVICE" in L.pih_last_error(peg.h)
    for bit in (64, 128, 1 << 20):
        assert view(peg.h, None, bit) == -2 and b"flag" in L.pih_last_error(peg.h)
    assert view(peg.h, None, 0, out.data_ptr() + 4) == -2 and b"aligned" in L.pih_last_error(peg.h)
    assert L.pih_render_view(peg.h, out.data_ptr(), None, 64, 48, 1, 3, 0, None) == -2
    good = list(_lib.VIEW_CAM_OVERVIEW)

    def cam_with(**kw):
        c = list(good)
        for k, v in kw.items():
            i = {"eye": 0, "target": 3, "up": 6, "fov": 9, "aspect": 10, "near": 11, "far": 12}[k]
            c[i:i + (3 if i < 9 else 1)] = v if i < 9 else [v]
        return (C.c_float * _lib.CAM_WORDS)(*c)
    assert view(peg.h, cam_with(), 0) == 0
    view_axis = [good[3 + i] - good[i] for i in range(3)]
    for kw, word in ((dict(eye=good[3:6]), b"eye"), (dict(up=view_axis), b"up"), (dict(up=[0.0, 0.0, 0.0]), b"up"), (dict(fov=0.0), b"fov"), (dict(fov=180.0), b"fov"),
                     (dict(aspect=0.0), b"aspect"), (dict(aspect=-1.0), b"aspect"), (dict(near=0.0), b"near"), (dict(far=0.01), b"far"), (dict(far=0.005), b"far"),
                     (dict(fov=float("nan")), b"fov")):
        for flags in (0, _lib.RENDER_CAM_EE, _lib.RENDER_CAM_EE_POS):
            assert view(peg.h, cam_with(**kw), flags) == -2, kw
            msg = L.pih_last_error(peg.h)
            assert b"degenerate camera" in msg and word in msg, (kw, msg)
    with pytest.raises(ValueError):
        peg.render_view(64, 48, camera=good[:12])
    # the entry points from before keep refusing what they refused
    assert L.pih_render_cam(peg.h, out.data_ptr(), None, 64, 48, 0, 3, 0, None) == -2
    assert L.pih_render_ex(peg.h, out.data_ptr(), 64, 48, 0, 3, _lib.RENDER_OUT_RGBA8, None) == -2
    with pytest.raises(ValueError):
        peg.render(64, 48, camera=good)
    with pytest.raises(ValueError):
        peg.render(64, 48, fmt="rgba8")
    with pytest.raises(ValueError):
        peg.tracking_cameras((1.0, 0.0, 1.0))
