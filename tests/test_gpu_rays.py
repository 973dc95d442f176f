"""Batched ray tests on the GPU: pih_ray_test / PihVecEnv.ray_test against the numpy fp64 ray caster of tests/render_ref.py by the rule of
tests/ray_cases.py at G_GPU and FLAT_GPU (two grid steps above what the fp32 host build needs), on handles of 4 envs of both tasks and
both objects: the ray counts at the lane, wavefront, workgroup and chunk boundaries, env ranges, shared and per-env rays, both frames,
IGNORE_ROBOT, guard words, bit-for-bit independence of the launch shape, bad rays, argument checks, the cross-check against the shipped
cameras and the README's example."""
import os
import re

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import ray_cases as RY
from tests import render_cases as RC
from tests import render_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 257, 600)       # one lane; one short of a wavefront; a wavefront; one past it; one past a workgroup; three chunks, the last partial
RANGES = ((1, 1), (1, 3))               # (env_begin, env_count)
TASKS = ("peg", "fly0", "fly1")
GUARD = -12345.0
N = 4


class Bed:
    """a handle of 4 envs with states of the host tests written into it, the reference scene of each env (from the handle's own state()),
    and a pool of 1024 aimed rays per env, shuffled (the family is ordered by the kind of target)"""

    def __init__(self, O, task):
        import torch
        from peg_in_hole_gym_amd.vec_env import PihVecEnv
        self.task, self.obj = ("peg", None) if task == "peg" else ("fly", int(task[3]))
        if self.task == "peg":
            self.env = PihVecEnv(N)
            states = RC.make_view_states(O)[[0, 3, 4, 5]]             # the rest pose, a reset, the scripted episode, 40 random steps
        else:
            self.env = RC.fly_handle(N, object_id=self.obj)
            states = RC.make_fly_states(O, self.obj, RY.FLY_STATES_PER_OBJECT, RY.FLY_SEED[self.obj])[[0, 1, 2, 0]]
        self.env.set_state(torch.tensor(states))
        self.rec = self.env.state().cpu().numpy()
        assert np.array_equal(self.rec[:, :states.shape[1]][:, :18], states[:, :18])
        self.scene = [R.peg_scene(O, r) if self.task == "peg" else R.fly_scene(O, r, self.obj) for r in self.rec]
        perm = np.random.default_rng(7).permutation(RY.N_AIMED)
        self.pool = np.stack([RY.aimed_rays(sc, 20 + e)[perm] for e, sc in enumerate(self.scene)])

    def call(self, rays, begin, count, flags, expect=0):
        """pih_ray_test with 64 guard words behind the output -> records float32 [count, R, 8]"""
        import torch
        rays = torch.as_tensor(np.ascontiguousarray(rays, dtype=np.float32)).to(self.env.device)
        R_ = rays.shape[-2]
        size = count * R_ * 8
        buf = torch.full((size + 64,), GUARD, device=self.env.device, dtype=torch.float32)
        with torch.cuda.device(self.env.device):
            rc = self.env.L.pih_ray_test(self.env.h, buf.data_ptr(), rays.data_ptr(), R_, begin, count, flags, self.env._stream())
        assert rc == expect, self.env.L.pih_last_error(self.env.h)
        out = buf.cpu().numpy()
        assert (out[size:] == GUARD).all(), "pih_ray_test wrote behind its output"
        assert not (out[:size] == GUARD).any(), "pih_ray_test left output words unwritten"
        return out[:size].reshape(count, R_, 8)

    def case(self, e, rays, frame, ignore):
        return dict(task=self.task, obj=self.obj, state=e, rec=self.rec[e], scene=self.scene[e], name="gpu", rays=rays, frame=frame, ignore=ignore, flags=0)


@pytest.fixture(scope="module")
def beds(oracle_mod):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    made = {}

    def get(task):
        if task not in made:
            made[task] = Bed(oracle_mod, task)
        return made[task]

    yield get
    for b in made.values():
        b.env.close()


@pytest.mark.parametrize("task", TASKS)
def test_per_env_rays_at_every_size_and_env_range(beds, task):
    """rays_per_env in SIZES x the env ranges, one ray set per env, env-local frame: every env's records against the reference; guard words
    survive, no output word stays unwritten"""
    b = beds(task)
    use = 0.0
    for R_ in SIZES:
        for begin, count in RANGES:
            rays = b.pool[begin:begin + count, :R_]
            out = b.call(rays, begin, count, 0)
            for k in range(count):
                use = max(use, RY.check(b.case(begin + k, rays[k], "env", False), RY.G_GPU, RY.FLAT_GPU, out[k])["use"])
    print("%s: largest bracket use %.3f at G = %g" % (task, use, RY.G_GPU))


@pytest.mark.parametrize("task", TASKS)
def test_flags_against_the_reference(beds, task):
    """shared rays in the end-effector frame (a ray_fan) with and without IGNORE_ROBOT, shared aimed rays with IGNORE_ROBOT, per-env rays in
    the end-effector frame; and PihVecEnv.ray_test gives the same bits as the raw calls"""
    import torch
    b = beds(task)
    fan = RY.fan_rays(b.scene[0])
    axis = np.array([0.0, 0.0, 1.0] if b.task == "peg" else [1.0, 0.0, 0.0])
    on_device = b.env.ray_fan(RY.FAN_AHEAD * axis, axis, **RY.FAN)          # (the device's sin and cos are not the host's to the last bit)
    assert on_device.device.type == "cuda" and np.abs(on_device.cpu().numpy() - fan).max() <= 1e-6
    shared = b.pool[1, :257]
    for rays, frame, ignore in ((fan, "ee", False), (fan, "ee", True), (shared, "env", True), (shared, "env", False)):
        flags = _lib.RAY_SHARED | (_lib.RAY_FRAME_EE if frame == "ee" else 0) | (_lib.RAY_IGNORE_ROBOT if ignore else 0)
        out = b.call(rays, 0, N, flags)
        for e in range(N):
            RY.check(b.case(e, rays, frame, ignore), RY.G_GPU, RY.FLAT_GPU, out[e])
        assert np.array_equal(out, b.env.ray_test(torch.tensor(rays), frame=frame, ignore_robot=ignore).cpu().numpy())
    fans = np.stack([fan, fan[::-1], fan, fan[::-1]])
    out = b.call(fans, 0, N, _lib.RAY_FRAME_EE)
    for e in range(N):
        RY.check(b.case(e, fans[e], "ee", False), RY.G_GPU, RY.FLAT_GPU, out[e])
    assert np.array_equal(out[1:3], b.env.ray_test(fans[1:3], frame="ee", env_begin=1, env_count=2).cpu().numpy())
    with pytest.raises(ValueError):
        b.env.ray_test(fans[:3])
    with pytest.raises(ValueError):
        b.env.ray_test(fan[:, :5])
    with pytest.raises(ValueError):
        b.env.ray_test(fan, frame="ee_pos")
    with pytest.raises(ValueError):
        b.env.ray_test(fan, out=torch.empty(N, len(fan), 8, dtype=torch.float64, device=b.env.device))


@pytest.mark.parametrize("task", ("peg", "fly0"))
def test_results_do_not_depend_on_the_launch_shape(beds, task, monkeypatch):
    """bit for bit: shared rays == the same rays tiled per env; the first 64 rays of the 600-ray call == the 64-ray call; an env range ==
    the rows of the whole call; every chunk size, chosen through the library's measurement switch.  The kernels without the
    bounding-sphere rejection (the other switch) are another compilation of the same code under -ffast-math: they name the same
    primitives and meet the reference by the same rule, in every chunk size bit for bit the same among themselves"""
    b = beds(task)
    rays = b.pool[2, :600]
    base = b.call(rays, 0, N, _lib.RAY_SHARED)
    assert np.array_equal(base, b.call(np.tile(rays, (N, 1, 1)), 0, N, 0))
    assert np.array_equal(base[:, :64], b.call(rays[:64], 0, N, _lib.RAY_SHARED))
    assert np.array_equal(base[1:4], b.call(rays, 1, 3, _lib.RAY_SHARED))
    monkeypatch.setenv("PIH_RAY_CULL", "0")
    plain = b.call(rays, 0, N, _lib.RAY_SHARED)
    assert np.array_equal(plain[..., 1], base[..., 1])
    for e in range(N):
        RY.check(b.case(e, rays, "env", False), RY.G_GPU, RY.FLAT_GPU, plain[e])
    for cull, want in (("0", plain), ("1", base)):
        monkeypatch.setenv("PIH_RAY_CULL", cull)
        for chunk in ("1", "2", "4"):
            monkeypatch.setenv("PIH_RAY_CHUNK", chunk)
            assert np.array_equal(want, b.call(rays, 0, N, _lib.RAY_SHARED)), (cull, chunk)


@pytest.mark.parametrize("task", ("peg", "fly1"))
def test_bad_rays_are_isolated(beds, task):
    """a zero-length ray and rays with NaN / Inf / huge words, among good ones: the miss record with `to` as given, in both frames; the
    good rays' records are what they are without the bad ones"""
    b = beds(task)
    rays, bad = RY.bad_ray_block()
    for flags in (_lib.RAY_SHARED, _lib.RAY_SHARED | _lib.RAY_IGNORE_ROBOT):
        out = b.call(rays, 0, N, flags)
        for e in range(N):
            RY.check_bad_rays(out[e], rays, bad)
    good = [r for r in range(len(rays)) if r not in bad]
    out = b.call(rays, 0, N, _lib.RAY_SHARED | _lib.RAY_FRAME_EE)
    for e in range(N):
        for r in bad:
            assert out[e, r, 0] == 1 and out[e, r, 1] == _lib.SEG_NONE and np.array_equal(out[e, r, 2:5], rays[r, 3:], equal_nan=True) and (out[e, r, 5:] == 0).all()
    assert np.array_equal(out[:, good], b.call(rays[good], 0, N, _lib.RAY_SHARED | _lib.RAY_FRAME_EE))


@pytest.mark.parametrize("task", ("peg", "fly0"))
def test_argument_checks(beds, task):
    """every -2 that needs a handle, with the argument named"""
    import torch
    b = beds(task); env = b.env; L = env.L
    rays = torch.zeros(4 * 8 * 6 + 4, device=env.device); out = torch.zeros(4 * 8 * 8 + 4, device=env.device)
    r, o = rays.data_ptr(), out.data_ptr()
    assert r % 16 == 0 and o % 16 == 0
    bad = (("out_dev", (None, r, 8, 0, 4, 0)), ("rays_dev", (o, None, 8, 0, 4, 0)), ("rays_per_env", (o, r, 0, 0, 4, 0)), ("rays_per_env", (o, r, (1 << 20) + 1, 0, 4, 0)),
           ("env_begin / env_count", (o, r, 8, -1, 2, 0)), ("env_begin / env_count", (o, r, 8, 0, 0, 0)), ("env_begin / env_count", (o, r, 8, 2, 3, 0)),
           ("env_begin / env_count", (o, r, 8, 5, 1, 0)), ("flags", (o, r, 8, 0, 4, 8)), ("flags", (o, r, 8, 0, 4, -1)), ("out_dev", (o + 4, r, 8, 0, 4, 0)),
           ("rays_dev", (o, r + 8, 8, 0, 4, 0)))
    for name, args in bad:
        with torch.cuda.device(env.device):
            assert L.pih_ray_test(env.h, *args, env._stream()) == -2, (name, args)
        assert L.pih_last_error(env.h).decode().startswith("pih_ray_test: " + name + " "), (name, L.pih_last_error(env.h))
    with torch.cuda.device(env.device):
        assert L.pih_ray_test(env.h, o, r, 8, 0, 4, 0, env._stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("task", TASKS)
def test_rays_through_pixel_centres_agree_with_the_camera(beds, task):
    """the shipped cameras at 40 x 30, the overview camera (peg-in-hole: render_view; random-fly: render): the ray through a pixel's centre,
    from the eye to the far plane, names the pixel's seg byte on >= 1 - CLASS_SHARE of the pixels, and where it does its eye-space depth
    t (d . f) agrees with the depth image's within the camera tests' bound"""
    b = beds(task)
    W, H = 40, 30
    if b.task == "peg":
        cam, frame = RC.peg_cameras(W, H)["overview"]; tol = RC.PEG_DEPTH_REL_TOL
        seg = b.env.render_view(W, H, camera=cam, frame=frame, fmt="rgba8").cpu().numpy()[..., 3]
        depth = b.env.render_view(W, H, camera=cam, frame=frame, fmt="depth").cpu().numpy()
    else:
        cam, frame = RC.fly_cameras(W, H)["overview"]; tol = RC.FLY_DEPTH_REL_TOL
        seg = b.env.render(W, H, camera=cam, fmt="rgba8").cpu().numpy()[..., 3]
        depth = b.env.render(W, H, camera=cam, fmt="depth").cpu().numpy()
    eye, d, df, near, far = R.camera_rays(b.scene[0], cam, W, H, frame)
    rays = np.concatenate([np.tile(eye, (W * H, 1)), eye + d * (far / df)[:, None]], axis=1).astype(np.float32)
    length = np.linalg.norm(rays[:, 3:].astype(np.float64) - rays[:, :3], axis=1)
    out = b.call(rays, 0, N, _lib.RAY_SHARED).astype(np.float64)
    for e in range(N):
        same = out[e, :, 1] == seg[e].reshape(-1)
        assert (~same).mean() <= RC.CLASS_SHARE, (e, (~same).sum())
        hit = same & (out[e, :, 1] != _lib.SEG_NONE)
        assert hit.sum() > W * H // 2
        z_img = RC.linear_depth(depth[e].reshape(-1), cam)
        assert np.abs(out[e, hit, 0] * length[hit] * df[hit] / z_img[hit] - 1).max() <= tol


def test_readme_example(beds):
    """the usage example of README.md, run verbatim"""
    import torch
    md = open(os.path.join(ROOT, "README.md")).read()
    code = re.search(r"```python\n(# a proximity ring on the hand.*?)```", md, re.S).group(1)
    scope = {}
    exec(code, scope)
    env, hits, rng = scope["env"], scope["hits"], scope["distance"]
    torch.cuda.synchronize()
    assert tuple(hits.shape) == (env.n, 25, 8) and tuple(rng.shape) == (env.n, 25) and bool(((rng > 0) & (rng <= 0.3)).all())
    assert bool((scope["clear"] == (hits[..., 1] == _lib.SEG_NONE)).all())
    env.close()
