"""Batched closest-point queries on the GPU: pih_closest_points / PihVecEnv.closest_points against the fp64 reference distances by the
rule of tests/dist_cases.py at G_GPU (two grid steps above what the fp32 host build needs), on handles of 4 envs of both tasks and both
objects: the query counts at the lane, wavefront, workgroup and chunk boundaries, env ranges, shared and per-env queries, both frames,
every single group and mixed masks, guard words, bit-for-bit independence of the launch shape, bad queries, argument checks, the
cross-check against pih_ray_test on the same handle and the README's example."""
import os
import re

import numpy as np
import pytest

from peg_in_hole_gym_amd import _lib
from tests import dist_cases as DC
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
ALL = _lib.GROUP_ALL
USE = {}                                # task -> the largest share of G_GPU a record used, printed by the last test


class Bed:
    """a handle of 4 envs with states of the host tests written into it, the reference scene of each env (from the handle's own state()),
    and a pool of 1024 near queries per env"""

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
        self.pool = np.stack([DC.near_points(sc, 20 + e) for e, sc in enumerate(self.scene)])

    def raw(self, buf, points, begin, count, flags, groups):
        import torch
        with torch.cuda.device(self.env.device):
            return self.env.L.pih_closest_points(self.env.h, buf.data_ptr(), points.data_ptr(), points.shape[-2], groups, begin, count, flags, self.env._stream())

    def call(self, points, begin, count, flags, groups=ALL):
        """pih_closest_points with 64 guard words behind the output -> records float32 [count, P, 8]"""
        import torch
        points = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32)).to(self.env.device)
        P = points.shape[-2]
        size = count * P * 8
        buf = torch.full((size + 64,), GUARD, device=self.env.device, dtype=torch.float32)
        rc = self.raw(buf, points, begin, count, flags, groups)
        assert rc == 0, self.env.L.pih_last_error(self.env.h)
        out = buf.cpu().numpy()
        assert (out[size:] == GUARD).all(), "pih_closest_points wrote behind its output"
        assert not (out[:size] == GUARD).any(), "pih_closest_points left output words unwritten"
        return out[:size].reshape(count, P, 8)

    def case(self, e, points, frame, groups):
        return dict(task=self.task, obj=self.obj, state=e, rec=self.rec[e], scene=self.scene[e], name="gpu", points=points, frame=frame, groups=groups, flags=0)

    def check(self, e, points, frame, groups, out):
        res = DC.check(self.case(e, points, frame, groups), DC.G_GPU, out)
        key = "%s%s" % (self.task, "" if self.obj is None else self.obj)
        USE[key] = max(USE.get(key, 0.0), res["use"])
        return res


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
    print("largest use of G_GPU = %g per task: %s" % (DC.G_GPU, {k: round(v, 3) for k, v in USE.items()}))


@pytest.mark.parametrize("task", TASKS)
def test_per_env_queries_at_every_size_and_env_range(beds, task):
    """points_per_env in SIZES x the env ranges, one query set per env, env-local frame, all groups: every env's records against the
    reference; guard words survive, no output word stays unwritten"""
    b = beds(task)
    for P in SIZES:
        for begin, count in RANGES:
            points = b.pool[begin:begin + count, :P]
            out = b.call(points, begin, count, 0)
            for k in range(count):
                b.check(begin + k, points[k], "env", ALL, out[k])
    print("%s: largest use of G %.3f at G = %g" % (task, max(USE.values()), DC.G_GPU))


@pytest.mark.parametrize("task", TASKS)
def test_groups_frames_and_the_python_call(beds, task):
    """shared queries against every single group of the task and two mixed masks; shared and per-env queries in the end-effector frame;
    PihVecEnv.closest_points gives the same bits as the raw calls, with group names, with a reach column and with the scalar reach"""
    import torch
    b = beds(task)
    shared = b.pool[1, :257]
    names = {v: k for k, v in _lib.GROUPS.items()}
    mixed = (_lib.GROUP_ARM | _lib.GROUP_TABLE, ALL & ~_lib.GROUP_ARM)
    for groups in DC.task_groups(b.task) + mixed:
        out = b.call(shared, 0, N, _lib.RAY_SHARED, groups)
        for e in range(N):
            b.check(e, shared, "env", groups, out[e])
        by_name = tuple(names[g] for g in names if g & groups)
        assert np.array_equal(out, b.env.closest_points(torch.tensor(shared), groups=by_name).cpu().numpy()), groups
        assert np.array_equal(out, b.env.closest_points(shared, groups=groups).cpu().numpy()), groups
    lattice = DC.ee_points()
    out = b.call(lattice, 0, N, _lib.RAY_SHARED | _lib.RAY_FRAME_EE)
    for e in range(N):
        b.check(e, lattice, "ee", ALL, out[e])
    assert np.array_equal(out, b.env.closest_points(lattice, frame="ee").cpu().numpy())
    per_env = np.stack([lattice, lattice[::-1], lattice, lattice[::-1]])
    out = b.call(per_env, 0, N, _lib.RAY_FRAME_EE)
    for e in range(N):
        b.check(e, per_env[e], "ee", ALL, out[e])
    assert np.array_equal(out[1:3], b.env.closest_points(per_env[1:3], frame="ee", env_begin=1, env_count=2).cpu().numpy())
    # three columns and the scalar reach == a fourth column of that reach; `out` is used in place
    q = shared.copy(); q[:, 3] = 0.07
    buf = torch.empty(N, len(q), 8, device=b.env.device)
    assert b.env.closest_points(q[:, :3], reach=0.07, groups="table", out=buf) is buf
    assert np.array_equal(buf.cpu().numpy(), b.call(q, 0, N, _lib.RAY_SHARED, _lib.GROUP_TABLE))
    for bad in (dict(points=per_env[:3]), dict(points=lattice[:, :2]), dict(points=lattice, frame="ee_pos"), dict(points=lattice, groups=("pipe",)),
                dict(points=lattice, reach=0.1), dict(points=lattice[:, :3]), dict(points=lattice, out=torch.empty(N, len(lattice), 8, dtype=torch.float64, device=b.env.device))):
        with pytest.raises(ValueError):
            b.env.closest_points(**bad)
    with pytest.raises(_lib.PihError):
        b.env.closest_points(lattice, groups=0)


@pytest.mark.parametrize("task", ("peg", "fly0"))
def test_results_do_not_depend_on_the_launch_shape(beds, task, monkeypatch):
    """bit for bit: shared queries == the same queries tiled per env; the first 64 of the 600-query call == the 64-query call; an env range
    == the rows of the whole call; every chunk size, chosen through the library's measurement switch.  The kernels without the
    bounding-sphere rejection (the other switch) are another compilation of the same code under -ffast-math: they name the same
    primitives and meet the reference by the same rule, in every chunk size bit for bit the same among themselves"""
    b = beds(task)
    points = b.pool[2, :600]
    base = b.call(points, 0, N, _lib.RAY_SHARED)
    assert np.array_equal(base, b.call(np.tile(points, (N, 1, 1)), 0, N, 0))
    assert np.array_equal(base[:, :64], b.call(points[:64], 0, N, _lib.RAY_SHARED))
    assert np.array_equal(base[1:4], b.call(points, 1, 3, _lib.RAY_SHARED))
    monkeypatch.setenv("PIH_DIST_CULL", "0")
    plain = b.call(points, 0, N, _lib.RAY_SHARED)
    assert np.array_equal(plain[..., 1], base[..., 1])
    for e in range(N):
        b.check(e, points, "env", ALL, plain[e])
    for cull, want in (("0", plain), ("1", base)):
        monkeypatch.setenv("PIH_DIST_CULL", cull)
        for chunk in ("1", "2", "4"):
            monkeypatch.setenv("PIH_DIST_CHUNK", chunk)
            assert np.array_equal(want, b.call(points, 0, N, _lib.RAY_SHARED)), (cull, chunk)


@pytest.mark.parametrize("task", ("peg", "fly1"))
def test_bad_queries_are_isolated(beds, task):
    """queries with NaN / Inf / huge words or reach <= 0, among good ones: the miss record with words 0 and 2 .. 4 as given, in both
    frames; the good queries' records are what they are without the bad ones"""
    b = beds(task)
    q, bad = DC.bad_query_block()
    good = [r for r in range(len(q)) if r not in bad]
    out = b.call(q, 0, N, _lib.RAY_SHARED, _lib.GROUP_TABLE)
    for e in range(N):
        DC.check_bad_queries(out[e], q, bad)
    for flags in (_lib.RAY_SHARED, _lib.RAY_SHARED | _lib.RAY_FRAME_EE):
        out = b.call(q, 0, N, flags)
        for e in range(N):
            for r in bad:
                assert out[e, r, 1] == _lib.SEG_NONE and np.array_equal(out[e, r, [0, 2, 3, 4]], q[r, [3, 0, 1, 2]], equal_nan=True) and (out[e, r, 5:] == 0).all()
        assert np.array_equal(out[:, good], b.call(q[good], 0, N, flags))


@pytest.mark.parametrize("task", ("peg", "fly0"))
def test_argument_checks(beds, task):
    """every -2 that needs a handle, with the argument named, and the output untouched"""
    import torch
    b = beds(task); env = b.env; L = env.L
    points = torch.zeros(4 * 8 * 4 + 4, device=env.device); out = torch.full((4 * 8 * 8 + 4,), GUARD, device=env.device)
    p, o = points.data_ptr(), out.data_ptr()
    assert p % 16 == 0 and o % 16 == 0
    lacking = _lib.GROUP_FINGERS | _lib.GROUP_HOLE
    bad = [("out_dev", (None, p, 8, ALL, 0, 4, 0)), ("points_dev", (o, None, 8, ALL, 0, 4, 0)), ("points_per_env", (o, p, 0, ALL, 0, 4, 0)),
           ("points_per_env", (o, p, (1 << 20) + 1, ALL, 0, 4, 0)), ("env_begin / env_count", (o, p, 8, ALL, -1, 2, 0)), ("env_begin / env_count", (o, p, 8, ALL, 0, 0, 0)),
           ("env_begin / env_count", (o, p, 8, ALL, 2, 3, 0)), ("env_begin / env_count", (o, p, 8, ALL, 5, 1, 0)), ("groups", (o, p, 8, 0, 0, 4, 0)),
           ("groups", (o, p, 8, 32, 0, 4, 0)), ("groups", (o, p, 8, ALL | 64, 0, 4, 0)), ("groups", (o, p, 8, -1, 0, 4, 0)),
           ("flags", (o, p, 8, ALL, 0, 4, _lib.RAY_IGNORE_ROBOT)), ("flags", (o, p, 8, ALL, 0, 4, 8)), ("flags", (o, p, 8, ALL, 0, 4, -1)),
           ("out_dev", (o + 4, p, 8, ALL, 0, 4, 0)), ("points_dev", (o, p + 8, 8, ALL, 0, 4, 0))]
    if b.task == "fly":
        bad.append(("groups", (o, p, 8, lacking, 0, 4, 0)))
    for name, args in bad:
        with torch.cuda.device(env.device):
            assert L.pih_closest_points(env.h, *args, env._stream()) == -2, (name, args)
        assert L.pih_last_error(env.h).decode().startswith("pih_closest_points: " + name + " "), (name, L.pih_last_error(env.h))
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()), "a refused call wrote to its output"
    with torch.cuda.device(env.device):
        assert L.pih_closest_points(env.h, o, p, 8, lacking | _lib.GROUP_TABLE, 0, 4, 0, env._stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[:4 * 8 * 8] != GUARD).all()) and bool((out[4 * 8 * 8:] == GUARD).all())


@pytest.mark.parametrize("task", TASKS)
def test_cross_check_with_ray_test(beds, task):
    """pih_ray_test on the same handle, with and without the robot, against pih_closest_points with the matching groups: for every ray that
    hits, the distance at its origin is at most the way to the hit, fraction x length + G_GPU, and the hit position lies on a surface,
    |distance| <= 2 G_GPU.  The rays are the ray tests' aimed family, those whose origin lies outside every selected primitive by the
    reference (from inside a sphere or a capsule a ray does not hit it, and what it hits behind may lie inside)"""
    b = beds(task)
    robot = _lib.GROUP_ARM | _lib.GROUP_FINGERS
    hits_seen = 0
    for ignore, groups in ((False, ALL), (True, ALL & ~robot)):
        for e in range(N):
            rays = RY.aimed_rays(b.scene[e], 40 + e)
            o = rays[:, :3].astype(np.float64)
            outside = np.min([DC.signed_distance(b.scene[e], pr, o) for pr in DC.selected(b.scene[e], groups)], axis=0) > 1e-3
            rays = rays[outside]
            assert len(rays) > RY.N_AIMED // 2
            hits = b.env.ray_test(rays, frame="env", ignore_robot=ignore, env_begin=e, env_count=1).cpu().numpy()[0]
            hit = hits[:, 1] != _lib.SEG_NONE
            assert hit.sum() >= 100
            length = np.linalg.norm(rays[:, 3:].astype(np.float64) - rays[:, :3], axis=1)
            at_origin = b.call(np.concatenate([rays[:, :3], np.full((len(rays), 1), 10.0, np.float32)], 1), e, 1, _lib.RAY_SHARED, groups)[0]
            at_hit = b.call(np.concatenate([hits[:, 2:5], np.full((len(rays), 1), 10.0, np.float32)], 1), e, 1, _lib.RAY_SHARED, groups)[0]
            way = hits[:, 0].astype(np.float64) * length
            over, off = (at_origin[:, 0] - way)[hit].max(), np.abs(at_hit[hit, 0]).max()
            print("%s env %d ignore %d: %d hits, distance(origin) - way at most %.2e, |distance(hit position)| at most %.2e" % (task, e, ignore, hit.sum(), over, off))
            assert over <= DC.G_GPU and off <= 2 * DC.G_GPU, (e, ignore, over, off)
            hits_seen += int(hit.sum())
    assert hits_seen > 2000


def test_readme_example(beds, oracle_mod):
    """the usage example of README.md, run verbatim: the clearance of each env's peg tip to the hole is the reference's distance of that
    point to the tube"""
    import torch
    md = open(os.path.join(ROOT, "README.md")).read()
    code = re.search(r"```python\n(# signed clearance of each env's peg tip to the hole.*?)```", md, re.S).group(1)
    scope = {}
    exec(code, scope)
    env, rec, tip, clearance = scope["env"], scope["rec"], scope["tip"], scope["clearance"]
    torch.cuda.synchronize()
    assert tuple(rec.shape) == (env.n, 1, 8) and tuple(clearance.shape) == (env.n,) and tuple(tip.shape) == (env.n, 3)
    tube = [pr for pr in R.peg_scene(oracle_mod, env.state()[0].cpu().numpy()).prims if pr.kind == "tube"][0]
    want = DC.signed_distance(None, tube, tip.cpu().numpy().astype(np.float64))
    assert bool((rec[:, 0, 1] == _lib.VIEW_SEG_HOLE).all()) and np.abs(clearance.cpu().numpy() - want).max() <= DC.G_GPU
    assert np.abs(tip.cpu().numpy() - (rec[:, 0, 2:5] + rec[:, 0, :1] * rec[:, 0, 5:8]).cpu().numpy()).max() <= 2 * DC.G_GPU
    env.close()
