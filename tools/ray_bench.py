"""Time the batched ray tests (pih_ray_test, include/pih_robot.h) with HIP events on the launch stream -- measurement tool for DESIGN
section 6.7.  4096 envs x 16, 64 and 1024 rays per env, both tasks, shared rays (one set for all envs) and per-env rays: the kernels with
and without the bounding-sphere rejection (PIH_RAY_CULL, alternating group by group so that they see the same machine), and for 1024 rays
every chunk size (PIH_RAY_CHUNK = 1, 2, 4 passes of 256 rays per workgroup) beside the library's choice.  Per line: microseconds per call
(median of REPEATS timed groups of CALLS back-to-back calls after a warm-up), rays per second, the output bytes per second as a fraction
of 8 TB/s.  Beside them, from the same run, two yardsticks: pih_link_states of the same 4096 envs (the same per-env set-up: what a
16-ray call cannot be faster than by much) and the depth-only camera at 32 x 32 (as many rays as 1024 per env, with a pinhole pattern
and tile culling: what culling is worth).
Rays: 16 and 64 are a ray_fan on the hand in the end-effector frame, robot ignored (the proximity-ring case); 1024 are segments between
random points of the workspace in the env-local frame (the incoherent case).
usage (GPU box): python tools/ray_bench.py [--json FILE]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peg_in_hole_gym_amd import _lib  # noqa: E402
from peg_in_hole_gym_amd.vec_env import PihVecEnv  # noqa: E402

WARMUP, CALLS, REPEATS = 10, 20, 7
PEAK = 8e12
N = 4096
C_FLOATS = ctypes.c_float * _lib.CAM_WORDS


def timed(f, variants, select):
    """[median microseconds per call of each variant]: the variants alternate group by group"""
    for v in variants:
        select(v)
        for _ in range(WARMUP):
            assert f() == 0
    torch.cuda.synchronize()
    us = {v: [] for v in variants}
    for _ in range(REPEATS):
        for v in variants:
            select(v)
            a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                f()
            b.record(); torch.cuda.synchronize()
            us[v].append(a.elapsed_time(b) / CALLS * 1e3)
    return [float(np.median(us[v])) for v in variants]


def switches(v):
    """v = (cull, chunk): "0" | "1" | None, "1" | "2" | "4" | None (None: the library's choice)"""
    for name, val in zip(("PIH_RAY_CULL", "PIH_RAY_CHUNK"), v):
        if val is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = val


def main():
    rows = []
    print("device:", torch.cuda.get_device_name(0))
    gen = torch.Generator(device="cuda"); gen.manual_seed(0)
    lo = torch.tensor([-0.6, -0.9, 0.0], device="cuda"); hi = torch.tensor([0.9, 0.3, 1.0], device="cuda")
    for task, name in ((0, "peg-in-hole"), (1, "random-fly")):
        kw = dict(task_id=1, max_episode_steps=480, contact_margin=0.02) if task else {}
        e = PihVecEnv(N, **kw); e.reset()
        st = e._stream()
        axis = (0.0, 0.0, 1.0) if task == 0 else (1.0, 0.0, 0.0)
        for R in (16, 64, 1024):
            if R < 1024:
                shared = e.ray_fan(tuple(0.02 * a for a in axis), axis, 60.0, 3, (R - 1) // 3, 0.5)
                flags = _lib.RAY_FRAME_EE | _lib.RAY_IGNORE_ROBOT
            else:
                pts = lo + (hi - lo) * torch.rand(2, R, 3, device="cuda", generator=gen)
                pts[1, :, 2] = pts[1, :, 2] * 0.6 - 0.1
                shared = torch.cat([pts[0], pts[1]], dim=1).contiguous()
                flags = 0
            R = shared.shape[0]
            per_env = (shared[None] + 1e-3 * torch.rand(N, R, 6, device="cuda", generator=gen)).contiguous()
            out = torch.empty(N, R, _lib.RAY_HIT_WORDS, device="cuda")
            for kind, rays, fl in (("shared", shared, flags | _lib.RAY_SHARED), ("per-env", per_env, flags)):
                variants = [("1", None), ("0", None)] + ([("1", c) for c in ("1", "2", "4")] if R > 256 else [])
                res = dict(zip(variants, timed(lambda: e.L.pih_ray_test(e.h, out.data_ptr(), rays.data_ptr(), R, 0, N, fl, st), variants, switches)))
                switches((None, None))
                hit = float((out[..., 1] != _lib.SEG_NONE).float().mean())
                for (cull, chunk), us in res.items():
                    rows.append({"call": "ray_test", "task": name, "envs": N, "rays_per_env": R, "rays": kind, "cull": int(cull), "chunk": chunk or "library", "us": us,
                                 "rays_per_s": N * R / us * 1e6, "out_bytes_fraction_of_8TBps": out.numel() * 4 / (us * 1e-6) / PEAK, "hit_share": hit})
                us = res[("1", None)]
                print("ray_test %-11s %4d rays %-7s: %8.1f us with the sphere rejection, %8.1f us without%s  (%.3g rays/s, output %5.2f %% of 8 TB/s, %.0f %% hit)" % (
                    name, R, kind, us, res[("0", None)], "".join(", chunk %s: %.1f us" % (c, res[("1", c)]) for c in ("1", "2", "4") if ("1", c) in res),
                    N * R / us * 1e6, 100 * out.numel() * 4 / (us * 1e-6) / PEAK, 100 * hit))
        # the yardsticks, from the same handle in the same run
        ls = torch.empty(N, _lib.link_states_frames(task), _lib.LINK_STATE_WORDS, device="cuda")
        us = timed(lambda: e.L.pih_link_states(e.h, ls.data_ptr(), 0, N, st), (None,), lambda v: None)[0]
        rows.append({"call": "link_states", "task": name, "envs": N, "us": us})
        print("link_states %-11s %d envs: %8.1f us" % (name, N, us))
        depth = torch.empty(N, 32, 32, device="cuda")
        if task == 0:
            cam = (C_FLOATS)(*_lib.VIEW_CAM_OVERVIEW)
            f = lambda: e.L.pih_render_view(e.h, depth.data_ptr(), cam, 32, 32, 0, N, _lib.RENDER_OUT_DEPTH, st)      # noqa: E731
        else:
            cam = (C_FLOATS)(*_lib.FLY_CAM_DEFAULT)
            f = lambda: e.L.pih_render_cam(e.h, depth.data_ptr(), cam, 32, 32, 0, N, _lib.RENDER_OUT_DEPTH, st)      # noqa: E731
        us = timed(f, (None,), lambda v: None)[0]
        rows.append({"call": "depth camera 32x32", "task": name, "envs": N, "us": us, "rays_per_s": N * 1024 / us * 1e6})
        print("depth camera 32 x 32 %-11s %d envs: %8.1f us  (%.3g pixels/s)" % (name, N, us, N * 1024 / us * 1e6))
        e.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
