"""Time the batched closest-point queries (pih_closest_points, include/pih_robot.h) with HIP events on the launch stream -- measurement
tool for DESIGN section 6.8, modelled on tools/ray_bench.py.  4096 envs x 16, 64 and 1024 queries per env, both tasks, shared queries (one
set for all envs) and per-env queries: the library's choice of kernel and the kernels with and without the bounding-sphere rejection
(PIH_DIST_CULL, alternating group by group so that they see the same machine), and for 1024 queries every chunk size
(PIH_DIST_CHUNK = 1, 2, 4 passes of 256 queries per workgroup, without the rejection) beside the library's choice.  Beside every line, from the same run and alternating with it, pih_ray_test at the same env and
ray counts with the library's defaults: the same per-env set-up, the same bytes out, 24 instead of 16 bytes in.
Queries and rays: 16 and 64 are the far ends of a ray_fan on the hand, 10 cm long, in the end-effector frame, measured against everything
but the robot (the rays: that fan, robot ignored); 1024 are random points of the workspace in the env-local frame against all groups (the
rays: segments from those points to other random points).  reach = 10 m: every query has an answer, and the rejection starts with
nothing to reject.
Per line: microseconds per call (median of REPEATS timed groups of CALLS back-to-back calls after a warm-up), queries per second, the
output bytes per second as a fraction of 8 TB/s.
usage (GPU box): python tools/dist_bench.py [--json FILE]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peg_in_hole_gym_amd import _lib  # noqa: E402
from peg_in_hole_gym_amd.vec_env import PihVecEnv  # noqa: E402
from ray_bench import N, PEAK, timed  # noqa: E402

REACH = 10.0
NO_ROBOT = _lib.GROUP_ALL & ~(_lib.GROUP_ARM | _lib.GROUP_FINGERS)


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
        for P in (16, 64, 1024):
            if P < 1024:
                rays = e.ray_fan(tuple(0.02 * a for a in axis), axis, 60.0, 3, (P - 1) // 3, 0.1)
                flags, ray_flags, groups = _lib.RAY_FRAME_EE, _lib.RAY_FRAME_EE | _lib.RAY_IGNORE_ROBOT, NO_ROBOT
            else:
                pts = lo + (hi - lo) * torch.rand(2, P, 3, device="cuda", generator=gen)
                pts[1, :, 2] = pts[1, :, 2] * 0.6 - 0.1
                rays = torch.cat([pts[0], pts[1]], dim=1).contiguous()
                flags, ray_flags, groups = 0, 0, _lib.GROUP_ALL
            P = rays.shape[0]
            points = torch.cat([rays[:, 3:] if P < 1024 else rays[:, :3], torch.full((P, 1), REACH, device="cuda")], dim=1).contiguous()
            per_env = {"points": (points[None] + 1e-3 * torch.rand(N, P, 4, device="cuda", generator=gen)).contiguous(),
                       "rays": (rays[None] + 1e-3 * torch.rand(N, P, 6, device="cuda", generator=gen)).contiguous()}
            out = torch.empty(N, P, _lib.CLOSEST_WORDS, device="cuda")
            for kind, q, r, sh in (("shared", points, rays, _lib.RAY_SHARED), ("per-env", per_env["points"], per_env["rays"], 0)):
                variants = [(None, None), ("1", None), ("0", None), "ray_test"] + ([("0", c) for c in ("1", "2", "4")] if P > 256 else [])
                which = {"v": None}

                def select(v):
                    which["v"] = v
                    for var, val in zip(("PIH_DIST_CULL", "PIH_DIST_CHUNK"), (None, None) if v == "ray_test" else v):
                        if val is None:
                            os.environ.pop(var, None)
                        else:
                            os.environ[var] = val

                def call():
                    if which["v"] == "ray_test":
                        return e.L.pih_ray_test(e.h, out.data_ptr(), r.data_ptr(), P, 0, N, ray_flags | sh, st)
                    return e.L.pih_closest_points(e.h, out.data_ptr(), q.data_ptr(), P, groups, 0, N, flags | sh, st)

                res = dict(zip(variants, timed(call, variants, select)))
                select((None, None))
                assert call() == 0
                torch.cuda.synchronize()
                select((None, None))
                hit = float((out[..., 1] != _lib.SEG_NONE).float().mean()); inside = float((out[..., 0] < 0).float().mean())
                for v, us in res.items():
                    row = {"task": name, "envs": N, "per_env": P, "kind": kind, "us": us, "per_s": N * P / us * 1e6, "out_bytes_fraction_of_8TBps": out.numel() * 4 / (us * 1e-6) / PEAK}
                    rows.append(dict(row, call="ray_test") if v == "ray_test" else dict(row, call="closest_points", cull="library" if v[0] is None else int(v[0]), chunk=v[1] or "library", hit_share=hit, inside_share=inside))
                us = res[(None, None)]
                print("closest_points %-11s %4d queries %-7s: %8.1f us (the library's choice), %8.1f us with the sphere rejection, %8.1f us without%s; ray_test %8.1f us (x %.2f)  (%.3g queries/s, output %5.2f %% of 8 TB/s, %.0f %% answered, %.0f %% inside)" % (
                    name, P, kind, us, res[("1", None)], res[("0", None)], "".join(", chunk %s: %.1f us" % (c, res[("0", c)]) for c in ("1", "2", "4") if ("0", c) in res),
                    res["ray_test"], us / res["ray_test"], N * P / us * 1e6, 100 * out.numel() * 4 / (us * 1e-6) / PEAK, 100 * hit, 100 * inside))
        e.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
