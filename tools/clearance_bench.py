"""Time the robot clearance queries (pih_robot_clearance, include/pih_robot.h) with HIP events on the launch stream -- measurement tool for
DESIGN section 6.9, modelled on tools/dist_bench.py.  4096 envs x 1 (q = NULL: the current state), 16, 64 and 256 configurations per env, both
tasks, shared q (one set for all envs) and per-env q, object + table, reach 0.2 m.  Per line, alternating group by group so that all
see the same machine:
  the library's choice of kernel instance; the four instances -- with / without the bounding-sphere rejection (PIH_CLEAR_CULL), one
  configuration or one (configuration, probe) pair per lane (PIH_CLEAR_SPLIT); for 256 configurations every chunk size
  (PIH_CLEAR_CHUNK = 1, 2, 4 passes of 256 work items per workgroup) of the library's instance
and two baselines from the same run:
  points       pih_closest_points at C x NP queries per env against the same groups: the same per-env set-up, two thirds of the output
               bytes, a point where the clearance call has a capsule
  composition  what a caller had to do before: pih_robot_fk of all configurations, 8 sample points per link capsule gathered with torch
               (the frame origins stand in for the capsule ends and the hand spheres), pih_closest_points on them
Configurations: the envs' current joint values + N(0, 0.3) per joint.
Per line: microseconds per call (median of REPEATS timed groups of CALLS back-to-back calls after a warm-up), configurations per second,
the output bytes per second as a fraction of 8 TB/s, the share of records with an answer and of overlapping ones.
usage (GPU box): python tools/clearance_bench.py [--json FILE]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peg_in_hole_gym_amd import _lib  # noqa: E402
from peg_in_hole_gym_amd.vec_env import PihVecEnv  # noqa: E402
from ray_bench import N, PEAK, timed  # noqa: E402

REACH = 0.2
GROUPS = _lib.GROUP_OBJECT | _lib.GROUP_TABLE
SAMPLES = 8
SWITCHES = ("PIH_CLEAR_CULL", "PIH_CLEAR_SPLIT", "PIH_CLEAR_CHUNK")


def main():
    rows = []
    print("device:", torch.cuda.get_device_name(0))
    gen = torch.Generator(device="cuda"); gen.manual_seed(0)
    for task, name in ((0, "peg-in-hole"), (1, "random-fly")):
        kw = dict(task_id=1, max_episode_steps=480, contact_margin=0.02) if task else {}
        e = PihVecEnv(N, **kw); e.reset()
        st = e._stream()
        robot = _lib.ROBOT_UR5 if task else _lib.ROBOT_PANDA
        nd, nf = _lib.robot_dims(robot)
        NP = _lib.clearance_probes(task)
        word0 = _lib.F_Q if task else _lib.S_QARM
        own = e.state()[:, word0:word0 + nd].contiguous()
        t = torch.linspace(0.0, 1.0, SAMPLES, device="cuda")[None, None, :, None]
        for C in (1, 16, 64, 256):
            per_env = (own[:, None, :] + (0.3 * torch.randn(N, C, nd, device="cuda", generator=gen) if C > 1 else 0.0)).contiguous()
            out = torch.empty(N, C, NP, _lib.CLEAR_WORDS, device="cuda")
            pts_out = torch.empty(N, C * NP, _lib.CLOSEST_WORDS, device="cuda")
            for kind, q, sh in (("current", None, 0),) if C == 1 else (("shared", per_env[0].contiguous(), _lib.RAY_SHARED), ("per-env", per_env, 0)):
                qq = per_env if q is None else q
                # the baselines' inputs: the points of the composition, and NP of them per configuration for the plain point call
                fk = e.robot_fk(qq.reshape(-1, nd))[:, :, :3]
                ends = torch.cat([torch.zeros_like(fk[:, :1]), fk], dim=1)[:, :NP + 1] if task == 0 else fk
                mid = 0.5 * (ends[:, :-1] + ends[:, 1:])
                few = torch.cat([mid[:, torch.arange(NP, device="cuda") % mid.shape[1]], torch.full((fk.shape[0], NP, 1), REACH, device="cuda")], dim=-1)
                few = few.reshape((C * NP, 4) if sh else (N, C * NP, 4)).contiguous()
                comp_out = torch.empty(N, C * (ends.shape[1] - 1) * SAMPLES, _lib.CLOSEST_WORDS, device="cuda")
                variants = [None, ("1", "0", None), ("0", "0", None), ("1", "1", None), ("0", "1", None), "points", "composition"]
                if C == 256:
                    variants += [(None, None, c) for c in ("1", "2", "4")]
                which = {"v": None}

                def select(v):
                    which["v"] = v
                    for var, val in zip(SWITCHES, v if isinstance(v, tuple) else (None, None, None)):
                        if val is None:
                            os.environ.pop(var, None)
                        else:
                            os.environ[var] = val

                def call():
                    v = which["v"]
                    if v == "points":
                        return e.L.pih_closest_points(e.h, pts_out.data_ptr(), few.data_ptr(), C * NP, GROUPS, 0, N, sh, st)
                    if v == "composition":
                        f = e.robot_fk(qq.reshape(-1, nd))[:, :, :3]
                        en = torch.cat([torch.zeros_like(f[:, :1]), f], dim=1)[:, :NP + 1] if task == 0 else f
                        p = (en[:, :-1, None, :] + t * (en[:, 1:, None, :] - en[:, :-1, None, :])).reshape((-1, 3) if sh else (N, -1, 3))
                        e.closest_points(p, reach=REACH, groups=GROUPS, out=comp_out if not sh else None)
                        return 0
                    return e.L.pih_robot_clearance(e.h, out.data_ptr(), None if q is None else q.data_ptr(), C, REACH, GROUPS, 0, N, sh, st)

                res = dict(zip(variants, timed(call, variants, select)))
                select(None)
                assert call() == 0
                torch.cuda.synchronize()
                hit = float((out[..., 1] != _lib.SEG_NONE).float().mean()); inside = float((out[..., 0] < 0).float().mean())
                for v, us in res.items():
                    row = {"task": name, "envs": N, "configs": C, "kind": kind, "us": us, "configs_per_s": N * C / us * 1e6}
                    if isinstance(v, str):
                        rows.append(dict(row, call=v))
                    else:
                        rows.append(dict(row, call="robot_clearance", cull="library" if v is None or v[0] is None else int(v[0]), split="library" if v is None or v[1] is None else int(v[1]),
                                         chunk="library" if v is None or v[2] is None else int(v[2]), out_bytes_fraction_of_8TBps=out.numel() * 4 / (us * 1e-6) / PEAK, hit_share=hit, inside_share=inside))
                us = res[None]
                print("robot_clearance %-11s %3d configs %-7s: %8.1f us (the library's choice); per configuration cull %8.1f / plain %8.1f us; per probe cull %8.1f / plain %8.1f us%s; "
                      "points %8.1f us (x %.2f), composition %8.1f us (x %.2f)  (%.3g configs/s, output %5.2f %% of 8 TB/s, %.0f %% answered, %.0f %% overlapping)" % (
                          name, C, kind, us, res[("1", "0", None)], res[("0", "0", None)], res[("1", "1", None)], res[("0", "1", None)],
                          "".join("; chunk %s: %.1f us" % (c, res[(None, None, c)]) for c in ("1", "2", "4") if (None, None, c) in res),
                          res["points"], res["points"] / us, res["composition"], res["composition"] / us, N * C / us * 1e6, 100 * out.numel() * 4 / (us * 1e-6) / PEAK, 100 * hit, 100 * inside))
        e.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
