"""Time the batched robot-model queries (include/pih_robot.h) with HIP events on the launch stream -- measurement tool for DESIGN section 6.6.
Each of pih_robot_fk / jacobian / mass_matrix / inverse_dynamics at n = 4096, 16 384, 32 768 and 65 536 problems, both robots: forced to
each store variant through PIH_ROBOT_STORE (every lane stores its own rows | a wavefront's rows staged in LDS and stored as contiguous
256-byte runs; inverse dynamics has the direct one only) and as the library picks by n; and pih_link_states at 4096 envs of both tasks.  Per line: microseconds per call (median of REPEATS timed groups of CALLS back-to-back calls after a warm-up; the two store variants alternate),
problems per second, and the output bytes per second as a fraction of 8 TB/s.
usage (GPU box): python tools/robot_query_bench.py [--json FILE]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peg_in_hole_gym_amd import _lib  # noqa: E402
from peg_in_hole_gym_amd.vec_env import PihVecEnv  # noqa: E402

WARMUP, CALLS, REPEATS = 20, 50, 7
PEAK = 8e12
REST = {0: [0.0, -0.215, -1.0471975511965976, -2.57, 0.0, 2.356, 2.356, 0.02, 0.02], 1: [0.0, -1.5707963267948966, 1.5707963267948966, -1.5707963267948966, -1.5707963267948966, 0.0]}


def timed(f, variants=(None,), select=lambda v: None):
    """[median microseconds per call of each variant]: the variants alternate group by group, so that they see the same machine"""
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


def main():
    rows = []
    print("device:", torch.cuda.get_device_name(0))
    g = PihVecEnv(1)
    rng = np.random.default_rng(0)
    for robot, name in ((_lib.ROBOT_PANDA, "panda"), (_lib.ROBOT_UR5, "ur5")):
        nd, nf = _lib.robot_dims(robot)
        for n in (4096, 16384, 32768, 65536):
            q = torch.tensor(np.asarray(REST[robot]) + rng.uniform(-0.3, 0.3, (n, nd)) * ([1] * (7 if robot == 0 else 6) + [0.03] * (2 if robot == 0 else 0)), dtype=torch.float32, device="cuda")
            qd = torch.tensor(rng.uniform(-2, 2, (n, nd)), dtype=torch.float32, device="cuda")
            qdd = torch.tensor(rng.uniform(-2, 2, (n, nd)), dtype=torch.float32, device="cuda")
            outs = {"robot_fk": torch.empty(n, nf, 13, device="cuda"), "jacobian": torch.empty(n, 6, nd, device="cuda"),
                    "mass_matrix": torch.empty(n, nd, nd, device="cuda"), "inverse_dynamics": torch.empty(n, nd, device="cuda")}
            st = g._stream(); L, h = g.L, g.h
            calls = {"robot_fk": lambda: L.pih_robot_fk(h, robot, n, q.data_ptr(), qd.data_ptr(), outs["robot_fk"].data_ptr(), st),
                     "jacobian": lambda: L.pih_robot_jacobian(h, robot, n, q.data_ptr(), nf - 1, None, outs["jacobian"].data_ptr(), st),
                     "mass_matrix": lambda: L.pih_robot_mass_matrix(h, robot, n, q.data_ptr(), outs["mass_matrix"].data_ptr(), st),
                     "inverse_dynamics": lambda: L.pih_robot_inverse_dynamics(h, robot, n, q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), outs["inverse_dynamics"].data_ptr(), st)}
            for call, f in calls.items():
                def force(v):
                    if v is None:
                        os.environ.pop("PIH_ROBOT_STORE", None)
                    else:
                        os.environ["PIH_ROBOT_STORE"] = v
                variants = ("direct", None) if call == "inverse_dynamics" else ("direct", "staged", None)
                res = dict(zip(variants, timed(f, variants, force)))
                force(None)
                nbytes = outs[call].numel() * 4
                for v, us in res.items():
                    rows.append({"call": call, "robot": name, "n": n, "store": v or "library", "us": us, "problems_per_s": n / us * 1e6,
                                 "out_bytes_fraction_of_8TBps": nbytes / (us * 1e-6) / PEAK})
                us = res[None]
                print("%-16s %-5s n=%6d: direct %6.1f us, staged %s us, library %6.1f us = %.4f ms, %.3g problems/s, output %5.2f %% of 8 TB/s" % (
                    call, name, n, res["direct"], "%6.1f" % res["staged"] if "staged" in res else "   n/a", us, us * 1e-3, n / us * 1e6, 100 * nbytes / (us * 1e-6) / PEAK))
    g.close()
    for task, name in ((0, "peg-in-hole"), (1, "random-fly")):
        n = 4096
        kw = dict(task_id=1, max_episode_steps=480, contact_margin=0.02) if task else {}
        e = PihVecEnv(n, **kw); e.reset()
        out = torch.empty(n, _lib.link_states_frames(task), 13, device="cuda")
        us = timed(lambda: e.L.pih_link_states(e.h, out.data_ptr(), 0, n, e._stream()))[0]
        rows.append({"call": "link_states", "task": name, "n": n, "store": "direct", "us": us, "problems_per_s": n / us * 1e6,
                     "out_bytes_fraction_of_8TBps": out.numel() * 4 / (us * 1e-6) / PEAK})
        print("link_states      %-11s n=%6d: %8.1f us  (%.3g envs/s, output %.2f %% of 8 TB/s)" % (name, n, us, n / us * 1e6, 100 * out.numel() * 4 / (us * 1e-6) / PEAK))
        e.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
