"""Diagnostic: largest contact normal force per step in scripted mode, row-space vs DOF-space solver.  usage: python tools/force_trace.py [n]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from peg_in_hole_gym_amd import _lib
from peg_in_hole_gym_amd.vec_env import PihVecEnv
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
for path in (0, 1):
    env = PihVecEnv(n, mode=1, dv=0.05, auto_reset=1, max_episode_steps=2227, seed=5, solver_path=path)
    big = []
    tot = torch.zeros((), dtype=torch.float64, device="cuda")
    for t in range(2300):
        env.step(None)
        st = env.state()
        f = st[:, _lib.S_CFORCE].abs()
        tot += f.double().sum()
        m, i = f.max(0)
        if float(m) > 1e5:
            big.append((t, float(m), int(i), int(st[i, _lib.S_NCONTACT]), int(st[i, _lib.S_SOLVER]), 0.0))
    print("solver_path %d: mean force %.1f; steps with a force > 1e5 N: %d" % (path, float(tot) / (2300 * n), len(big)))
    for b in big[:25]:
        print("   step %d force %.3g env %d contacts %d solver %d" % b[:5])
