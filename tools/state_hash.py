"""Bit-level fingerprint of the product's trajectories: sha256 of the state tensors after seeded rollouts (action mode 4096 envs x 500
steps, scripted mode 1024 x 900, random-fly 4096 x 300).  Two builds whose kernels perform the same arithmetic in the same order print
the same lines -- the check used when an optimisation only re-schedules instructions.  usage: python tools/state_hash.py"""
import sys, os, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from peg_in_hole_gym_amd import _lib
from peg_in_hole_gym_amd.vec_env import PihVecEnv


def run(name, n, steps, adim, **kw):
    env = PihVecEnv(n, auto_reset=1, seed=7, **kw)
    gen = torch.Generator(device="cuda").manual_seed(99)
    h = hashlib.sha256(); variants = torch.zeros(6, dtype=torch.long)
    for t in range(steps):
        obs, rew, done = env.step(torch.rand(n, adim, device="cuda", generator=gen) * 2 - 1)
        if t % 50 == 49:
            st = env.state()
            h.update(st.cpu().numpy().tobytes()); h.update(obs.cpu().numpy().tobytes())
            if adim == 4:
                variants += torch.bincount(st[:, _lib.S_SOLVER].long().cpu(), minlength=6)
    print("%-28s %s  solver variants %s" % (name, h.hexdigest()[:32], variants.tolist()))


run("peg-in-hole action", 4096, 500, 4)
run("peg-in-hole action stride 1", 1024, 300, 4, exit_check_stride=1)
run("peg-in-hole scripted", 1024, 900, 4, mode=1, dv=0.05)
run("peg-in-hole DOF space", 512, 300, 4, solver_path=1)
run("random-fly Banana", 4096, 300, 6, task_id=1, dt=1 / 120.)
