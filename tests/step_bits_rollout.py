"""The rollouts behind tests/test_gpu_step_bits.py and tests/golden/make_step_bits_golden.py: 256 envs at the library defaults (residual
threshold 1e-7, warm start 0.85, exit test in iterations 1..4, 20, 36, 50), random actions from a fixed seed,

  reset      steps 1 .. 40 from reset: the pipes fall freely and the exit test ends 7.6 % of the solves early;
  prerolled  steps 301 .. 340 of the same run: contact steady state (mean 7.3 contacts, up to 25), every row-space solver variant.

Recorded per step: PIH_S_PGS_ITERS, PIH_S_SOLVER, PIH_S_NCONTACT, reward and done of every env; every eighth step the observations; after
the last step of each part the state words below the end of the warm-start cache."""
import numpy as np

from peg_in_hole_gym_amd import _lib

N, STEPS, PREROLL, SEED = 256, 40, 300, 11
WORDS = _lib.S_CACHE_LAMBDA + 48
OBS_EVERY = 8
ARRAYS = ("iters", "solver", "ncontact", "reward", "done", "obs", "state")


def rollout(torch, env):
    """env: a PihVecEnv of N envs fresh from its constructor -> {part_name: array}"""
    rng = np.random.default_rng(SEED)
    out = {}

    def part(name):
        it = np.zeros((STEPS, N), np.uint8); var = np.zeros((STEPS, N), np.uint8); nc = np.zeros((STEPS, N), np.uint8)
        rew = np.zeros((STEPS, N), np.float32); done = np.zeros((STEPS, N), np.uint8); obs = []
        for t in range(STEPS):
            o, r, d = env.step(torch.tensor(rng.uniform(-1, 1, (N, 4)), dtype=torch.float32))
            s = env.state().cpu().numpy()
            it[t] = s[:, _lib.S_PGS_ITERS]; var[t] = s[:, _lib.S_SOLVER]; nc[t] = s[:, _lib.S_NCONTACT]
            rew[t] = r.cpu().numpy(); done[t] = d.cpu().numpy()
            if t % OBS_EVERY == OBS_EVERY - 1:
                obs.append(o.cpu().numpy().astype(np.float32))
        out.update({name + "_iters": it, name + "_solver": var, name + "_ncontact": nc, name + "_reward": rew, name + "_done": done,
                    name + "_obs": np.array(obs), name + "_state": s[:, :WORDS].astype(np.float32)})
    part("reset")
    for t in range(PREROLL - STEPS):
        env.step(torch.tensor(rng.uniform(-1, 1, (N, 4)), dtype=torch.float32))
    part("prerolled")
    return out
