"""TEST-ONLY backend: the fp64 oracle behind the same surface as PihVecEnv, so the host-side façade and the sharding
logic can be tested in this GPU-less container.  Never imported by the product."""
import numpy as np

from oracle import oracle as O
from peg_in_hole_gym_amd import _lib


class OracleBackend:
    def __init__(self, n, offsets=None, mode=0, seed=0, env_index0=0, auto_reset=0, device=None, task_id=0, **cfg):
        kw = dict(mode=mode, seed=seed, env_index0=env_index0, auto_reset=auto_reset)
        kw.update(cfg)
        self.n = n
        self.task_id = task_id
        self.adim = 6 if task_id == 1 else 4
        self.offsets = np.zeros((n, 3)) if offsets is None else np.asarray(offsets, dtype=float).reshape(n, 3)
        self.o = (O.FlyOracle if task_id == 1 else O.Oracle)(n, offsets=self.offsets, **kw)
        self._obs = None

    def reset(self, mask=None, hard_reset=False):
        self.o.reset(None if mask is None else np.asarray(mask), hard_reset=hard_reset)

    def reseed(self, seed):
        self.o.reseed(seed)

    def invalid(self):
        return self.o.get_state()[:, _lib.F_INVALID if self.task_id == 1 else _lib.S_INVALID] != 0

    def step(self, actions):
        a = np.asarray(actions, dtype=np.float64).reshape(self.n, self.adim)
        obs, rew, done = self.o.step(a)
        self._obs = obs
        return obs.astype(np.float32), rew.astype(np.float32), done

    def step_n(self, k, actions=None):
        a = np.zeros((self.n, 4)) if actions is None else np.asarray(actions, dtype=np.float64).reshape(self.n, 4)
        out = None
        for _ in range(k):
            out = self.o.step(a)
        return out[0].astype(np.float32), out[1].astype(np.float32), out[2]

    def state(self):
        if self.task_id == 1:
            return self.o.get_state()
        s = np.zeros((self.n, 256))
        s[:, :O.STATE_WORDS] = self.o.get_state()
        return s

    def ee_position(self):
        st = self.o.get_state()
        return np.array([O.fk_arm(st[i, _lib.S_QARM : _lib.S_QDARM], 9)[0] + self.offsets[i] for i in range(self.n)])

    def tip_pose(self):
        return self.o.tip_pose()

    def contact_force(self):
        return self.o.contact_force()

    def render(self, width=300, height=300, shaded=False):
        return self.o.render(width, height, shaded=shaded)

    def grasp_labels(self, size=300):
        ang = self.o.get_state()[:, _lib.S_GRASP_ANGLE]
        outs = [O.grasp_labels(a, size) for a in ang]
        return np.stack([x[0] for x in outs]), np.stack([x[1] for x in outs])

    def close(self):
        pass


def factory(n, offsets, **cfg):
    return OracleBackend(n, offsets, **cfg)


class RecordingBackend:
    """a backend that computes nothing: it records the keywords the task classes forward to render, render_view and link_states"""

    def __init__(self, n, offsets, **cfg):
        self.n, self.cfg, self.calls = n, cfg, []

    def reset(self, mask=None, hard_reset=False):
        pass

    def render(self, width=300, height=300, **kw):
        self.calls.append(dict(width=width, height=height, **kw))
        return np.full((self.n, height, width, 4), 7.0, dtype=np.float32)

    def render_view(self, **kw):
        self.calls.append(kw)
        return "image"

    def link_states(self, **kw):
        self.calls.append(kw)
        return "states"
