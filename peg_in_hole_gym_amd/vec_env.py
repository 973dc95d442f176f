"""Tensor-level vectorised environment: thin host wrapper over the C ABI (include/pih.h).

All data stay on the GPU as PyTorch-ROCm tensors; PyTorch is only the owner of device memory and of the stream."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def tracking_cameras(opos, eye, up=(0.0, 0.0, 1.0), fov=60.0, aspect=1.0, near=0.01, far=100.0):
    """Cameras that follow a point per env: opos float [n, 3] (any device) -> float32 [n, 13] on the same device, row e = (eye, target =
    opos[e], up, fov, aspect, near, far) in the camera words of pih_render_cam.  eye and up: 3 numbers for all envs, or [n, 3].  Pure
    torch: with PihVecEnv.render(camera=...) the viewpoint moves with the simulation without leaving the device."""
    opos = torch.as_tensor(opos).to(torch.float32)
    if opos.ndim != 2 or opos.shape[1] != 3:
        raise ValueError("tracking_cameras: opos must have shape [n, 3], got %s" % (tuple(opos.shape),))
    n = opos.shape[0]
    cam = torch.empty(n, _lib.CAM_WORDS, dtype=torch.float32, device=opos.device)
    cam[:, 0:3] = torch.as_tensor(eye, dtype=torch.float32, device=opos.device)
    cam[:, 3:6] = opos
    cam[:, 6:9] = torch.as_tensor(up, dtype=torch.float32, device=opos.device)
    cam[:, 9] = float(fov); cam[:, 10] = float(aspect); cam[:, 11] = float(near); cam[:, 12] = float(far)
    return cam


def random_lights(n, device, generator=None, elevation=(20.0, 80.0)):
    """float32 [n, 11] on `device`: _lib.LIGHT_DEFAULT with a unit direction of uniformly drawn azimuth and elevation (degrees) per row.  Pure
    torch on the device."""
    lo, hi = float(elevation[0]), float(elevation[1])
    if not (-90.0 <= lo <= hi <= 90.0):
        raise ValueError("random_lights: elevation must be a range within [-90, 90] degrees, got %r" % (elevation,))
    u = torch.rand(n, 2, device=device, generator=generator, dtype=torch.float32)
    az = u[:, 0] * (2.0 * np.pi); el = torch.deg2rad(lo + (hi - lo) * u[:, 1])
    light = torch.tensor(_lib.LIGHT_DEFAULT, dtype=torch.float32, device=device).repeat(n, 1)
    light[:, 0] = torch.cos(el) * torch.cos(az); light[:, 1] = torch.cos(el) * torch.sin(az); light[:, 2] = torch.sin(el)
    return light


def ray_fan(origin, axis, half_angle_deg, rings, per_ring, length, device=None):
    """A cone of rays for PihVecEnv.ray_test, the proximity-sensor pattern: float32 [1 + rings * per_ring, 6] rows (from, to).  Every ray
    starts at `origin` and is `length` long; ray 0 runs along `axis`, ring k = 1 .. rings holds per_ring rays at the angle
    half_angle_deg * k / rings from the axis, equally spaced around it (ring k turned by half a spacing against ring k - 1).  origin and
    axis: 3 numbers or tensors (axis need not be unit).  Pure torch on `device` (default: origin's, if it is a tensor): no host round
    trip."""
    if rings < 0 or per_ring < 1 or not (0.0 <= float(half_angle_deg) < 180.0):
        raise ValueError("ray_fan: rings >= 0, per_ring >= 1 and 0 <= half_angle_deg < 180, got %r, %r, %r" % (rings, per_ring, half_angle_deg))
    if device is None:
        device = origin.device if torch.is_tensor(origin) else "cpu"
    o = torch.as_tensor(origin, dtype=torch.float32).to(device).reshape(3)
    a = torch.as_tensor(axis, dtype=torch.float32).to(device).reshape(3)
    a = a / torch.linalg.norm(a)
    # a unit vector across the axis: from the coordinate axis the cone's axis is furthest from
    helper = torch.where(a[0].abs() < 0.9, torch.tensor([1.0, 0.0, 0.0], device=device), torch.tensor([0.0, 1.0, 0.0], device=device))
    u = torch.linalg.cross(a, helper); u = u / torch.linalg.norm(u)
    v = torch.linalg.cross(a, u)
    k = torch.arange(1, rings + 1, dtype=torch.float32, device=device).repeat_interleave(per_ring)
    j = torch.arange(per_ring, dtype=torch.float32, device=device).repeat(rings)
    polar = torch.cat([torch.zeros(1, device=device), torch.deg2rad(torch.as_tensor(float(half_angle_deg), device=device)) * k / max(rings, 1)])
    azim = torch.cat([torch.zeros(1, device=device), (j + 0.5 * k) * (2.0 * np.pi / per_ring)])
    d = torch.cos(polar)[:, None] * a + torch.sin(polar)[:, None] * (torch.cos(azim)[:, None] * u + torch.sin(azim)[:, None] * v)
    return torch.cat([o.expand(len(d), 3), o + float(length) * d], dim=1).contiguous()


class PihVecEnv:
    """N independent worlds of one task on one MI355X.

    task_id 0 ('peg-in-hole', default): Panda + pipe + hole, one wavefront per world;
        step(actions[N,4]) -> obs[N,5] (finger1, finger2, ee xyz; envs/peg_in_hole.py:13), reward[N], done[N]
    task_id 1 ('random-fly'): UR5 + one free-flying object, one LANE per world;
        step(actions[N,6] = ee target xyz + euler rpy, envs/utils.py:70-72) -> obs[N,6] (ee xyz, object xyz), reward[N], done[N]
    mirrors BaseEnv.step (envs/base_env.py:60-75) for every agent at once; see include/pih.h for what each call replaces.
    """

    def __init__(self, n_envs, device="cuda:0", offsets=None, **cfg):
        if not torch.cuda.is_available():
            raise _lib.PihError("no ROCm device visible: peg_in_hole_gym_amd has no CPU path")
        self.L = _lib.load()
        self.n = int(n_envs)
        self.device = torch.device(device)
        self.cfg = _lib.default_config(n_envs=self.n, **cfg)
        self.task_id = int(self.cfg.task_id)
        self.action_dim, self.obs_dim, self.state_words = _lib.task_dims(self.task_id)
        self._invalid_word = _lib.F_INVALID if self.task_id == _lib.TASK_RANDOM_FLY else _lib.S_INVALID
        off = None
        if offsets is not None:
            off = np.ascontiguousarray(np.asarray(offsets, dtype=np.float32).reshape(self.n, 3))
        self.h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.L.pih_create(C.byref(self.cfg), off.ctypes.data if off is not None else None, C.byref(self.h))
        if rc != 0:
            raise _lib.PihError("pih_create failed (%d): %s" % (rc, self.L.pih_last_error(None).decode()))
        self.obs = torch.zeros(self.n, self.obs_dim, device=self.device)
        self.reward = torch.zeros(self.n, device=self.device)
        self.done = torch.zeros(self.n, dtype=torch.uint8, device=self.device)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.pih_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _chk(self, rc, what):
        if rc != 0:
            raise _lib.PihError("%s failed (%d): %s" % (what, rc, self.L.pih_last_error(self.h).decode()))

    def reset(self, mask=None, hard_reset=False, seed=0):
        """pih_reset: every reset (soft or hard) draws a NEW scene from the env's own sequence, as the reference does with the global
        `random` (envs/peg_in_hole.py:239-267); hard_reset (resetSimulation, envs/base_env.py:85-86) also clears the non-finite-reset
        count.  seed != 0: explicit replay -- new base seed, the reset envs restart their draw sequence from its beginning."""
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_reset(self.h, m.data_ptr() if m is not None else None, int(bool(hard_reset)), int(seed), self._stream()), "pih_reset")

    def reseed(self, seed):
        """New base seed (env seed = seed + 1000 + global env index); the envs reset by the NEXT reset() restart their draw sequence."""
        self._chk(self.L.pih_reseed(self.h, int(seed)), "pih_reseed")

    def invalid(self):
        """uint8-like [n]: envs whose state became non-finite with auto_reset = 0 (re-initialised, done, frozen until reset)."""
        return self.state()[:, self._invalid_word] != 0

    def step(self, actions, obs_out=None):
        """obs_out: optional float32 [n, obs_dim] device tensor to receive the observation instead of self.obs (a caller that hands the
        observation to an asynchronous consumer -- bench.py's overlapped all-gather -- alternates between two of them)"""
        a = None
        if actions is not None:
            a = actions.to(device=self.device, dtype=torch.float32).contiguous()
            assert a.shape == (self.n, self.action_dim), a.shape
        obs = self.obs if obs_out is None else obs_out
        if obs_out is not None:
            assert obs.shape == self.obs.shape and obs.dtype == torch.float32 and obs.is_contiguous() and obs.device == self.obs.device
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_step(self.h, a.data_ptr() if a is not None else None, obs.data_ptr(), self.reward.data_ptr(),
                                      self.done.data_ptr(), self._stream()), "pih_step")
        return obs, self.reward, self.done

    def step_n(self, k, actions=None):
        a = None
        if actions is not None:
            a = actions.to(device=self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_step_n(self.h, int(k), a.data_ptr() if a is not None else None, self.obs.data_ptr(),
                                        self.reward.data_ptr(), self.done.data_ptr(), self._stream()), "pih_step_n")
        return self.obs, self.reward, self.done

    def _get(self, field, shape):
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_get_state(self.h, field, out.data_ptr(), self._stream()), "pih_get_state")
        return out

    def state(self):
        return self._get(_lib.FIELD_STATE, (self.n, self.state_words))

    def set_state(self, s):
        s = s.to(device=self.device, dtype=torch.float32).contiguous()
        assert s.shape == (self.n, self.state_words)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_set_state(self.h, _lib.FIELD_STATE, s.data_ptr(), self._stream()), "pih_set_state")

    # --- checkpoint / resume: everything a handle owns is its per-env state record -- the 98 physical words incl. the
    # RNG draw counters and step counters, the derived outputs, the warm-start contact cache -- plus the base seed; the config rides
    # along so that a checkpoint is only loaded into a handle that simulates the same thing.
    # Every field of pih_config has to agree but these: `schedule` and `debug` do not change what is simulated (schedule + 64 selects another rounding of the same PGS solve), `seed` is checked on its own,
    # `reserved_f` is unused.  (A new field is compared unless it is excluded here.)
    _CFG_KEYS = tuple(f for f, _ in _lib.PihConfig._fields_ if f not in ("schedule", "debug", "seed", "reserved_f"))

    def state_dict(self):
        """-> {'state': float32 [n, state_words] (host copy), 'seed': int, 'config': {...}, 'abi_version': int}"""
        torch.cuda.synchronize(self.device)
        return {"state": self.state().cpu(), "seed": int(self.cfg.seed), "abi_version": int(self.L.pih_abi_version()),
                "config": {k: (float(getattr(self.cfg, k)) if isinstance(getattr(self.cfg, k), float) else int(getattr(self.cfg, k))) for k in self._CFG_KEYS}}

    def load_state_dict(self, sd, strict=True):
        """Resume: after this call the handle continues bit for bit like the one that produced `sd` (same later draws: the RNG counters
        are part of the record; the base seed must be the handle's).  strict: refuse a checkpoint of another config."""
        if int(sd["abi_version"]) != int(self.L.pih_abi_version()):
            raise _lib.PihError("checkpoint written by ABI v%d, this library is v%d" % (sd["abi_version"], self.L.pih_abi_version()))
        mine = self.state_dict()["config"]
        diff = {k: (v, mine[k]) for k, v in sd["config"].items() if k in mine and (abs(v - mine[k]) > 1e-9 * max(1.0, abs(v)))}
        if strict and diff:
            raise _lib.PihError("checkpoint / handle config mismatch: %s" % diff)
        st = sd["state"]
        if tuple(st.shape) != (self.n, self.state_words):
            raise _lib.PihError("checkpoint state has shape %s, this handle %s" % (tuple(st.shape), (self.n, self.state_words)))
        if int(sd["seed"]) != int(self.cfg.seed):       # (the base seed is fixed at creation: later auto-resets would draw other scenes)
            raise _lib.PihError("checkpoint seed %d != handle seed %d: create the handle with seed=%d or use PihVecEnv.from_state_dict" % (sd["seed"], self.cfg.seed, sd["seed"]))
        self.set_state(st)

    @classmethod
    def from_state_dict(cls, sd, device="cuda:0", offsets=None):
        """A new handle with the checkpoint's config and seed, resumed from its state (offsets live in the state record)."""
        cfg = dict(sd["config"]); n = int(cfg.pop("n_envs"))
        env = cls(n, device=device, offsets=offsets, seed=int(sd["seed"]), **cfg)
        env.load_state_dict(sd)
        return env

    def ee_position(self):
        """World position of the grasp-target frame (pybullet link 11) after the last step / reset."""
        return self._get(_lib.FIELD_EE_POS, (self.n, 3))

    def tip_pose(self):
        return self._get(_lib.FIELD_TIP_POSE, (self.n, 7))

    def contact_force(self):
        return self._get(_lib.FIELD_CONTACT_FORCE, (self.n,))

    def debug(self):
        return self._get(_lib.FIELD_DEBUG, (self.n, _lib.DEBUG_WORDS))

    def ik(self, q0, tpos, tquat):
        q0 = q0.to(device=self.device, dtype=torch.float32).contiguous()
        tpos = tpos.to(device=self.device, dtype=torch.float32).contiguous()
        tquat = tquat.to(device=self.device, dtype=torch.float32).contiguous()
        n = q0.shape[0]
        out = torch.empty(n, 9, device=self.device)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_ik(self.h, n, q0.data_ptr(), tpos.data_ptr(), tquat.data_ptr(), out.data_ptr(), self._stream()), "pih_ik")
        return out

    def ik_ur5(self, q0, tpos, tquat):
        """Batched calculateInverseKinematics for the UR5 chain (ur_execute, envs/utils.py:79): q0 [n,6] -> q* [n,6]."""
        q0 = q0.to(device=self.device, dtype=torch.float32).contiguous()
        tpos = tpos.to(device=self.device, dtype=torch.float32).contiguous()
        tquat = tquat.to(device=self.device, dtype=torch.float32).contiguous()
        n = q0.shape[0]
        out = torch.empty(n, 6, device=self.device)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_ik_ur5(self.h, n, q0.data_ptr(), tpos.data_ptr(), tquat.data_ptr(), out.data_ptr(), self._stream()), "pih_ik_ur5")
        return out

    # --- batched robot-model queries (include/pih_robot.h): what a controller or a reward asks pybullet per env -- getLinkStates,
    # calculateJacobian, calculateMassMatrix, calculateInverseDynamics -- for n problems at once on the device.  n is independent of the
    # handle's env count; robot = _lib.ROBOT_PANDA / _lib.ROBOT_UR5, None = the robot of the handle's task.  Inputs of any float dtype /
    # device are brought to float32 on the handle's device, as ik() does; nothing synchronises.
    def _robot(self, robot):
        if robot is None:
            robot = _lib.ROBOT_UR5 if self.task_id == _lib.TASK_RANDOM_FLY else _lib.ROBOT_PANDA
        ndof, nframes = _lib.robot_dims(robot)         # (PihError for an unknown robot)
        return int(robot), ndof, nframes

    def _rows(self, what, t, n, width):
        t = torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous()
        if t.ndim != 2 or t.shape[1] != width or (n is not None and t.shape[0] != n):
            raise ValueError("%s must have shape [%s, %d], got %s" % (what, "n" if n is None else n, width, tuple(t.shape)))
        return t

    def robot_fk(self, q, qd=None, robot=None):
        """getLinkStates(computeLinkVelocity=1): q [n, ndof] (qd [n, ndof] or None: zero velocities) -> float32 [n, nframes, 13] = pos,
        quat xyzw, linear velocity of the frame origin, angular velocity of every URDF link frame (Panda: 0..8 links, 9 grasp-target;
        UR5: 0..5 links, 6 ee_link), robot-base-local like ik()'s targets (no env offset)."""
        robot, ndof, nframes = self._robot(robot)
        q = self._rows("robot_fk: q", q, None, ndof); n = q.shape[0]
        qd = None if qd is None else self._rows("robot_fk: qd", qd, n, ndof)
        out = torch.empty(n, nframes, _lib.LINK_STATE_WORDS, device=self.device)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_robot_fk(self.h, robot, n, q.data_ptr(), qd.data_ptr() if qd is not None else None, out.data_ptr(), self._stream()), "pih_robot_fk")
        return out

    def jacobian(self, q, frame=None, local_pos=None, robot=None):
        """calculateJacobian: float32 [n, 6, ndof], rows 0..2 linear and 3..5 angular, for the point local_pos ([n, 3] in the frame's
        coordinates; None = its origin) of frame `frame` (None = the end-effector frame)."""
        robot, ndof, nframes = self._robot(robot)
        q = self._rows("jacobian: q", q, None, ndof); n = q.shape[0]
        lp = None if local_pos is None else self._rows("jacobian: local_pos", local_pos, n, 3)
        out = torch.empty(n, 6, ndof, device=self.device)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_robot_jacobian(self.h, robot, n, q.data_ptr(), nframes - 1 if frame is None else int(frame),
                                                lp.data_ptr() if lp is not None else None, out.data_ptr(), self._stream()), "pih_robot_jacobian")
        return out

    def mass_matrix(self, q, robot=None):
        """calculateMassMatrix: float32 [n, ndof, ndof], bitwise symmetric (Panda: 9 x 9 with the two finger DOF)."""
        robot, ndof, _ = self._robot(robot)
        q = self._rows("mass_matrix: q", q, None, ndof); n = q.shape[0]
        out = torch.empty(n, ndof, ndof, device=self.device)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_robot_mass_matrix(self.h, robot, n, q.data_ptr(), out.data_ptr(), self._stream()), "pih_robot_mass_matrix")
        return out

    def inverse_dynamics(self, q, qd, qdd, robot=None):
        """float32 [n, ndof]: tau = M(q) qdd + Coriolis + gravity + the step's damping -- the inverse of the step's FREE dynamics.
        pybullet's calculateInverseDynamics has no damping: include/pih_robot.h says how to take it out."""
        robot, ndof, _ = self._robot(robot)
        q = self._rows("inverse_dynamics: q", q, None, ndof); n = q.shape[0]
        qd = self._rows("inverse_dynamics: qd", qd, n, ndof); qdd = self._rows("inverse_dynamics: qdd", qdd, n, ndof)
        out = torch.empty(n, ndof, device=self.device)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_robot_inverse_dynamics(self.h, robot, n, q.data_ptr(), qd.data_ptr(), qdd.data_ptr(), out.data_ptr(), self._stream()), "pih_robot_inverse_dynamics")
        return out

    def link_states(self, env_begin=0, env_count=None, out=None):
        """Every frame of the envs' CURRENT state in world coordinates (env offset added): float32 [count, frames, 13].  peg-in-hole: the
        10 Panda frames, then the 24 pipe links (34); random-fly: the 7 UR5 frames, then the object (8)."""
        count = self.n - env_begin if env_count is None else env_count
        shape = (count, _lib.link_states_frames(self.task_id), _lib.LINK_STATE_WORDS)
        if out is None:
            out = torch.empty(shape, device=self.device)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape and self._here(out) and out.is_contiguous()):
            raise ValueError("link_states: out must be a contiguous float32 tensor of shape %s on %s" % (shape, self.device))
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_link_states(self.h, out.data_ptr(), int(env_begin), int(count), self._stream()), "pih_link_states")
        return out

    _RAY_FRAME = {"env": 0, "ee": _lib.RAY_FRAME_EE}

    def ray_test(self, rays, frame="env", ignore_robot=False, env_begin=0, env_count=None, out=None):
        """rayTestBatch against the scene the task's free camera draws, at the envs' CURRENT state (pih_ray_test, include/pih_robot.h):
        peg-in-hole arm, hand, finger pads, pipe, hole and table; random-fly UR5, object and table.
        rays: [R, 6] = (from xyz, to xyz), the same rays for every env of the call, or [count, R, 6], one set per env (row e: env
            env_begin + e).  A float32 tensor on this handle's device is used in place, anything else is converted and moved there.
        frame: "env" = the env-local frame (the env offset does not enter); "ee" = the end-effector frame of each env (peg-in-hole: the
            grasp-target frame; random-fly: ee_link) -- parentObjectUniqueId / parentLinkIndex of rayTestBatch.
        ignore_robot: the arm is transparent (a sensor mounted on the hand looks out through it).
        -> float32 [count, R, 8] on the device: hit fraction in (0, 1] (1 = no hit), what was hit (the seg values of render_view /
        render's "rgba8" format as floats, _lib.SEG_NONE for nothing), hit position xyz and outward unit normal xyz, both env-local.
        No hit: position = the ray's end, normal 0.  A ray with a NaN / Inf word or of zero length reports no hit; the others of the call
        are not affected.  out: a contiguous float32 tensor of that shape on this handle's device (ValueError otherwise)."""
        count = self.n - env_begin if env_count is None else env_count
        if frame not in self._RAY_FRAME:
            raise ValueError("ray_test: frame must be one of %s, got %r" % (sorted(self._RAY_FRAME), frame))
        rays = torch.as_tensor(rays).to(device=self.device, dtype=torch.float32).contiguous()
        if rays.ndim not in (2, 3) or rays.shape[-1] != _lib.RAY_WORDS or rays.shape[-2] < 1 or (rays.ndim == 3 and rays.shape[0] != count):
            raise ValueError("ray_test: rays must have shape [R, %d] (shared) or [%d, R, %d] (one set per env of the call) with R >= 1, got %s"
                             % (_lib.RAY_WORDS, count, _lib.RAY_WORDS, tuple(rays.shape)))
        if rays.data_ptr() % 16:
            rays = rays.clone()                # (a view into a larger tensor: the kernel loads aligned pairs of words)
        R = rays.shape[-2]
        shape = (count, R, _lib.RAY_HIT_WORDS)
        if out is None:
            out = torch.empty(shape, device=self.device)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape and self._here(out) and out.is_contiguous()):
            raise ValueError("ray_test: out must be a contiguous float32 tensor of shape %s on %s" % (shape, self.device))
        flags = self._RAY_FRAME[frame] | (_lib.RAY_SHARED if rays.ndim == 2 else 0) | (_lib.RAY_IGNORE_ROBOT if ignore_robot else 0)
        self._rays_keep = rays                 # (a converted copy lives until the next call: the launch is asynchronous)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_ray_test(self.h, out.data_ptr(), rays.data_ptr(), int(R), int(env_begin), int(count), flags, self._stream()), "pih_ray_test")
        return out

    def closest_points(self, points, reach=None, frame="env", groups=("arm", "fingers", "object", "hole", "table"), env_begin=0, env_count=None, out=None):
        """getClosestPoints of points against the scene of ray_test, at the envs' CURRENT state (pih_closest_points, include/pih_robot.h).
        points: [P, 3 | 4] = x, y, z (and reach), the same queries for every env of the call, or [count, P, 3 | 4], one set per env.  A
            3-column tensor takes the scalar `reach` for every query (required then; with 4 columns `reach` must be None).  reach [m] is
            the `distance` argument of getClosestPoints: only what is nearer is reported.
        frame: "env" | "ee", as for ray_test.
        groups: what the points are measured against: names of _lib.GROUPS ("arm", "fingers", "object", "hole", "table") or a mask of
            _lib.GROUP_*.  A group the task does not have selects nothing; a mask that selects nothing at all is an error.
        -> float32 [count, P, 8] on the device: signed distance (negative inside a primitive), what is nearest (the seg values of
        ray_test as floats), the closest point on its surface xyz and the outward unit normal there xyz, both env-local: point = closest
        point + distance x normal.  Nothing within reach: reach, _lib.SEG_NONE, the query point, normal 0.  A query with a NaN / Inf word
        or reach <= 0 reports that too; the others of the call are not affected.  out: a contiguous float32 tensor of that shape on this
        handle's device (ValueError otherwise)."""
        count = self.n - env_begin if env_count is None else env_count
        if frame not in self._RAY_FRAME:
            raise ValueError("closest_points: frame must be one of %s, got %r" % (sorted(self._RAY_FRAME), frame))
        if isinstance(groups, str):
            groups = (groups,)
        if not isinstance(groups, int):
            unknown = [g for g in groups if g not in _lib.GROUPS]
            if unknown:
                raise ValueError("closest_points: groups must be names of %s, got %r" % (sorted(_lib.GROUPS), unknown))
            mask = 0
            for g in groups:
                mask |= _lib.GROUPS[g]
            groups = mask
        points = torch.as_tensor(points).to(device=self.device, dtype=torch.float32)
        if points.ndim not in (2, 3) or points.shape[-1] not in (3, _lib.POINT_WORDS) or points.shape[-2] < 1 or (points.ndim == 3 and points.shape[0] != count):
            raise ValueError("closest_points: points must have shape [P, 3 | 4] (shared) or [%d, P, 3 | 4] (one set per env of the call) with P >= 1, got %s"
                             % (count, tuple(points.shape)))
        if (points.shape[-1] == 3) != (reach is not None):
            raise ValueError("closest_points: give `reach` with 3-column points and only then (a fourth column is the reach of each query)")
        if reach is not None:
            points = torch.cat([points, torch.full(points.shape[:-1] + (1,), float(reach), device=self.device)], dim=-1)
        points = points.contiguous()
        if points.data_ptr() % 16:
            points = points.clone()            # (a view into a larger tensor: the kernel loads a query as one aligned 16-byte word)
        P = points.shape[-2]
        shape = (count, P, _lib.CLOSEST_WORDS)
        if out is None:
            out = torch.empty(shape, device=self.device)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape and self._here(out) and out.is_contiguous()):
            raise ValueError("closest_points: out must be a contiguous float32 tensor of shape %s on %s" % (shape, self.device))
        flags = self._RAY_FRAME[frame] | (_lib.RAY_SHARED if points.ndim == 2 else 0)
        self._points_keep = points             # (a converted copy lives until the next call: the launch is asynchronous)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_closest_points(self.h, out.data_ptr(), points.data_ptr(), int(P), int(groups), int(env_begin), int(count), flags, self._stream()),
                      "pih_closest_points")
        return out

    def robot_clearance(self, q=None, reach=1.0, groups=("object", "table"), env_begin=0, env_count=None, out=None):
        """getClosestPoints(robot, body, distance, linkIndexA) for every link of the task's robot placed at joint values q, against the
        pipe / the flying object and the table at the envs' CURRENT state (pih_robot_clearance, include/pih_robot.h).
        q: [C, ndof], the same C configurations for every env of the call, or [count, C, ndof], one set per env; ndof = 9 (Panda: the two
            finger words move no probe) or 6 (UR5).  None: every env at its own current joint state (C = 1).
        reach [m] > 0: only what is nearer is reported.
        groups: "object" and / or "table" (names of _lib.GROUPS or a mask of _lib.GROUP_*).  The hole, the fingers and the arm itself are
            not measured: any other group is an error, as is a mask that selects nothing.
        -> float32 [count, C, NP, 12] on the device, NP = 11 probes (Panda: the capsules of links 0 .. 6, the four hand spheres) or 6 (UR5),
        per probe: signed distance of the two surfaces (negative = overlap), the nearest obstacle's seg value, the closest point on the
        probe xyz, the closest point on the obstacle xyz, the unit normal on the obstacle towards the probe xyz (point on probe = point on
        obstacle + distance x normal), the probe's own seg (its link).  Nothing within reach: reach, _lib.SEG_NONE, the probe's first axis
        end point twice, normal 0.  A configuration with a NaN / Inf word reports that with the points 0 for all its probes; the others of
        the call are not affected.  out: a contiguous float32 tensor of that shape on this handle's device (ValueError otherwise)."""
        count = self.n - env_begin if env_count is None else env_count
        if isinstance(groups, str):
            groups = (groups,)
        if not isinstance(groups, int):
            unknown = [g for g in groups if g not in _lib.GROUPS]
            if unknown:
                raise ValueError("robot_clearance: groups must be names of %s, got %r" % (sorted(_lib.GROUPS), unknown))
            mask = 0
            for g in groups:
                mask |= _lib.GROUPS[g]
            groups = mask
        fly = self.task_id == _lib.TASK_RANDOM_FLY
        ndof = _lib.robot_dims(_lib.ROBOT_UR5 if fly else _lib.ROBOT_PANDA)[0]
        if q is not None:
            q = torch.as_tensor(q).to(device=self.device, dtype=torch.float32)
            if q.ndim not in (2, 3) or q.shape[-1] != ndof or q.shape[-2] < 1 or (q.ndim == 3 and q.shape[0] != count):
                raise ValueError("robot_clearance: q must have shape [C, %d] (shared) or [%d, C, %d] (one set per env of the call) with C >= 1, got %s"
                                 % (ndof, count, ndof, tuple(q.shape)))
            q = q.contiguous()
        Cn = 1 if q is None else q.shape[-2]
        shape = (count, Cn, _lib.clearance_probes(self.task_id), _lib.CLEAR_WORDS)
        if out is None:
            out = torch.empty(shape, device=self.device)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape and self._here(out) and out.is_contiguous()):
            raise ValueError("robot_clearance: out must be a contiguous float32 tensor of shape %s on %s" % (shape, self.device))
        flags = _lib.RAY_SHARED if q is not None and q.ndim == 2 else 0
        self._clear_keep = q                   # (a converted copy lives until the next call: the launch is asynchronous)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_robot_clearance(self.h, out.data_ptr(), None if q is None else q.data_ptr(), int(Cn), float(reach), int(groups),
                                                 int(env_begin), int(count), flags, self._stream()), "pih_robot_clearance")
        return out

    def ray_fan(self, origin, axis, half_angle_deg, rings, per_ring, length):
        """float32 [1 + rings * per_ring, 6] device tensor: a cone of rays from `origin` about `axis` (module function ray_fan), for
        ray_test -- with frame="ee" a proximity sensor that rides on the hand.  Built on the device, no host round trip."""
        return ray_fan(origin, axis, half_angle_deg, rings, per_ring, length, device=self.device)

    def _here(self, t):
        """is the tensor on this handle's device? (a handle made with device="cuda" has no index)"""
        return t.device.type == self.device.type and (self.device.index is None or t.device.index == self.device.index)

    _RENDER_FMT = {"float4": (0, torch.float32, (4,)), "rgba8": (_lib.RENDER_OUT_RGBA8, torch.uint8, (4,)), "depth": (_lib.RENDER_OUT_DEPTH, torch.float32, ())}

    def _camera_arg(self, what, camera, count):
        """camera argument of render / render_view -> (ctypes argument, flag): None -> (None, 0); 13 numbers -> a host array; [count, 13] -> the
        device address of a float32 tensor on this handle's device (used in place, or converted and uploaded) with RENDER_CAM_DEVICE"""
        if camera is None:
            return None, 0
        if (camera.ndim if hasattr(camera, "ndim") else np.ndim(camera)) >= 2:
            if not (torch.is_tensor(camera) and camera.dtype == torch.float32 and self._here(camera) and camera.is_contiguous()):
                camera = torch.as_tensor(np.asarray(camera.cpu() if torch.is_tensor(camera) else camera, dtype=np.float32)).to(self.device).contiguous()
            if tuple(camera.shape) != (count, _lib.CAM_WORDS):
                raise ValueError("%s: per-env cameras must have shape [%d, %d] (one row per env of the call), got %s" % (what, count, _lib.CAM_WORDS, tuple(camera.shape)))
            self._cam_keep = camera          # (the uploaded copy lives until the next call: the launch is asynchronous)
            return C.c_void_p(camera.data_ptr()), _lib.RENDER_CAM_DEVICE
        vals = [float(x) for x in camera]
        if len(vals) != _lib.CAM_WORDS:
            raise ValueError("%s: camera must have %d numbers (eye, target, up, fov, aspect, near, far), got %d" % (what, _lib.CAM_WORDS, len(vals)))
        return (C.c_float * _lib.CAM_WORDS)(*vals), 0

    def _light_arg(self, what, light, count):
        """light argument of render / render_view (never None) -> (ctypes argument, flag): "default" -> (None, 0) = _lib.LIGHT_DEFAULT;
        11 numbers -> a host array; [count, 11] -> the device address of a float32 tensor on this handle's device (used in place, or
        converted and moved there; never read back) with RENDER_LIGHT_DEVICE"""
        if isinstance(light, str):
            if light != "default":
                raise ValueError("%s: light must be None, \"default\", %d numbers or a [count, %d] array, got %r" % (what, _lib.LIGHT_WORDS, _lib.LIGHT_WORDS, light))
            return None, 0
        if (light.ndim if hasattr(light, "ndim") else np.ndim(light)) >= 2:
            if torch.is_tensor(light):
                light = light.to(device=self.device, dtype=torch.float32).contiguous()
            else:
                light = torch.as_tensor(np.asarray(light, dtype=np.float32)).to(self.device).contiguous()
            if tuple(light.shape) != (count, _lib.LIGHT_WORDS):
                raise ValueError("%s: per-env lights must have shape [%d, %d] (one row per env of the call), got %s" % (what, count, _lib.LIGHT_WORDS, tuple(light.shape)))
            self._light_keep = light         # (lives until the next call: the launch is asynchronous)
            return C.c_void_p(light.data_ptr()), _lib.RENDER_LIGHT_DEVICE
        vals = [float(x) for x in light]
        if len(vals) != _lib.LIGHT_WORDS:
            raise ValueError("%s: light must have %d numbers (direction xyz, colour rgb, ambient, diffuse, specular, shininess, shadow factor), got %d" % (what, _lib.LIGHT_WORDS, len(vals)))
        return (C.c_float * _lib.LIGHT_WORDS)(*vals), 0

    def _out_arg(self, what, out, fmt, count, height, width):
        """output tensor of render / render_view for format `fmt` -> (tensor, format flag)"""
        fmt_flag, dtype, tail = self._RENDER_FMT[fmt]
        shape = (count, height, width) + tail
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        elif fmt != "float4" and not (torch.is_tensor(out) and out.dtype == dtype and tuple(out.shape) == shape and self._here(out) and out.is_contiguous()):
            raise ValueError("%s: out must be a contiguous %s tensor of shape %s on %s for fmt=%r" % (what, dtype, shape, self.device, fmt))
        return out, fmt_flag

    def render(self, width=300, height=300, env_begin=0, env_count=None, out=None, shaded=False, camera=None, ee_frame=False, fmt="float4", light=None):
        """Camera image of a block of envs at the current state (analytic ray caster): float32 [count, height, width, 4] =
        (depth buffer, r, g, b), RGB on the 0..255 scale, flat per object or (shaded=True) times ambient + diffuse of TinyRenderer's
        default light.
        peg-in-hole: PegInHole.render (envs/peg_in_hole.py:276-304), the wrist camera (pih_render_ex); the camera and the format are
            fixed, so `camera` / `ee_frame` / a `fmt` other than "float4" raise ValueError.
        random-fly: a free camera over the UR5's capsules, the object and the table (pih_render_cam).  camera = 13 numbers (eye xyz,
            target xyz, up xyz, vertical fov in degrees, aspect, near, far: the arguments of computeViewMatrix and
            computeProjectionMatrixFOV) or None = _lib.FLY_CAM_DEFAULT, one camera for all envs of the call, in each env's local frame
            (the env offset does not enter); ee_frame=True: in the ee_link frame of each env's UR5 (eye-in-hand).
            camera of shape [count, 13]: one camera per env of the call (row e: env env_begin + e), read by the kernel from device memory
            -- a float32 tensor on this handle's device is used in place, anything else is converted and uploaded.  These cameras are
            not validated on the host: an env whose row is degenerate gets the background image (a 1-D camera raises PihError).
            fmt: what getCameraImage returns, in two calls --
              "float4"  float32 [count, height, width, 4]   (depth buffer, r, g, b)
              "rgba8"   uint8   [count, height, width, 4]   (r, g, b, seg): the colours rounded half up to bytes; seg = link index 0..5,
                                                            _lib.SEG_OBJECT, _lib.SEG_TABLE or _lib.SEG_NONE
              "depth"   float32 [count, height, width]      the depth buffer alone
            out: for "rgba8" / "depth" it must be a contiguous tensor of that dtype and shape on this handle's device (ValueError).
            light: None = the calls above.  Anything else draws the image under a caller-given light, with a specular term and cast
            shadows (pih_render_lit, include/pih_render_light.h states the model; always shaded): "default" = _lib.LIGHT_DEFAULT; 11 numbers
            (direction towards the light in the env-local frame, colour rgb, ambient, diffuse, specular, shininess, shadow factor: 1 = no
            shadows), one light for all envs; shape [count, 11]: one light per env of the call in device memory (random_lights()), tested by
            the kernel: an env whose row is degenerate gets the background.  Fewer or more than 11 numbers: ValueError."""
        count = self.n - env_begin if env_count is None else env_count
        fly = self.task_id == _lib.TASK_RANDOM_FLY
        if light is not None and not fly:
            raise ValueError("render: the peg-in-hole wrist camera of render() takes no light; render_view(light=...) does (camera=None is the same camera)")
        if not fly and (camera is not None or ee_frame):
            raise ValueError("render: the peg-in-hole task has a fixed wrist camera; camera / ee_frame belong to the random-fly task")
        if fmt not in self._RENDER_FMT:
            raise ValueError("render: fmt must be one of %s, got %r" % (sorted(self._RENDER_FMT), fmt))
        if not fly and fmt != "float4":
            raise ValueError("render: the peg-in-hole wrist camera has the one format 'float4'; 'rgba8' / 'depth' belong to the random-fly task")
        cam, cam_flag = self._camera_arg("render", camera, count)
        out, fmt_flag = self._out_arg("render", out, fmt, count, height, width)
        if light is not None:
            lgt, light_flag = self._light_arg("render", light, count)
            flags = _lib.RENDER_SHADED | (_lib.RENDER_CAM_EE if ee_frame else 0) | fmt_flag | cam_flag | light_flag
            with torch.cuda.device(self.device):
                self._chk(self.L.pih_render_lit(self.h, out.data_ptr(), cam, lgt, width, height, env_begin, count, flags, self._stream()), "pih_render_lit")
            return out
        with torch.cuda.device(self.device):
            if fly:
                flags = (_lib.RENDER_SHADED if shaded else 0) | (_lib.RENDER_CAM_EE if ee_frame else 0) | fmt_flag | cam_flag
                self._chk(self.L.pih_render_cam(self.h, out.data_ptr(), cam, width, height, env_begin, count, flags, self._stream()), "pih_render_cam")
            else:
                self._chk(self.L.pih_render_ex(self.h, out.data_ptr(), width, height, env_begin, count, 1 if shaded else 0, self._stream()), "pih_render_ex")
        return out

    _VIEW_FRAME = {"env": 0, "ee": _lib.RENDER_CAM_EE, "ee_pos": _lib.RENDER_CAM_EE_POS}

    def render_view(self, width=300, height=300, env_begin=0, env_count=None, out=None, shaded=False, camera=None, frame="env", fmt="float4", light=None):
        """peg-in-hole from any viewpoint (pih_render_view): the scene of render() -- table, pipe, hole, finger pads -- plus a stand-in
        arm (one capsule per link, the hand's spheres), at the current state; nothing of the state changes.
        camera = 13 numbers as in render() of the random-fly task, one camera for all envs of the call; None = the wrist preset
            (_lib.VIEW_CAM_WRIST in the "ee_pos" frame: the camera of render(), whatever `frame` says); _lib.VIEW_CAM_OVERVIEW shows the
            whole arm from the side.  camera of shape [count, 13]: one camera per env of the call, read by the kernel from device memory
            (a float32 tensor on this handle's device is used in place); such cameras are not validated on the host: an env whose row
            is degenerate gets the background image.  Following each env's peg tip without a host round trip:
                render_view(camera=tracking_cameras(env.tip_pose()[:, :3], eye))
        frame: "env" = the env-local frame; "ee" = the grasp-target frame (pybullet link 11): the camera turns with the hand;
            "ee_pos" = eye and target offset by the grasp-target's position, axes env-local: it follows the hand and does not turn.
        fmt: "float4" float32 [count, height, width, 4] (depth buffer, r, g, b); "rgba8" uint8 [count, height, width, 4] (r, g, b, seg),
            seg = arm link 0..6 (the hand is 6), fingers 7 and 8, _lib.VIEW_SEG_HOLE, _lib.VIEW_SEG_TABLE, _lib.VIEW_SEG_PIPE0 + pipe
            capsule 0..23, _lib.SEG_NONE; "depth" float32 [count, height, width].  out: as in render().
        light: as in render(): None = pih_render_view; "default", 11 numbers or [count, 11] = the image under that light, with a specular
            term and the shadows of arm, hand, pipe and hole (pih_render_lit; always shaded)."""
        count = self.n - env_begin if env_count is None else env_count
        if self.task_id != _lib.TASK_PEG_IN_HOLE:
            raise ValueError("render_view: this camera belongs to the peg-in-hole task (random-fly: render(camera=...))")
        if fmt not in self._RENDER_FMT:
            raise ValueError("render_view: fmt must be one of %s, got %r" % (sorted(self._RENDER_FMT), fmt))
        if frame not in self._VIEW_FRAME:
            raise ValueError("render_view: frame must be one of %s, got %r" % (sorted(self._VIEW_FRAME), frame))
        cam, cam_flag = self._camera_arg("render_view", camera, count)
        out, fmt_flag = self._out_arg("render_view", out, fmt, count, height, width)
        flags = (_lib.RENDER_SHADED if shaded else 0) | self._VIEW_FRAME[frame] | fmt_flag | cam_flag
        if light is not None:
            lgt, light_flag = self._light_arg("render_view", light, count)
            with torch.cuda.device(self.device):
                self._chk(self.L.pih_render_lit(self.h, out.data_ptr(), cam, lgt, width, height, env_begin, count, flags | _lib.RENDER_SHADED | light_flag, self._stream()), "pih_render_lit")
            return out
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_render_view(self.h, out.data_ptr(), cam, width, height, env_begin, count, flags, self._stream()), "pih_render_view")
        return out

    def tracking_cameras(self, eye, up=(0.0, 0.0, 1.0), fov=60.0, aspect=1.0, near=0.01, far=100.0):
        """random-fly: float32 [n, 13] device tensor, one camera per env that looks from `eye` (env-local frame) at the env's object (the
        PIH_F_OPOS words of the device state, no host synchronisation) -- feed it to render(camera=...)."""
        if self.task_id != _lib.TASK_RANDOM_FLY:
            raise ValueError("tracking_cameras: the object to follow belongs to the random-fly task")
        return tracking_cameras(self.state()[:, _lib.F_OPOS:_lib.F_OPOS + 3], eye, up, fov, aspect, near, far)

    def random_lights(self, generator=None, elevation=(20.0, 80.0)):
        """float32 [n, 11] device tensor of _lib.LIGHT_DEFAULT lights whose direction is drawn per env: azimuth uniform in [0, 360), elevation
        uniform in `elevation` (degrees above the table).  Built on the device, no host round trip -- feed it to render(light=...) /
        render_view(light=...); the companion of tracking_cameras.  generator: a torch.Generator on this handle's device, or None."""
        return random_lights(self.n, self.device, generator, elevation)

    def grasp_labels(self, size=300, env_begin=0, env_count=None):
        """Label images + [x, y, angle_deg, width, length] of random_grasp (envs/peg_in_hole.py:72-99,116):
        (float32 [count, 4, size, size] = pos, sin, cos, wid ; float32 [count, 5])."""
        count = self.n - env_begin if env_count is None else env_count
        out = torch.empty(count, 4, size, size, device=self.device)
        meta = torch.empty(count, 5, device=self.device)
        with torch.cuda.device(self.device):
            self._chk(self.L.pih_grasp_labels(self.h, out.data_ptr(), meta.data_ptr(), size, env_begin, count, self._stream()), "pih_grasp_labels")
        return out, meta

    def set_timing(self, enable):
        self.L.pih_set_timing(self.h, int(enable))

    def timing(self, reset=True):
        """(average ms per step = the two numbers of timing2 added, number of timed steps)"""
        ms = C.c_double(0)
        n = C.c_int64(0)
        self._chk(self.L.pih_timing(self.h, int(reset), C.byref(ms), C.byref(n)), "pih_timing")
        return ms.value, n.value

    def timing2(self, reset=True):
        """(average ms before the step kernel, average ms of the step kernel, number of timed steps), HIP events on the launch stream.  The
        first number is pih_pre_kernel (controller + dispatch order) in the two-launch peg-in-hole step (schedule + 8); under the fused launch
        the controller wavefronts are part of the step kernel and it is only the gap between two event records, close to 0."""
        a = C.c_double(0); b = C.c_double(0); n = C.c_int64(0)
        self._chk(self.L.pih_timing2(self.h, int(reset), C.byref(a), C.byref(b), C.byref(n)), "pih_timing2")
        return a.value, b.value, n.value
