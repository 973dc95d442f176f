"""Inputs, fp64 references and measured fp32 bounds of the robot-model queries (include/pih_robot.h), shared by tests/test_robot_query.py
(host builds, no GPU) and tests/test_gpu_robot_query.py.  The references are the fp64 oracle's fk_arm / fk_ur5, jacobian_ee /
jacobian_ur5, mass_matrix / fly_mass_matrix, free_accel and FlyOracle.debug_udot; nothing here restates the kinematics, except the
Bullet link-damping torque of `ur5_link_damping_torque`, which is built from the oracle's frames and the model header's masses."""
import functools
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA, UR5 = 0, 1
NDOF = {PANDA: 9, UR5: 6}
NFRAMES = {PANDA: 10, UR5: 7}
NAMES = {PANDA: "panda", UR5: "ur5"}
LSW = 13

# fp32 bounds.  MEASURED = the largest error of the f32 HOST build against the fp64 oracle over `inputs()` (absolute, per quantity; printed
# by tests/test_robot_query.py::test_f32_host_build_within_measured_bounds with pytest -s; units: m, 1, m/s, rad/s, m or 1, kg m^2, N m; the
# references reach 1.3 m, 4.5 m/s, 6.8 rad/s, 4.6 kg m^2 and 76 N m).  The bound of the host f32 build and of the GPU is MARGIN x MEASURED: the GPU's -ffast-math
# sin / cos / rsqrt / division are looser than the host's.
MARGIN = 4.0
MEASURED = {
    PANDA: {"pos": 2.14e-07, "quat": 1.88e-07, "vlin": 8.01e-07, "vang": 1.1e-06, "jac": 3.93e-07, "mass": 1.27e-06, "tau": 1.49e-05},
    UR5: {"pos": 1.9e-07, "quat": 3.45e-07, "vlin": 4.96e-07, "vang": 7.99e-07, "jac": 4.27e-07, "mass": 1.33e-06, "tau": 1.41e-05},
}
# the same for the 24 pipe links of the peg-in-hole link states: the f32 host build against the f64 host build (which the URDF relations pin
# to 1e-9) on tests/test_robot_query.py's 16 reset states with random joint angles, rates and base twist; their largest velocity word is
# PIPE_VEL_REF (m/s or rad/s), and the velocity words are linear in the state's rates, so the velocity bounds scale with the largest
# velocity word of the states compared.  The input rounding of the state to fp32 is part of the figures (positions up to 3 m from the offsets).
MEASURED_PIPE = {"pos": 2.83e-07, "quat": 1.59e-07, "vlin": 4.89e-07, "vang": 5.34e-07}
PIPE_VEL_REF = 4.75


def pipe_bound(quantity, largest_velocity_word=0.0):
    scale = max(1.0, largest_velocity_word / PIPE_VEL_REF) if quantity in ("vlin", "vang") else 1.0
    return MARGIN * MEASURED_PIPE[quantity] * scale


def pipe_errors(got, want):
    """{quantity: largest absolute difference} of link-state rows [.., 13], quaternion signs aligned"""
    return {"pos": np.abs(got[..., :3] - want[..., :3]).max(), "quat": np.abs(align_quat(got[..., 3:7], want[..., 3:7]) - want[..., 3:7]).max(),
            "vlin": np.abs(got[..., 7:10] - want[..., 7:10]).max(), "vang": np.abs(got[..., 10:] - want[..., 10:]).max()}


def bound(robot, quantity):
    return MARGIN * MEASURED[robot][quantity]


@functools.lru_cache(None)
def model():
    """{name: value} of the numeric #defines of include/pih_model.h"""
    out = {}
    for m in re.finditer(r"^#define (PIH_\w+) (\{.*?\}|\(?-?[0-9.e+-]+\)?)\s*(?:/\*.*)?$", open(os.path.join(ROOT, "include", "pih_model.h")).read(), re.M):
        try:
            out[m.group(1)] = json.loads(m.group(2).replace("{", "[").replace("}", "]").replace("(", "").replace(")", ""))
        except ValueError:
            pass
    return out


def limits(robot):
    m = model()
    if robot == PANDA:
        return np.array(m["PIH_LINK_LO"][:9]), np.array(m["PIH_LINK_HI"][:9])
    return np.array(m["PIH_UR5_LO"]), np.array(m["PIH_UR5_HI"])


def rest(robot):
    return np.array(model()["PIH_ARM_REST" if robot == PANDA else "PIH_UR5_REST"], dtype=np.float64)


@functools.lru_cache(None)
def inputs(robot):
    """(q, qd, qdd, local) float64: q = 0; the rest pose; each joint alone at -/+ its limit; 200 random q within the limits (Panda fingers in
    [0, 0.04]); 20 with |q| up to 2 pi on the revolute joints.  qd, qdd uniform in +-2; local: 3 random points per problem, +-0.2 m."""
    rng = np.random.default_rng(1234 + robot)
    nd = NDOF[robot]; lo, hi = limits(robot)
    rows = [np.zeros(nd), rest(robot)]
    for j in range(nd):
        for lim in (lo[j], hi[j]):
            q = np.zeros(nd); q[j] = lim; rows.append(q)
    rows += list(rng.uniform(lo, hi, (200, nd)))
    wide = rng.uniform(-2 * np.pi, 2 * np.pi, (20, nd))
    if robot == PANDA:
        wide[:, 7:] = rng.uniform(0, 0.04, (20, 2))
    rows += list(wide)
    q = np.ascontiguousarray(rows, dtype=np.float64); n = len(q)
    return q, rng.uniform(-2, 2, (n, nd)), rng.uniform(-2, 2, (n, nd)), rng.uniform(-0.2, 0.2, (n, 3, 3))


def draw(robot, n, seed):
    """n problems drawn from inputs(robot) (with replacement), for the GPU batch sizes"""
    q, qd, qdd, local = inputs(robot)
    idx = np.random.default_rng(seed).integers(0, len(q), n)
    return idx, q[idx], qd[idx], qdd[idx], local[idx]


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                     [2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w],
                     [2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]])


def align_quat(got, ref):
    """got with the sign of each quaternion chosen to match ref (q and -q are the same rotation)"""
    s = np.where((got * ref).sum(-1, keepdims=True) < 0, -1.0, 1.0)
    return got * s


def _O():
    from oracle import oracle as O
    O.build()
    return O


def oracle_fk(robot, q, frame):
    O = _O()
    return O.fk_arm(q, frame) if robot == PANDA else O.fk_ur5(q, frame)


def _poses(robot, q):
    """([nf, 3], [nf, 3, 3]) of one q"""
    P = np.zeros((NFRAMES[robot], 3)); R = np.zeros((NFRAMES[robot], 3, 3))
    for f in range(NFRAMES[robot]):
        p, qt = oracle_fk(robot, q, f); P[f] = p; R[f] = quat_to_R(qt)
    return P, R


def _vee(dR):
    return np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])


@functools.lru_cache(None)
def ref_fk(robot):
    """[n, nf, 7] pos + quat of every frame of inputs(robot), from fk_arm / fk_ur5"""
    q = inputs(robot)[0]
    out = np.zeros((len(q), NFRAMES[robot], 7))
    for i in range(len(q)):
        for f in range(NFRAMES[robot]):
            p, qt = oracle_fk(robot, q[i], f); out[i, f, :3] = p; out[i, f, 3:] = qt
    return out


@functools.lru_cache(None)
def ref_vel(robot, h=1e-6):
    """[n, nf, 6]: central differences of the oracle's FK along qd; the angular part through the rotation difference (tests/test_ur5_chain.py)"""
    q, qd = inputs(robot)[:2]
    out = np.zeros((len(q), NFRAMES[robot], 6))
    for i in range(len(q)):
        Pp, Rp = _poses(robot, q[i] + h * qd[i]); Pm, Rm = _poses(robot, q[i] - h * qd[i])
        out[i, :, :3] = (Pp - Pm) / (2 * h)
        for f in range(NFRAMES[robot]):
            out[i, f, 3:] = _vee(Rp[f] @ Rm[f].T) / (4 * h)
    return out


@functools.lru_cache(None)
def ref_jac_ee(robot):
    O = _O(); q = inputs(robot)[0]
    out = np.zeros((len(q), 6, NDOF[robot]))
    for i in range(len(q)):
        Jl, Ja = O.jacobian_ee(q[i]) if robot == PANDA else O.jacobian_ur5(q[i])
        out[i, :3] = Jl; out[i, 3:] = Ja
    return out


@functools.lru_cache(None)
def ref_jac_fd(robot, h=1e-6):
    """[n, nf, 4, 6, ndof]: Jacobian of point k (0: the frame origin, 1..3: inputs().local[:, k - 1]) of every frame by central differences
    of the oracle's FK; the point is p + R local from the oracle's pose."""
    q, _, _, local = inputs(robot)
    nd, nf = NDOF[robot], NFRAMES[robot]
    out = np.zeros((len(q), nf, 4, 6, nd))
    for i in range(len(q)):
        pts = np.concatenate([np.zeros((1, 3)), local[i]])           # [4, 3]
        for j in range(nd):
            e = np.zeros(nd); e[j] = h
            Pp, Rp = _poses(robot, q[i] + e); Pm, Rm = _poses(robot, q[i] - e)
            for f in range(nf):
                out[i, f, :, :3, j] = ((Pp[f] + pts @ Rp[f].T) - (Pm[f] + pts @ Rm[f].T)) / (2 * h)
                out[i, f, :, 3:, j] = _vee(Rp[f] @ Rm[f].T) / (4 * h)
    return out


def panda_state(q, qd=None):
    """the oracle's 128-word state with q in PIH_S_QARM (qd in PIH_S_QDARM) and the identity pipe pose"""
    from peg_in_hole_gym_amd import _lib
    s = np.zeros(128); s[_lib.S_QARM:_lib.S_QARM + 9] = q
    if qd is not None:
        s[_lib.S_QDARM:_lib.S_QDARM + 9] = qd
    s[_lib.S_QUAT + 3] = 1.0
    return s


@functools.lru_cache(None)
def ref_mass(robot):
    O = _O(); q = inputs(robot)[0]
    if robot == PANDA:
        return np.array([O.mass_matrix(panda_state(qi))[:9, :9] for qi in q])
    return np.array([O.fly_mass_matrix(qi) for qi in q])


def ur5_free_accel(q, qd):
    """[n, 6] free acceleration of the oracle's random-fly step at (q, qd): FlyOracle.debug_udot after set_state and one step, the object
    parked 5 m away.  (Motor, limit and contact rows do not enter udot: it is computed before the solve.)"""
    O = _O(); n = len(q)
    F = O.FlyOracle(n)
    s = np.zeros((n, O.FLY_STATE_WORDS))
    s[:, O.F_Q:O.F_Q + 6] = q; s[:, O.F_QD:O.F_QD + 6] = qd; s[:, O.F_TARGET:O.F_TARGET + 6] = q
    s[:, O.F_OPOS:O.F_OPOS + 3] = (5.0, 0.0, 1.0); s[:, O.F_OQUAT + 3] = 1.0
    F.set_state(s)
    F.step(np.tile([0.4, 0.0, 0.5, 0.0, 0.0, 0.0], (n, 1)))
    return np.array([F.debug_udot(e)[:6] for e in range(n)])


@functools.lru_cache(None)
def ref_tau(robot):
    """tau = M (qdd - free acceleration of the step at (q, qd)), M and the free acceleration from the oracle"""
    O = _O(); q, qd, qdd, _ = inputs(robot)
    M = ref_mass(robot)
    if robot == PANDA:
        free = np.array([O.free_accel(panda_state(q[i], qd[i]))[:9] for i in range(len(q))])
    else:
        free = ur5_free_accel(q, qd)
    return np.einsum("nij,nj->ni", M, qdd - free)


def ur5_link_damping_torque(q, qd, k=0.04):
    """Generalised force of Bullet's per-link damping on the UR5 -- force m v_c (k + k |v_c|) at each link's centre of mass and moment
    I w (k + k |w|) -- from the oracle's frames (fk_ur5) and PIH_UR5_MASS / COM / INERTIA.  It is part of the step's free dynamics (and of
    the oracle's fly_rnea), odd in qd, and not part of PIH_UR5_DAMPING."""
    m = model(); mass, com, inertia, axis = m["PIH_UR5_MASS"], np.array(m["PIH_UR5_COM"]), np.array(m["PIH_UR5_INERTIA"]), np.array(m["PIH_UR5_AXIS"])
    P, R = _poses(UR5, q)
    a = np.array([R[j] @ axis[j] for j in range(6)])       # (a joint's axis is fixed by its own rotation)
    tau = np.zeros(6)
    for L in range(6):
        c = P[L] + R[L] @ com[L]
        Jl = np.zeros((3, 6)); Ja = np.zeros((3, 6))
        for j in range(L + 1):
            Jl[:, j] = np.cross(a[j], c - P[j]); Ja[:, j] = a[j]
        v, w = Jl @ qd, Ja @ qd
        I6 = inertia[L]; Il = np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]])
        Iw = R[L] @ Il @ R[L].T @ w
        tau += Jl.T @ (mass[L] * (k + k * np.linalg.norm(v)) * v) + Ja.T @ ((k + k * np.linalg.norm(w)) * Iw)
    return tau


# ---- link states of an env state, from the oracle's FK and the pipe's URDF
def pipe_joints():
    """[(origin xyz x 0.01 (the reference's globalScaling), axis)] of the pipe's 23 movable joints, from tests/golden's pipe.urdf; the fixed
    joint between pipe link 0 and 1 (merged into the root) is added to the first one's origin"""
    import xml.etree.ElementTree as ET
    root = ET.parse(os.path.join(ROOT, "tests", "golden", "model_assets", "peg_in_hole_gym", "envs", "assets", "urdf", "pipe.urdf")).getroot()
    out = []; carry = np.zeros(3)
    for j in root.findall("joint"):
        o = np.array([float(x) for x in j.find("origin").get("xyz").split()]) * 0.01
        if j.get("type") == "fixed":
            assert (j.find("origin").get("rpy") or "0 0 0").split() == ["0", "0", "0"]
            carry = carry + o
            continue
        out.append((carry + o, np.array([float(x) for x in j.find("axis").get("xyz").split()])))
        carry = np.zeros(3)
    return out
