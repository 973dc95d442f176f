"""Batched robot-model queries (include/pih_robot.h) without a GPU: the product's per-lane algorithms (csrc/pih_robot.h) compiled for the
host in double and float (tests/emul/pih_robot_emul.cpp) against the fp64 oracle, over tests/robot_cases.py's inputs for both robots;
the link-state algorithm on reset states of both tasks; the C ABI; the sanitizer run of a stand-alone program; and the code-object
metadata of the new kernels (no scratch).
fp64: every directly compared quantity agrees to 1e-9 x its largest magnitude (fp64 rounding at these sizes); comparisons with central
differences of the oracle's FK (h = 1e-6) to 1e-6.  fp32: robot_cases.MARGIN x robot_cases.MEASURED."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import robot_cases as rc
from tests.emul import robot_emul
from tests.oracle_backend import RecordingBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOTS = (rc.PANDA, rc.UR5)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("robot_emul")
    return {prec: robot_emul.Host(robot_emul.lib(d, prec)) for prec in ("f64", "f32")}


def errors(H, robot):
    """{quantity: (largest absolute error against the oracle, largest magnitude of the reference)} of one host build; FK, velocities, the
    end-effector Jacobian, mass matrix and inverse dynamics over all of inputs(robot)"""
    q, qd, qdd, _ = rc.inputs(robot)
    fk = H.fk(robot, q, qd); ref = rc.ref_fk(robot); vel = rc.ref_vel(robot)
    out = {"pos": (np.abs(fk[..., :3] - ref[..., :3]).max(), np.abs(ref[..., :3]).max()),
           "quat": (np.abs(rc.align_quat(fk[..., 3:7], ref[..., 3:]) - ref[..., 3:]).max(), 1.0),
           "vlin": (np.abs(fk[..., 7:10] - vel[..., :3]).max(), np.abs(vel[..., :3]).max()),
           "vang": (np.abs(fk[..., 10:13] - vel[..., 3:]).max(), np.abs(vel[..., 3:]).max())}
    J = H.jacobian(robot, q, rc.NFRAMES[robot] - 1); Jr = rc.ref_jac_ee(robot)
    out["jac"] = (np.abs(J - Jr).max(), np.abs(Jr).max())
    M = H.mass_matrix(robot, q); Mr = rc.ref_mass(robot)
    out["mass"] = (np.abs(M - Mr).max(), np.abs(Mr).max())
    tau = H.inverse_dynamics(robot, q, qd, qdd); tr = rc.ref_tau(robot)
    out["tau"] = (np.abs(tau - tr).max(), np.abs(tr).max())
    return out


@pytest.mark.parametrize("robot", ROBOTS)
def test_f64_host_build_matches_the_oracle(hosts, robot):
    """FK of every frame == fk_arm / fk_ur5, EE Jacobian == jacobian_ee / jacobian_ur5, M == mass_matrix[0:9, 0:9] / fly_mass_matrix,
    tau == M (qdd - free acceleration): 1e-9 x the largest magnitude.  Velocities == central differences of the oracle's FK: 1e-6."""
    e = errors(hosts["f64"], robot)
    print(rc.NAMES[robot], "f64", {k: "%.3g of %.3g" % v for k, v in e.items()})
    for k in ("pos", "quat", "jac", "mass", "tau"):
        assert e[k][0] <= 1e-9 * e[k][1], (k, e[k])
    for k in ("vlin", "vang"):
        assert e[k][0] <= 1e-6, (k, e[k])


@pytest.mark.parametrize("robot", ROBOTS)
def test_f32_host_build_within_measured_bounds(hosts, robot):
    """The f32 host build against the oracle: each quantity within MARGIN x MEASURED (tests/robot_cases.py; MEASURED is what this test
    printed when the table was written)."""
    e = errors(hosts["f32"], robot)
    print(rc.NAMES[robot], "f32 measured", {k: float("%.3g" % v[0]) for k, v in e.items()})
    for k, (err, _) in e.items():
        assert err <= rc.bound(robot, k), (k, err, rc.bound(robot, k))


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("robot", ROBOTS)
def test_jacobian_of_every_frame_and_point(hosts, robot, prec):
    """Every frame, at its origin and at 3 random local points, == central differences of the oracle's FK (fp64: 1e-6; fp32: the jac
    bound + 1e-6); the columns of joints that are not ancestors are exactly 0, a finger column is (axis, 0); J qd == the velocity words of
    robot_fk (fp64: 1e-9 x magnitude; fp32: the velocity bounds)."""
    H = hosts[prec]; q, qd, _, local = rc.inputs(robot)
    nd, nf = rc.NDOF[robot], rc.NFRAMES[robot]
    ref = rc.ref_jac_fd(robot); fk = H.fk(robot, q, qd)
    tol = 1e-6 if prec == "f64" else rc.bound(robot, "jac") + 1e-6
    worst = 0.0
    for f in range(nf):
        for k in range(4):
            J = H.jacobian(robot, q, f, None if k == 0 else local[:, k - 1])
            worst = max(worst, np.abs(J - ref[:, f, k]).max())
            link = f if f < nd else (6 if robot == rc.PANDA else 5)
            for j in range(nd):
                anc = (j <= link) if robot == rc.UR5 else ((j <= 6 and j <= link) or j == link)
                if not anc:
                    assert (J[:, :, j] == 0).all(), (f, j)
            if robot == rc.PANDA and f in (7, 8):
                assert (J[:, 3:, f] == 0).all() and np.allclose(np.linalg.norm(J[:, :3, f], axis=1), 1, atol=1e-6)
            if k == 0:
                v = np.einsum("nij,nj->ni", J, qd)
                if prec == "f64":
                    assert np.abs(v - fk[:, f, 7:]).max() <= 1e-9 * max(1.0, np.abs(fk[:, f, 7:]).max())
                else:
                    assert np.abs(v[:, :3] - fk[:, f, 7:10]).max() <= 2 * rc.bound(robot, "vlin") and np.abs(v[:, 3:] - fk[:, f, 10:]).max() <= 2 * rc.bound(robot, "vang")
    print(rc.NAMES[robot], prec, "jacobian vs central differences: %.3g" % worst)
    assert worst <= tol


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("robot", ROBOTS)
def test_mass_matrix_properties(hosts, robot, prec):
    """bitwise symmetric; numpy.linalg.cholesky succeeds; UR5: 1/2 qd^T M qd == fly_arm_kinetic_energy."""
    H = hosts[prec]; q, qd, _, _ = rc.inputs(robot)
    M = H.mass_matrix(robot, q)
    assert np.array_equal(M, M.transpose(0, 2, 1))
    np.linalg.cholesky(M)
    if robot == rc.UR5:
        from oracle import oracle as O
        ke = np.array([O.fly_arm_kinetic_energy(q[i], qd[i]) for i in range(len(q))])
        mine = 0.5 * np.einsum("ni,nij,nj->n", qd, M, qd)
        tol = 1e-9 * np.abs(ke).max() if prec == "f64" else rc.bound(robot, "mass") * 0.5 * (np.abs(qd).sum(1) ** 2).max()
        assert np.abs(mine - ke).max() <= tol


@pytest.mark.parametrize("prec", ("f64", "f32"))
def test_ur5_inverse_dynamics_parts(hosts, prec):
    """tau(q, 0, e_j) - tau(q, 0, 0) == column j of fly_mass_matrix.
    The part of tau(q, qd, 0) - tau(q, 0, 0) that is even in qd, (tau(qd) + tau(-qd)) / 2 - tau(0), is the Coriolis / centrifugal term: it
    equals sum_jk (dM_ij/dq_k - 1/2 dM_jk/dq_i) qd_j qd_k, from central differences of fly_mass_matrix (h = 1e-5, tolerance 1e-5 x |qd|^2).
    The odd part, (tau(qd) - tau(-qd)) / 2, is the damping: PIH_UR5_DAMPING qd plus Bullet's per-link damping, which the step's free
    dynamics contain (robot_cases.ur5_link_damping_torque builds it from the oracle's frames).
    Over these inputs the link term reaches 1.13 N m where the joint term reaches 1.0 N m; the joint term is read from PIH_UR5_DAMPING,
    the link term is computed independently of the code under test."""
    from oracle import oracle as O
    H = hosts[prec]; q, qd, _, _ = rc.inputs(rc.UR5)
    n = len(q); z = np.zeros_like(q)
    t0 = H.inverse_dynamics(rc.UR5, q, z, z)
    Mr = rc.ref_mass(rc.UR5)
    tol_m = 1e-9 * np.abs(Mr).max() if prec == "f64" else 2 * rc.bound(rc.UR5, "tau")
    for j in range(6):
        e = np.zeros_like(q); e[:, j] = 1
        assert np.abs(H.inverse_dynamics(rc.UR5, q, z, e) - t0 - Mr[:, :, j]).max() <= tol_m
    tp, tm = H.inverse_dynamics(rc.UR5, q, qd, z), H.inverse_dynamics(rc.UR5, q, -qd, z)
    even, odd = (tp + tm) / 2 - t0, (tp - tm) / 2
    damping = np.array(rc.model()["PIH_UR5_DAMPING"])
    want_odd = np.array([damping * qd[i] + rc.ur5_link_damping_torque(q[i], qd[i]) for i in range(n)])
    tol = 1e-9 * np.abs(want_odd).max() if prec == "f64" else 2 * rc.bound(rc.UR5, "tau")
    assert np.abs(odd - want_odd).max() <= tol, np.abs(odd - want_odd).max()
    h = 1e-5
    for i in range(0, n, 12):       # (12 mass matrices per problem: every 12th problem)
        dM = np.zeros((6, 6, 6))
        for k in range(6):
            e = np.zeros(6); e[k] = h
            dM[:, :, k] = (O.fly_mass_matrix(q[i] + e) - O.fly_mass_matrix(q[i] - e)) / (2 * h)
        cor = np.einsum("ijk,j,k->i", dM, qd[i], qd[i]) - 0.5 * np.einsum("jki,j,k->i", dM, qd[i], qd[i])
        assert np.abs(even[i] - cor).max() <= 1e-5 * (qd[i] ** 2).sum() + (0 if prec == "f64" else 2 * rc.bound(rc.UR5, "tau")), (i, even[i], cor)


def test_velocity_words_are_zero_without_qd(hosts):
    for robot in ROBOTS:
        q = rc.inputs(robot)[0]
        for prec in ("f64", "f32"):
            a = hosts[prec].fk(robot, q, None)
            assert (a[..., 7:] == 0).all() and np.array_equal(a[..., :7], hosts[prec].fk(robot, q, np.zeros_like(q))[..., :7])


def test_nan_and_huge_inputs_stay_per_problem(hosts):
    """A NaN q gives non-finite outputs for that problem and leaves its neighbours bit for bit; |q| far beyond 2 pi stays finite."""
    H = hosts["f32"]
    for robot in ROBOTS:
        q, qd, qdd, _ = (x[:8].copy() for x in rc.inputs(robot))
        base = (H.fk(robot, q, qd), H.jacobian(robot, q, 3), H.mass_matrix(robot, q), H.inverse_dynamics(robot, q, qd, qdd))
        q[3, 1] = np.nan
        bad = (H.fk(robot, q, qd), H.jacobian(robot, q, 3), H.mass_matrix(robot, q), H.inverse_dynamics(robot, q, qd, qdd))
        keep = np.arange(8) != 3
        for a, b in zip(base, bad):
            assert np.array_equal(a[keep], b[keep]) and not np.isfinite(b[3]).all()
        q[3, 1] = 1e6
        for a in (H.fk(robot, q, qd), H.jacobian(robot, q, 3), H.mass_matrix(robot, q), H.inverse_dynamics(robot, q, qd, qdd)):
            assert np.isfinite(a).all()


# ---------------------------------------------------------------------------------------------- link states of an env state
def reset_states(task, n=16):
    """n reset states [n, words] of the fp64 oracle with random arm velocities, pipe joint angles / rates and a base twist, and offsets"""
    from oracle import oracle as O
    from peg_in_hole_gym_amd import _lib
    O.build()
    rng = np.random.default_rng(7 + task)
    off = rng.uniform(-3, 3, (n, 3))
    if task == 0:
        o = O.Oracle(n, offsets=off); o.reset(); s = o.get_state()
        s[:, _lib.S_QDARM:_lib.S_QDARM + 9] = rng.uniform(-1, 1, (n, 9))
        s[:, _lib.S_VLIN:_lib.S_VLIN + 6] = rng.uniform(-1, 1, (n, 6))
        s[:, _lib.S_QJ:_lib.S_QJ + 23] = rng.uniform(-0.3, 0.3, (n, 23)); s[:, _lib.S_QDJ:_lib.S_QDJ + 23] = rng.uniform(-1, 1, (n, 23))
        qt = rng.normal(size=(n, 4)); s[:, _lib.S_QUAT:_lib.S_QUAT + 4] = qt / np.linalg.norm(qt, axis=1, keepdims=True)
        s[:, _lib.S_GRASP] = 23
        return s
    o = O.FlyOracle(n, offsets=off); o.reset(); s = o.get_state()
    s[:, _lib.F_QD:_lib.F_QD + 6] = rng.uniform(-1, 1, (n, 6))
    return s


@pytest.mark.parametrize("prec", ("f64", "f32"))
def test_peg_link_states(hosts, oracle_mod, prec):
    """fp64: arm frames == robot_fk of the state's q / qd + the offset; pipe link 0 == the state's base pose and twist; last link origin +
    R (0, 0.015, 0) == the oracle's tip_pose with PIH_S_GRASP = 23; consecutive pipe links: R_k^T (o_k+1 - o_k) and R_k^T R_k+1 == the joint
    origin x 0.01 and the axis-angle of the joint's axis by PIH_S_QJ, both read from pipe.urdf; the velocities of consecutive links obey
    the rigid-body relation with the joint rate PIH_S_QDJ: all to 1e-9 (1e-8 on products of two such quantities).
    fp32: every word of the 24 pipe links against the fp64 build, within MARGIN x MEASURED_PIPE (tests/robot_cases.py; the figures are
    printed); the arm frames == robot_fk + offset within one fp32 rounding of the sum (positions up to 4.3 m: 4.8e-7)."""
    from peg_in_hole_gym_amd import _lib
    H = hosts[prec]; s = reset_states(0); n = len(s)
    tol = 1e-9
    ls = H.link_states(0, s)
    assert ls.shape == (n, 34, 13)
    off = s[:, _lib.S_OFFSET:_lib.S_OFFSET + 3]
    arm = H.fk(rc.PANDA, s[:, _lib.S_QARM:_lib.S_QARM + 9], s[:, _lib.S_QDARM:_lib.S_QDARM + 9])
    arm[..., :3] += off[:, None, :]
    assert np.abs(ls[:, :10] - arm).max() <= (0 if prec == "f64" else 4.8e-7)
    if prec == "f32":
        want = hosts["f64"].link_states(0, s)
        e = rc.pipe_errors(ls[:, 10:], want[:, 10:]); vmax = np.abs(want[:, 10:, 7:]).max()
        print("pipe links f32 measured", {k: float("%.3g" % v) for k, v in e.items()}, "largest velocity word %.3g" % vmax)
        for k, v in e.items():
            assert v <= rc.pipe_bound(k, vmax), (k, v)
        return
    root = ls[:, 10]
    assert np.abs(root[:, :3] - (s[:, _lib.S_POS:_lib.S_POS + 3] + off)).max() <= tol
    assert np.abs(rc.align_quat(root[:, 3:7], s[:, _lib.S_QUAT:_lib.S_QUAT + 4]) - s[:, _lib.S_QUAT:_lib.S_QUAT + 4]).max() <= max(tol, 1e-12)
    assert np.abs(root[:, 7:] - s[:, _lib.S_VLIN:_lib.S_VLIN + 6]).max() <= tol
    o = oracle_mod.Oracle(n); full = o.get_state(); full[:] = s; o.set_state(full); tip = o.tip_pose()
    joints = rc.pipe_joints()
    assert len(joints) == 23
    for e in range(n):
        R = [rc.quat_to_R(ls[e, 10 + k, 3:7]) for k in range(24)]
        last = ls[e, 33]
        assert np.abs(last[:3] + R[23] @ [0, 0.015, 0] - off[e] - tip[e, :3]).max() <= tol
        assert np.abs(R[23] - rc.quat_to_R(tip[e, 3:])).max() <= 10 * tol
        for k in range(23):
            origin, axis = joints[k]
            a, b = ls[e, 10 + k], ls[e, 11 + k]
            assert np.abs(R[k].T @ (b[:3] - a[:3]) - origin).max() <= tol
            th = s[e, _lib.S_QJ + k]; K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
            assert np.abs(R[k].T @ R[k + 1] - (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)).max() <= 10 * tol
            assert np.abs(b[7:10] - (a[7:10] + np.cross(a[10:], b[:3] - a[:3]))).max() <= 10 * tol
            assert np.abs(b[10:] - (a[10:] + s[e, _lib.S_QDJ + k] * (R[k] @ axis))).max() <= 10 * tol


@pytest.mark.parametrize("prec", ("f64", "f32"))
def test_fly_link_states(hosts, prec):
    from peg_in_hole_gym_amd import _lib
    H = hosts[prec]; s = reset_states(1); n = len(s)
    ls = H.link_states(1, s)
    assert ls.shape == (n, 8, 13)
    off = s[:, _lib.F_OFFSET:_lib.F_OFFSET + 3]
    arm = H.fk(rc.UR5, s[:, _lib.F_Q:_lib.F_Q + 6], s[:, _lib.F_QD:_lib.F_QD + 6])
    arm[..., :3] += off[:, None, :]
    assert np.abs(ls[:, :7] - arm).max() <= (0 if prec == "f64" else 4.8e-7)       # (one fp32 rounding of position + offset, up to 4.3 m)
    assert np.abs(ls[:, 6, :3] - s[:, _lib.F_EE:_lib.F_EE + 3]).max() <= (1e-9 if prec == "f64" else rc.bound(rc.UR5, "pos") + 4.8e-7)       # the state's own ee word
    want = np.concatenate([s[:, _lib.F_OPOS:_lib.F_OPOS + 3] + off, s[:, _lib.F_OQUAT:_lib.F_OQUAT + 4], s[:, _lib.F_OVLIN:_lib.F_OVLIN + 6]], axis=1)
    assert np.abs(ls[:, 7] - want).max() <= (0 if prec == "f64" else 4.8e-7)


# ---------------------------------------------------------------------------------------------- C ABI
def test_robot_exports_match_header_and_library():
    import __graft_entry__ as ge
    ge.build()
    from peg_in_hole_gym_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pih_robot.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(pih_[a-z_0-9]+)\s*\(", hdr)))
    assert names == sorted(_lib.ROBOT_EXPORTS) and not set(names) & set(_lib.EXPORTS)
    assert '#include "pih_robot.h"' in open(os.path.join(ROOT, "include", "pih.h")).read()
    L = C.CDLL(os.path.join(ROOT, "peg_in_hole_gym_amd", "csrc", "libpih_hip.so"))
    for n in names:
        assert hasattr(L, n), n
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "peg_in_hole_gym_amd", "csrc", "libpih_hip.so")], text=True)
    exported = set(re.findall(r" T (pih_[a-z_0-9]+)$", out, re.M))
    assert exported == set(_lib.EXPORTS) | set(_lib.ROBOT_EXPORTS) | set(_lib.VIEW_EXPORTS) | set(_lib.LIGHT_EXPORTS), exported
    assert L.pih_abi_version() == 4 == _lib.ABI_VERSION
    assert (_lib.ROBOT_PANDA, _lib.ROBOT_UR5, _lib.LINK_STATE_WORDS) == (0, 1, 13)
    assert _lib.robot_dims(_lib.ROBOT_PANDA) == (9, 10) and _lib.robot_dims(_lib.ROBOT_UR5) == (6, 7)
    assert _lib.link_states_frames(_lib.TASK_PEG_IN_HOLE) == 34 and _lib.link_states_frames(_lib.TASK_RANDOM_FLY) == 8
    with pytest.raises(_lib.PihError):
        _lib.robot_dims(2)
    assert L.pih_link_states_frames(2) < 0


def test_argument_checks_that_need_no_device():
    """-2 with the argument named in pih_last_error: a NULL handle in every call, pih_robot_dims' robot and output.  (The checks that need a
    handle -- robot, n, frame, NULL pointers, the env range -- are in tests/test_gpu_robot_query.py: a handle exists only on a GPU.)"""
    import __graft_entry__ as ge
    ge.build()
    from peg_in_hole_gym_amd import _lib
    L = _lib.load()
    calls = {"pih_robot_fk": lambda: L.pih_robot_fk(None, 0, 1, None, None, None, None),
             "pih_robot_jacobian": lambda: L.pih_robot_jacobian(None, 0, 1, None, 0, None, None, None),
             "pih_robot_mass_matrix": lambda: L.pih_robot_mass_matrix(None, 0, 1, None, None, None),
             "pih_robot_inverse_dynamics": lambda: L.pih_robot_inverse_dynamics(None, 0, 1, None, None, None, None, None),
             "pih_link_states": lambda: L.pih_link_states(None, None, 0, 1, None)}
    for name, f in calls.items():
        assert f() == -2, name
        msg = L.pih_last_error(None).decode()
        assert msg.startswith(name + ": h "), msg
    out = (C.c_int32 * 2)()
    assert L.pih_robot_dims(7, C.byref(out)) == -2 and "robot" in L.pih_last_error(None).decode()
    assert L.pih_robot_dims(0, None) == -2 and "out" in L.pih_last_error(None).decode()


def test_task_classes_delegate_link_states():
    from peg_in_hole_gym_amd.envs.peg_in_hole import PegInHole, RandomFly
    for cls in (PegInHole, RandomFly):
        t = cls(backend_factory=RecordingBackend)
        assert t.link_states(env_begin=0) == "states" and t._backend.calls == [{"env_begin": 0}]


# ---------------------------------------------------------------------------------------------- sanitizers, scratch
def test_sanitized_standalone_program(tmp_path):
    """The float build inside a stand-alone program (its own main) under -fsanitize=address,undefined, run once as a plain subprocess over
    the test inputs of both robots and 16 reset states of each task: exit status 0, nothing on stderr, every output word finite."""
    exe = robot_emul.build_sanitized_program(tmp_path)
    for robot in ROBOTS:
        q, qd, qdd, local = rc.inputs(robot)
        peg, fly = reset_states(0), reset_states(1)
        peg256 = np.zeros((len(peg), 256)); peg256[:, :128] = peg
        f = tmp_path / ("inputs_%d.bin" % robot)
        np.concatenate([[robot, len(q)], q.ravel(), qd.ravel(), qdd.ravel(), local[:, 0].ravel(), [len(peg256)], peg256.ravel(), [len(fly)], fly.ravel()]).astype(np.float64).tofile(str(f))
        r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        m = re.fullmatch(r"robot (\d+) n (\d+) words (\d+) finite (\d+)\n", r.stdout)
        assert m and int(m.group(1)) == robot and int(m.group(2)) == len(q) and m.group(3) == m.group(4) and int(m.group(3)) > 0, r.stdout


def test_new_kernels_use_no_scratch():
    """Code-object metadata of pih_robot.hip alone (tools/isa_fingerprint.py's assembly() / metadata()): every kernel has
    private_segment_fixed_size == 0 -- a lane that spills its link arrays has lost the point of the one-problem-per-lane layout -- and at
    most 33.5 KB of LDS (the staged Panda link states)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_fingerprint as fp
    assert "pih_robot.hip" in fp.sources(ROOT)
    meta = fp.metadata(fp.assembly(ROOT, "pih_robot.hip"))
    kinds = ("pih_robot_fk_kernel", "pih_robot_jacobian_kernel", "pih_robot_mass_kernel", "pih_robot_invdyn_kernel")
    assert len(meta) == 3 * 4 + 2 + 2, sorted(meta)       # three queries x two robots x direct / staged, inverse dynamics x two robots, two link-state kernels
    assert all(sum(k in name for name in meta) == (2 if "invdyn" in k else 4) for k in kinds) and sum("link_states_kernel" in name for name in meta) == 2
    for name, md in meta.items():
        assert int(md["private_segment_fixed_size"]) == 0, (name, md)
        assert int(md["group_segment_fixed_size"]) <= 64 * 131 * 4, (name, md)
