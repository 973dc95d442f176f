"""Builder and ctypes binding of the TEST-ONLY host build of the robot-model queries (tests/emul/pih_robot_emul.cpp): the product's
peg_in_hole_gym_amd/csrc/pih_robot.h compiled with g++ for the host, in double ("f64") and float ("f32"), with the flags of this
directory's Makefile; and the stand-alone sanitizer program (pih_robot_sanitize_main.cpp).  Everything is built into a directory the
caller names (a pytest tmp dir), nothing in-tree."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emul.render_emul import CXX, CXXFLAGS

_DIR = os.path.dirname(os.path.abspath(__file__))
# (the default CXXFLAGS of tests/emul/Makefile)
# the flags of the Makefile's sanitizer build
SANFLAGS = ["-O1", "-g", "-std=c++17", "-fno-fast-math", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
PANDA, UR5 = 0, 1


def build(outdir, prec):
    so = os.path.join(str(outdir), "libpih_robot_emul_%s.so" % prec)
    subprocess.check_call([CXX] + CXXFLAGS + ["-DPIH_REAL=" + {"f64": "double", "f32": "float"}[prec], "-shared", "-o", so, "pih_robot_emul.cpp"], cwd=_DIR)
    return so


def build_sanitized_program(outdir):
    exe = os.path.join(str(outdir), "pih_robot_sanitize")
    subprocess.check_call([CXX] + SANFLAGS + ["-DPIH_REAL=float", "-o", exe, "pih_robot_sanitize_main.cpp"], cwd=_DIR)
    return exe


def lib(outdir, prec):
    L = C.CDLL(build(outdir, prec))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.pihr_dims.argtypes = [C.c_int, ip]
    L.pihr_fk.argtypes = [C.c_int, C.c_int, dp, dp, dp]
    L.pihr_jacobian.argtypes = [C.c_int, C.c_int, dp, C.c_int, dp, dp]
    L.pihr_mass_matrix.argtypes = [C.c_int, C.c_int, dp, dp]
    L.pihr_inverse_dynamics.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp]
    L.pihr_link_states.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp]
    assert L.pihr_real_bytes() == (8 if prec == "f64" else 4)
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Host:
    """numpy front of one host build: float64 arrays in and out, shapes as the C ABI's"""

    def __init__(self, L):
        self.L = L

    def dims(self, robot):
        d = (C.c_int * 2)()
        assert self.L.pihr_dims(robot, d) == 0
        return d[0], d[1]

    def fk(self, robot, q, qd=None):
        q = np.ascontiguousarray(q, dtype=np.float64); out = np.zeros((len(q), self.dims(robot)[1], 13))
        qd = None if qd is None else np.ascontiguousarray(qd, dtype=np.float64)
        assert self.L.pihr_fk(robot, len(q), _dp(q), _dp(qd) if qd is not None else None, _dp(out)) == 0
        return out

    def jacobian(self, robot, q, frame, local=None):
        q = np.ascontiguousarray(q, dtype=np.float64); out = np.zeros((len(q), 6, self.dims(robot)[0]))
        local = None if local is None else np.ascontiguousarray(local, dtype=np.float64)
        assert self.L.pihr_jacobian(robot, len(q), _dp(q), frame, _dp(local) if local is not None else None, _dp(out)) == 0
        return out

    def mass_matrix(self, robot, q):
        q = np.ascontiguousarray(q, dtype=np.float64); nd = self.dims(robot)[0]; out = np.zeros((len(q), nd, nd))
        assert self.L.pihr_mass_matrix(robot, len(q), _dp(q), _dp(out)) == 0
        return out

    def inverse_dynamics(self, robot, q, qd, qdd):
        q, qd, qdd = (np.ascontiguousarray(x, dtype=np.float64) for x in (q, qd, qdd)); out = np.zeros((len(q), self.dims(robot)[0]))
        assert self.L.pihr_inverse_dynamics(robot, len(q), _dp(q), _dp(qd), _dp(qdd), _dp(out)) == 0
        return out

    def link_states(self, task, states):
        s = np.ascontiguousarray(states, dtype=np.float64); frames = self.L.pihr_link_states_frames(task)
        out = np.zeros((len(s), frames, 13))
        assert self.L.pihr_link_states(task, len(s), s.shape[1], _dp(s), _dp(out)) == 0
        return out
