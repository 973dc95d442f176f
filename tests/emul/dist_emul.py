"""Builder and ctypes binding of the TEST-ONLY host build of the batched closest-point queries (tests/emul/pih_dist_emul.cpp): the
product's peg_in_hole_gym_amd/csrc/pih_dist.h compiled with g++ for the host, in double ("f64") and float ("f32"), with the flags of this
directory's Makefile, bound as ray_emul.py binds the ray tests; and the stand-alone sanitizer program (pih_dist_sanitize_main.cpp).
Everything is built into a directory the caller names (a pytest tmp dir), nothing in-tree."""
import ctypes as C
import os
import subprocess

import numpy as np

from peg_in_hole_gym_amd import _lib
from tests.emul.render_emul import CXX, CXXFLAGS
from tests.emul.robot_emul import SANFLAGS

_DIR = os.path.dirname(os.path.abspath(__file__))
_dp, _fp = C.POINTER(C.c_double), C.POINTER(C.c_float)


def lib(outdir, prec):
    so = os.path.join(str(outdir), "libpih_dist_emul_%s.so" % prec)
    subprocess.check_call([CXX] + CXXFLAGS + ["-DPIH_REAL=" + {"f64": "double", "f32": "float"}[prec], "-shared", "-o", so, "pih_dist_emul.cpp"], cwd=_DIR)
    L = C.CDLL(so)
    L.pihdist_view.argtypes = [_dp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _dp]
    L.pihdist_fly.argtypes = [_dp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _dp]
    assert L.pihdist_real_bytes() == (8 if prec == "f64" else 4)
    return L


def libs(outdir):
    return {prec: lib(outdir, prec) for prec in ("f64", "f32")}


def build_sanitized_program(outdir):
    exe = os.path.join(str(outdir), "pih_dist_sanitize")
    subprocess.check_call([CXX] + SANFLAGS + ["-DPIH_REAL=float", "-o", exe, "pih_dist_sanitize_main.cpp"], cwd=_DIR)
    return exe


def points_of(L, task, rec, obj, points, flags, groups, cull=True):
    """records float64 [n, 8] of the queries float32 [n, 4] against one state record; task "peg" | "fly"; cull: with the bounding-sphere
    rejection of the kernels, or with every distance function called"""
    rec = np.ascontiguousarray(rec, dtype=np.float64); points = np.ascontiguousarray(points, dtype=np.float32)
    assert points.ndim == 2 and points.shape[1] == _lib.POINT_WORDS
    out = np.full((len(points), _lib.CLOSEST_WORDS), np.nan)
    if task == "peg":
        assert rec.shape == (_lib.STATE_WORDS,)
        rc = L.pihdist_view(rec.ctypes.data_as(_dp), points.ctypes.data_as(_fp), len(points), flags, groups, int(cull), out.ctypes.data_as(_dp))
    else:
        assert rec.shape == (_lib.FLY_STATE_WORDS,)
        rc = L.pihdist_fly(rec.ctypes.data_as(_dp), obj, points.ctypes.data_as(_fp), len(points), flags, groups, int(cull), out.ctypes.data_as(_dp))
    assert rc == 0, rc
    return out


def closest(L, case, cull=True):
    """a case of tests/dist_cases.py -> records float64 [n, 8]"""
    return points_of(L, case["task"], case["rec"], case["obj"], case["points"], case["flags"], case["groups"], cull)
