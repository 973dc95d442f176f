"""Builder and ctypes binding of the TEST-ONLY host build of the robot clearance queries (tests/emul/pih_clear_emul.cpp): the product's
peg_in_hole_gym_amd/csrc/pih_clear.h compiled with g++ for the host, in double ("f64") and float ("f32"), with the flags of this
directory's Makefile, bound as dist_emul.py binds the closest-point queries; and the stand-alone sanitizer program
(pih_clear_sanitize_main.cpp).  Everything is built into a directory the caller names (a pytest tmp dir), nothing in-tree."""
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
    so = os.path.join(str(outdir), "libpih_clear_emul_%s.so" % prec)
    subprocess.check_call([CXX] + CXXFLAGS + ["-DPIH_REAL=" + {"f64": "double", "f32": "float"}[prec], "-shared", "-o", so, "pih_clear_emul.cpp"], cwd=_DIR)
    L = C.CDLL(so)
    L.pihclear_view.argtypes = [_dp, _fp, C.c_int, C.c_int, C.c_double, C.c_int, _dp]
    L.pihclear_fly.argtypes = [_dp, C.c_int, _fp, C.c_int, C.c_int, C.c_double, C.c_int, _dp]
    assert L.pihclear_real_bytes() == (8 if prec == "f64" else 4)
    assert (L.pihclear_probes(0), L.pihclear_probes(1)) == (_lib.CLEAR_PROBES_PANDA, _lib.CLEAR_PROBES_UR5)
    return L


def libs(outdir):
    return {prec: lib(outdir, prec) for prec in ("f64", "f32")}


def build_sanitized_program(outdir):
    exe = os.path.join(str(outdir), "pih_clear_sanitize")
    subprocess.check_call([CXX] + SANFLAGS + ["-DPIH_REAL=float", "-o", exe, "pih_clear_sanitize_main.cpp"], cwd=_DIR)
    return exe


def records_of(L, task, rec, obj, q, groups, reach, cull=True):
    """records float64 [C, NP, 12] of the configurations q float32 [C, ndof] (None: the record's own joint words, C = 1) against one state
    record; task "peg" | "fly"; cull: with or without the bounding-sphere rejection"""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    ndof, NP = (9, _lib.CLEAR_PROBES_PANDA) if task == "peg" else (6, _lib.CLEAR_PROBES_UR5)
    if q is not None:
        q = np.ascontiguousarray(q, dtype=np.float32)
        assert q.ndim == 2 and q.shape[1] == ndof
    n = 1 if q is None else len(q)
    out = np.full((n, NP, _lib.CLEAR_WORDS), np.nan)
    qp = None if q is None else q.ctypes.data_as(_fp)
    if task == "peg":
        assert rec.shape == (_lib.STATE_WORDS,)
        rc = L.pihclear_view(rec.ctypes.data_as(_dp), qp, n, groups, float(reach), int(cull), out.ctypes.data_as(_dp))
    else:
        assert rec.shape == (_lib.FLY_STATE_WORDS,)
        rc = L.pihclear_fly(rec.ctypes.data_as(_dp), obj, qp, n, groups, float(reach), int(cull), out.ctypes.data_as(_dp))
    assert rc == 0, rc
    return out


def clearance(L, case, cull=True):
    """a case of tests/clear_cases.py -> records float64 [C, NP, 12]"""
    return records_of(L, case["task"], case["rec"], case["obj"], case["q"], case["groups"], case["reach"], cull)
