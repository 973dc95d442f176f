"""Builder and ctypes binding of the TEST-ONLY host build of the batched ray tests (tests/emul/pih_rays_emul.cpp): the product's
peg_in_hole_gym_amd/csrc/pih_rays.h compiled with g++ for the host, in double ("f64") and float ("f32"), with the flags of this
directory's Makefile, bound as render_emul.py binds the cameras; and the stand-alone sanitizer program (pih_rays_sanitize_main.cpp).
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
    so = os.path.join(str(outdir), "libpih_rays_emul_%s.so" % prec)
    subprocess.check_call([CXX] + CXXFLAGS + ["-DPIH_REAL=" + {"f64": "double", "f32": "float"}[prec], "-shared", "-o", so, "pih_rays_emul.cpp"], cwd=_DIR)
    L = C.CDLL(so)
    L.pihray_view.argtypes = [_dp, _fp, C.c_int, C.c_int, C.c_int, _dp]
    L.pihray_fly.argtypes = [_dp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, _dp]
    assert L.pihray_real_bytes() == (8 if prec == "f64" else 4)
    return L


def libs(outdir):
    return {prec: lib(outdir, prec) for prec in ("f64", "f32")}


def build_sanitized_program(outdir):
    exe = os.path.join(str(outdir), "pih_rays_sanitize")
    subprocess.check_call([CXX] + SANFLAGS + ["-DPIH_REAL=float", "-o", exe, "pih_rays_sanitize_main.cpp"], cwd=_DIR)
    return exe


def rays_of(L, task, rec, obj, rays, flags, cull=True):
    """records float64 [n, 8] of the rays float32 [n, 6] against one state record; task "peg" | "fly"; cull: with the bounding-sphere
    rejection of the kernels, or with every primitive function called"""
    rec = np.ascontiguousarray(rec, dtype=np.float64); rays = np.ascontiguousarray(rays, dtype=np.float32)
    assert rays.ndim == 2 and rays.shape[1] == _lib.RAY_WORDS
    out = np.full((len(rays), _lib.RAY_HIT_WORDS), np.nan)
    if task == "peg":
        assert rec.shape == (_lib.STATE_WORDS,)
        rc = L.pihray_view(rec.ctypes.data_as(_dp), rays.ctypes.data_as(_fp), len(rays), flags, int(cull), out.ctypes.data_as(_dp))
    else:
        assert rec.shape == (_lib.FLY_STATE_WORDS,)
        rc = L.pihray_fly(rec.ctypes.data_as(_dp), obj, rays.ctypes.data_as(_fp), len(rays), flags, int(cull), out.ctypes.data_as(_dp))
    assert rc == 0, rc
    return out


def trace(L, case, cull=True):
    """a case of tests/ray_cases.py -> records float64 [n, 8]"""
    return rays_of(L, case["task"], case["rec"], case["obj"], case["rays"], case["flags"], cull)
