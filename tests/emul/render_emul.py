"""Builder and ctypes binding of the TEST-ONLY host builds of the cameras' per-scene and per-pixel code: pih_fly_render_emul.cpp,
pih_fly_image_emul.cpp, pih_view_emul.cpp and pih_lit_emul.cpp compiled with g++ for the host, in double ("f64") and float ("f32"), with
the default CXXFLAGS of this directory's Makefile; and the numpy fronts of their render calls.  Everything is built into a directory the
caller names (a pytest tmp dir), nothing in-tree."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from peg_in_hole_gym_amd import _lib

_DIR = os.path.dirname(os.path.abspath(__file__))
CXX = os.environ.get("CXX", "g++")
CXXFLAGS = re.search(r"^CXXFLAGS \?= (.*)$", open(os.path.join(_DIR, "Makefile")).read(), re.M).group(1).split()
assert "-fno-fast-math" in CXXFLAGS and "-O2" in CXXFLAGS
_dp, _fp, _bp, _int = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_int
# source -> (symbol prefix, {function: argtypes})
SOURCES = {
    "fly_render": ("pihfr", dict(render=[_dp, _fp, _int, _int, _int, _int, _int, _dp])),
    "fly_image": ("pihfi", dict(render=[_dp, _fp, _int, _int, _int, _int, _int, C.c_void_p, C.c_void_p], pack_byte=[C.c_double], cam_degenerate=[_fp])),
    "view": ("pihv", dict(render=[_dp, _fp, _int, _int, _int, _int, _dp, _bp, _dp], pack_byte=[C.c_double])),
    "lit": ("pihl", dict(view_render=[_dp, _fp, _fp, _int, _int, _int, _int, _dp, _bp, _dp], fly_render=[_dp, _fp, _fp, _int, _int, _int, _int, _int, _dp, _bp, _dp],
                         pack_byte=[C.c_double], light_degenerate=[_fp, C.POINTER(C.c_char_p)])),
}


def lib(outdir, source, prec):
    """compiles tests/emul/pih_<source>_emul.cpp for `prec` into outdir -> the bound library"""
    prefix, functions = SOURCES[source]
    so = os.path.join(str(outdir), "libpih_%s_%s.so" % (source, prec))
    subprocess.check_call([CXX] + CXXFLAGS + ["-DPIH_REAL=" + {"f64": "double", "f32": "float"}[prec], "-shared", "-o", so, "pih_%s_emul.cpp" % source], cwd=_DIR)
    L = C.CDLL(so)
    for name, argtypes in functions.items():
        getattr(L, "%s_%s" % (prefix, name)).argtypes = argtypes
    assert getattr(L, prefix + "_real_bytes")() == (8 if prec == "f64" else 4)
    return L


def libs(outdir, source):
    return {prec: lib(outdir, source, prec) for prec in ("f64", "f32")}


def _words(rec, cam):
    rec = np.ascontiguousarray(rec, dtype=np.float64); cam = np.ascontiguousarray(cam, dtype=np.float32)
    assert cam.shape == (_lib.CAM_WORDS,)
    return rec, cam, rec.ctypes.data_as(_dp), cam.ctypes.data_as(_fp)


def _flags(shaded, frame):
    return (_lib.RENDER_SHADED if shaded else 0) | {"env": 0, "ee": _lib.RENDER_CAM_EE, "ee_pos": _lib.RENDER_CAM_EE_POS}[frame]


def fly_render(L, rec, cam, obj, W, H, shaded, frame, cull):
    """-> float4 image [H, W, 4] of the fly_render build"""
    rec, cam, prec, pcam = _words(rec, cam)
    out = np.zeros((H, W, 4))
    assert L.pihfr_render(prec, pcam, obj, W, H, _flags(shaded, frame), int(cull), out.ctypes.data_as(_dp)) == 0
    return out


def fly_image(L, rec, cam, obj, W, H, shaded, frame, cull):
    """-> (uint8 [H, W, 4] = r, g, b, seg; float64 [H, W] depth; code of the camera test) of the fly_image build"""
    rec, cam, prec, pcam = _words(rec, cam)
    rgba = np.full((H, W, 4), 0xA5, dtype=np.uint8); depth = np.full((H, W), np.nan)
    rc = L.pihfi_render(prec, pcam, obj, W, H, _flags(shaded, frame), int(cull), rgba.ctypes.data, depth.ctypes.data)
    assert rc >= 0
    return rgba, depth, rc


def cam_code(L, cam):
    cam = np.ascontiguousarray(cam, dtype=np.float32)
    return L.pihfi_cam_degenerate(cam.ctypes.data_as(_fp))


def view_render(L, rec, cam, W, H, shaded, frame, cull, expect=0):
    """-> (float4 image [H, W, 4], rgba8 image [H, W, 4] uint8, depth image [H, W]) of the view build"""
    rec, cam, prec, pcam = _words(rec, cam)
    assert rec.shape == (_lib.STATE_WORDS,)
    out = np.zeros((H, W, 4)); rgba = np.zeros((H, W, 4), dtype=np.uint8); depth = np.zeros((H, W))
    rc = L.pihv_render(prec, pcam, W, H, _flags(shaded, frame), int(cull), out.ctypes.data_as(_dp), rgba.ctypes.data_as(_bp), depth.ctypes.data_as(_dp))
    assert rc == expect
    return out, rgba, depth


def lit_render(L, case, light, lcull=True, expect=0, cam=None):
    """-> (float4 image [H, W, 4], rgba8 [H, W, 4] uint8, depth [H, W]) of the lit build for a case of tests/render_cases.py"""
    W, H = case["size"]
    rec, cam, prec, pcam = _words(case["rec"], case["cam"] if cam is None else cam)
    light = np.ascontiguousarray(light, dtype=np.float32)
    assert light.shape == (_lib.LIGHT_WORDS,)
    out = np.zeros((H, W, 4)); rgba = np.zeros((H, W, 4), dtype=np.uint8); depth = np.zeros((H, W))
    args = (W, H, case["flags"], int(lcull), out.ctypes.data_as(_dp), rgba.ctypes.data_as(_bp), depth.ctypes.data_as(_dp))
    if case["task"] == "peg":
        rc = L.pihl_view_render(prec, pcam, light.ctypes.data_as(_fp), *args)
    else:
        rc = L.pihl_fly_render(prec, pcam, light.ctypes.data_as(_fp), case["obj"], *args)
    assert rc == expect, rc
    return out, rgba, depth
