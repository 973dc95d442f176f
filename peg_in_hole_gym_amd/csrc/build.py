"""Build libpih_hip.so (gfx950) in-tree with hipcc.  Used by __graft_entry__.build() and by developers."""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# One translation unit each, linked into one library: the C ABI first, then the kernels.  (Every csrc/*.hip: tests/test_sources.py.)
SRCS = [os.path.join(HERE, f) for f in ("pih_hip.hip", "pih_peg.hip", "pih_fly.hip", "pih_fly_image.hip", "pih_view.hip", "pih_lit.hip", "pih_robot.hip", "pih_rays.hip", "pih_dist.hip", "pih_clear.hip")]
SRC = SRCS[0]
OUT = os.path.join(HERE, "libpih_hip.so")
DEPS = SRCS + glob.glob(os.path.join(HERE, "*.h")) + glob.glob(os.path.join(HERE, "..", "..", "include", "*.h"))
# compiler flags of the device code (tools/isa_fingerprint.py compiles with the same ones)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-fno-slp-vectorize", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-ffast-math"]


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build(force=False, verbose=False):
    if not force and not needs_build():
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + FLAGS + ["-shared", "-o", OUT] + SRCS
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=HERE)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print("built", OUT)
