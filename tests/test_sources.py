"""The library's translation units: build.py's explicit list is every csrc/*.hip (tools/isa_fingerprint.py reads the same set from the
tree), and the C ABI's translation unit holds no kernel (no compile, no GPU)."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "peg_in_hole_gym_amd", "csrc")


def test_build_lists_every_translation_unit():
    from peg_in_hole_gym_amd.csrc import build
    on_disk = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(build.SRCS) == len(set(build.SRCS))
    assert sorted(os.path.normpath(p) for p in build.SRCS) == [os.path.normpath(p) for p in on_disk]


def test_c_abi_translation_unit_has_no_kernel():
    text = open(os.path.join(CSRC, "pih_hip.hip")).read()
    assert "__global__" not in text
