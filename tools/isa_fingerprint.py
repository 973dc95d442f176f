#!/usr/bin/env python3
"""Fingerprint of the gfx950 code of every kernel of the library (every csrc/*.hip of the tree), without a GPU: one line per kernel with a hash of its instruction
stream, the instruction count and the VGPR / AGPR / SGPR / LDS / scratch numbers of the code object metadata.  A refactor that leaves
the lines of the hot kernels unchanged leaves their speed unchanged (the step kernels sit at the 256-register limit).
That is the rule for the STEP kernels (pih_step_kernel, the four pih_fly_step_kernel instances: what bench.py times) and for every
kernel that is neither a camera nor a ray kernel: a refactor shows their lines unchanged, hash included.
The 13 camera kernels are not held by their hashes -- that rule made every camera feature write its scene's primitive list
again -- but by the contract the hash stood in for: their outputs are pinned bit for bit to a recording of the build
before (tests/test_gpu_scene_bits.py, tests/golden/scene_bits.npz) and their times are measured against that build on one box
(profiles/scene_share_bench.txt); the 4 ray kernels are held the same way, and as it happens their lines are the parent's too: that
measurement sent them back to their own walk (pih_rays.h).  For them the listing shows registers, LDS and scratch (none may appear), and which instances a change left instruction for
instruction alone.
Listings: profiles/scene_share_fingerprint.txt (one walk, one normal, one bounding sphere per scene), profiles/camera_refactor_fingerprint.txt
(one tile walk, one scene set-up per task).
usage: python tools/isa_fingerprint.py [SOURCE_TREE]    (default: this checkout; e.g. a `git worktree add` of another commit)"""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from peg_in_hole_gym_amd.csrc.build import FLAGS  # noqa: E402

META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def sources(tree):
    """the translation units of a tree: every csrc/*.hip it has (another commit's tree has its own set)"""
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(tree, "peg_in_hole_gym_amd", "csrc", "*.hip")))


def assembly(tree, name):
    src = os.path.join(tree, "peg_in_hole_gym_amd", "csrc", name)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["--offload-device-only", "-S", "-w", "-o", out, src],
                       check=True, cwd=os.path.dirname(src))
        return open(out).read()


def kernels(asm):
    """{symbol: [instruction lines]}: comments and directives dropped, basic-block labels without the function number"""
    funcs = set(re.findall(r"\.type\s+(\w+),@function", asm))
    body, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in funcs:
            cur = m.group(1); body[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";", 1)[0].strip()
        if s and not (s.startswith(".") and not s.startswith(".LBB")):
            body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return body


def metadata(asm):
    """{symbol: {key: value}} from the amdhsa.kernels list"""
    meta, cur = {}, {}
    for line in asm[asm.index("amdhsa.kernels:"):].splitlines():
        m = re.match(r"^  (?:- |  )\.(\w+):\s+(\S+)$", line)
        if line.startswith("  - "):
            cur = {}
        if m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    return meta


def main():
    tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
    meta, body = {}, {}
    for src in sources(tree):
        asm = assembly(tree, src)
        if "amdhsa.kernels:" in asm:      # (a translation unit of host code alone has none)
            meta.update(metadata(asm)); body.update(kernels(asm))
    print("%-16s %6s  %4s %4s %4s %6s %4s  %s" % ("sha256[:16]", "instr", "vgpr", "agpr", "sgpr", "lds", "scr", "kernel"))
    for name, ins in sorted(body.items()):
        md = meta.get(name, {})
        print("%-16s %6d  %4s %4s %4s %6s %4s  %s" % (hashlib.sha256("\n".join(ins).encode()).hexdigest()[:16], sum(not i.endswith(":") for i in ins),
                                                    *(md.get(k, "?") for k in META), name))


if __name__ == "__main__":
    main()
