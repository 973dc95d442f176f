"""Record tests/golden/scene_bits.npz: the calls of tests/scene_bits_cases.py on the library PIH_LIB_PATH names, on an MI355X.
The committed file was recorded on the build BEFORE the camera and ray kernels took their nearest-hit walk, normals and bounding spheres
from one definition per scene (its parent commit: float4 images of one host camera from pih_fly_render_kernel, the lit peg-in-hole
images from the written-out pih_lit_view_kernel); record again, on the build before the change, when a change is MEANT to alter a bit of
an image or a ray record.
usage: PIH_LIB_PATH=/path/to/libpih_hip.so python tests/golden/make_scene_bits_golden.py [OUT.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import scene_bits_cases as X  # noqa: E402

O.build()
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "scene_bits.npz")
images, records = X.run(torch, O)
got = X.pack(images, records)
np.savez_compressed(out, **got)
print("wrote %s: %d image digests, %d ray calls (%d records), %d bytes" % (out, len(got["image_keys"]), len(got["ray_keys"]), got["ray_words"].shape[1], os.path.getsize(out)))
