"""The cameras of a scene share one nearest-hit walk, one normal and one bounding sphere (pih_fly_render.h, pih_view.h); the ray tests walk
the same scenes.  Moving that code must not move a bit: the calls of tests/scene_bits_cases.py on this build against
tests/golden/scene_bits.npz, recorded on the build before the pieces were shared -- one SHA-256 per image and env, the ray records word
for word.  In that recording the float4 image of one host camera came from a kernel of its own (pih_fly_render_kernel); that
pih_fly_image_kernel<0> writes the same bytes is what let that kernel go.  (The ray kernels keep a walk of their own, pih_rays.h; their
records are held here all the same.)"""
import os

import numpy as np
import pytest

from tests import scene_bits_cases as X

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_bits.npz")


@pytest.fixture(scope="module")
def runs(oracle_mod):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    want_images, want_records = X.unpack(dict(np.load(GOLDEN)))
    images, records = X.run(torch, oracle_mod)
    return want_images, want_records, X.digests(images), records


def test_recording_covers_the_cases(runs):
    want_images, want_records, _, _ = runs
    keys = set(k.rsplit("/", 2)[0] for k in want_images)
    assert len(keys) == (2 * len(X.FLY_CAMERAS) + len(X.PEG_CAMERAS) + 1) * len(X.SIZES)
    outputs = set(k.split("/")[3] for k in want_images)
    assert len(outputs) == 13 and {"f4_flat", "f4_sub", "u8_devcam", "u8_lit_perenv"} <= outputs
    assert len(set(want_images.values())) > len(want_images) // 2                         # (not one image over and over)
    assert len(want_records) == 54 + 3 * 4 and all(np.isfinite(v).all() for k, v in want_records.items() if "-bad-" not in k)
    hits = np.concatenate([v[:, 1] for k, v in want_records.items() if "-aimed" in k])
    assert (hits != 255).mean() > 0.4


@pytest.mark.parametrize("task", ["fly0", "fly1", "peg"])
def test_images_bit_for_bit(runs, task):
    want, _, got, _ = runs
    mine = sorted(k for k in want if k.startswith(task + "/"))
    assert mine and sorted(k for k in got if k.startswith(task + "/")) == mine
    bad = [k for k in mine if got[k] != want[k]]
    assert not bad, "%d of %d images differ from the recording (task/camera/size/output/env): %s" % (len(bad), len(mine), ", ".join(bad[:12]))


@pytest.mark.parametrize("task", ["fly0", "fly1", "peg"])
def test_ray_records_bit_for_bit(runs, task):
    _, want, _, got = runs
    mine = sorted(k for k in got if k.startswith(task + "-"))
    assert sorted(k for k in want if k.startswith(task + "-")) == [k for k in mine if X.per_env_key(k) is None]
    for key in mine:
        shared = X.per_env_key(key)
        recorded = want[key] if shared is None else np.stack([want[k] for k in shared])
        diff = X.first_difference(recorded, got[key])
        assert diff is None, "ray records of %s [env, ray, word]: %s" % (key, diff)
