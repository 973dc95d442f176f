"""The calls behind tests/test_gpu_scene_bits.py and tests/golden/make_scene_bits_golden.py: every output of the camera and ray kernels
that walk a scene's primitives (fly::FlyScene, view::ViewScene), on small fixed inputs, so that a change which only MOVES that code can be
held to the bits of the build before it.

  random-fly   both objects, 6 envs of RC.make_fly_states; cameras `close-up` (env frame) and `eye-in-hand` at (97, 61) and (5, 3)
  peg-in-hole  the 8 states of RC.make_peg_states; render_view with the wrist preset, VIEW_CAM_OVERVIEW and the `eye-in-hand` camera of
               RC.peg_cameras at the same sizes; render() flat and shaded
  per camera   float4 flat and shaded, rgba8 shaded, depth, float4 + rgba8 with per-env device cameras (the camera's row, fov 50 .. 70
               degrees over the envs), the sub-range env_begin = 3, env_count = 2 of the float4 call; lit ("default", specular 0 with
               shadow factor 1, per-env lights: RC.LIGHTS in turn) in float4 and rgba8
  ray tests    every case of ray_cases.make_cases with shared rays (one env per call), the aimed and fan families again as per-env rays
               over all of a handle's envs (the same records, bit for bit), and ray_cases.bad_ray_block in both frames with
               ignore_robot on and off

run() -> (images, records).  The golden holds one SHA-256 per (image key, env) and the ray records themselves (pack / unpack)."""
import hashlib

import numpy as np

from peg_in_hole_gym_amd import _lib
from tests import ray_cases as RY
from tests import render_cases as RC

SIZES = ((97, 61), (5, 3))
FLY_CAMERAS = ("close-up", "eye-in-hand")
PEG_CAMERAS = ("wrist", "overview", "eye-in-hand")
SUB = (3, 2)                                    # env_begin, env_count of the sub-range call
_D = list(_lib.LIGHT_DEFAULT)
LIGHT_NO_SPECULAR_NO_SHADOW = _D[:8] + [0.0, _D[9], 1.0]


def _per_env(row, n):
    """[n, len(row)] float32: the row for every env, the fov (cameras) spread over 50 .. 70 degrees"""
    rows = np.tile(np.asarray(row, dtype=np.float32), (n, 1))
    rows[:, 9] = np.linspace(50.0, 70.0, n)
    return rows


def _lights(n):
    return np.array([RC.LIGHTS[RC.LIGHT_NAMES[e % len(RC.LIGHT_NAMES)]] for e in range(n)], dtype=np.float32)


def _camera_outputs(torch, n, draw, cam):
    """the outputs of one camera at one size: draw(**kw) is render / render_view with size and frame bound -> {output name: array [envs, ...]}"""
    dev = torch.tensor(_per_env(cam, n), device="cuda")
    out = {"f4_flat": draw(camera=cam), "f4_shaded": draw(camera=cam, shaded=True), "u8_shaded": draw(camera=cam, shaded=True, fmt="rgba8"),
           "depth": draw(camera=cam, fmt="depth"), "f4_devcam": draw(camera=dev), "u8_devcam": draw(camera=dev, fmt="rgba8"),
           "f4_sub": draw(camera=cam, env_begin=SUB[0], env_count=SUB[1])}
    for name, light in (("default", "default"), ("plain", LIGHT_NO_SPECULAR_NO_SHADOW), ("perenv", torch.tensor(_lights(n), device="cuda"))):
        out["f4_lit_" + name] = draw(camera=cam, light=light)
        out["u8_lit_" + name] = draw(camera=cam, light=light, fmt="rgba8")
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _ray_records(torch, g, cases, n_states, name):
    """shared-ray calls of `cases` (all of one handle, whose env k holds state k), the per-env calls of the aimed and fan families and
    the bad-ray block -> {key: float32 [.., R, 8]}"""
    rec = {}
    for c in cases:
        rec[RY.case_id(c)] = g.ray_test(torch.tensor(c["rays"]), frame=c["frame"], ignore_robot=c["ignore"], env_begin=c["state"], env_count=1).cpu().numpy()[0]
    for family, frame in (("aimed", "env"), ("fan", "ee")):
        for ignore in (False, True):
            rays = np.stack([c["rays"] for c in sorted((c for c in cases if c["name"] == family and c["ignore"] == ignore), key=lambda c: c["state"])])
            assert len(rays) == n_states
            rec["%s-perenv-%s%s" % (name, family, "-ignore" if ignore else "")] = g.ray_test(torch.tensor(rays), frame=frame, ignore_robot=ignore, env_count=n_states).cpu().numpy()
    bad, _ = RY.bad_ray_block()
    for frame in ("env", "ee"):
        for ignore in (False, True):
            rec["%s-bad-%s%s" % (name, frame, "-ignore" if ignore else "")] = g.ray_test(torch.tensor(bad), frame=frame, ignore_robot=ignore, env_count=n_states).cpu().numpy()
    return rec


def per_env_key(key):
    """the shared-ray keys, in env order, whose records a per-env call repeats -- or None"""
    if "-perenv-" not in key:
        return None
    name, family = key.split("-perenv-")
    n = 6 if name == "peg" else RY.FLY_STATES_PER_OBJECT
    family, ignore = (family[:-len("-ignore")], "-ignore") if family.endswith("-ignore") else (family, "")
    return ["%s-%d-%s%s" % (name, k, family, ignore) for k in range(n)]


def run(torch, O):
    """-> (images {"task/camera/WxH/output": array [envs, ...]}, records {key: float32 [.., R, 8]})"""
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    images, records = {}, {}
    ray_cases = RY.make_cases(O)
    for obj in RC.OBJECTS:
        n = 6
        g = RC.fly_handle(n, object_id=obj)
        for name in FLY_CAMERAS:
            g.set_state(torch.tensor(RC.make_fly_states(O, obj, n, seed=RC.SCENE_SEED[(obj, name)], eye_in_hand=name == "eye-in-hand")))
            for (W, H) in SIZES:
                cam, frame = RC.fly_cameras(W, H)[name]
                outs = _camera_outputs(torch, n, lambda **kw: g.render(W, H, ee_frame=frame == "ee", **kw), cam)
                images.update({"fly%d/%s/%dx%d/%s" % (obj, name, W, H, k): v for k, v in outs.items()})
        ns = RY.FLY_STATES_PER_OBJECT
        g.set_state(torch.tensor(np.tile(RC.make_fly_states(O, obj, ns, RY.FLY_SEED[obj]), (n // ns, 1))))
        records.update(_ray_records(torch, g, [c for c in ray_cases if c["task"] == "fly" and c["obj"] == obj], ns, "fly%d" % obj))
        g.close()
    states = RC.make_peg_states(O)
    n = len(states)
    g = PihVecEnv(n)
    g.set_state(torch.tensor(states))
    for name in PEG_CAMERAS:
        for (W, H) in SIZES:
            cam, frame = RC.peg_cameras(W, H)[name]
            outs = _camera_outputs(torch, n, lambda **kw: g.render_view(W, H, frame=frame, **kw), cam)
            images.update({"peg/%s/%dx%d/%s" % (name, W, H, k): v for k, v in outs.items()})
    for (W, H) in SIZES:
        images["peg/render/%dx%d/f4_flat" % (W, H)] = g.render(W, H).cpu().numpy()
        images["peg/render/%dx%d/f4_shaded" % (W, H)] = g.render(W, H, shaded=True).cpu().numpy()
    records.update(_ray_records(torch, g, [c for c in ray_cases if c["task"] == "peg"], 6, "peg"))      # (make_view_states: the first six of make_peg_states)
    g.close()
    return images, records


def digests(images):
    """{"key/env": SHA-256 of that env's image bytes}; the envs of a sub-range call carry their own numbers"""
    out = {}
    for key, a in images.items():
        first = SUB[0] if key.endswith("/f4_sub") else 0
        for e in range(len(a)):
            out["%s/env%d" % (key, first + e)] = hashlib.sha256(np.ascontiguousarray(a[e]).tobytes()).hexdigest()
    return out


def pack(images, records):
    """what the golden file holds: the digests' keys and bytes, the records of the shared-ray and bad-ray calls (a per-env call repeats
    the shared-ray records bit for bit: asserted here, on the build that is recorded, not stored)"""
    for key, a in records.items():
        shared = per_env_key(key)
        assert shared is None or _bits(a).tobytes() == _bits(np.stack([records[k] for k in shared])).tobytes(), key
    dg = digests(images)
    keys = sorted(dg)
    out = {"image_keys": np.array(keys), "image_sha256": np.array([list(bytes.fromhex(dg[k])) for k in keys], dtype=np.uint8)}
    # the records of all calls in one float32 array, word-major (rows of one record word compress far better than records do)
    rkeys = sorted(k for k in records if per_env_key(k) is None)
    out["ray_keys"] = np.array(rkeys)
    out["ray_shapes"] = np.array([(records[k].shape[0] if records[k].ndim == 3 else 0, records[k].shape[-2]) for k in rkeys], dtype=np.int32)
    out["ray_words"] = np.ascontiguousarray(np.concatenate([records[k].astype(np.float32).reshape(-1, _lib.RAY_HIT_WORDS) for k in rkeys]).T)
    return out


def unpack(golden):
    """-> (digests {"key/env": hex}, records {key: float32 array}) of a loaded golden file"""
    dg = {str(k): bytes(v.tolist()).hex() for k, v in zip(golden["image_keys"], golden["image_sha256"])}
    rows = np.ascontiguousarray(golden["ray_words"].T)
    records, at = {}, 0
    for key, (envs, R) in zip(golden["ray_keys"], golden["ray_shapes"]):
        n = max(int(envs), 1) * int(R)
        records[str(key)] = rows[at:at + n].reshape((int(envs), int(R), -1) if envs else (int(R), -1))
        at += n
    assert at == len(rows)
    return dg, records


def first_difference(a, b):
    """two float32 arrays of one shape, compared as bits -> None or a text that names the first place"""
    if a.shape != b.shape:
        return "shape %s against the recorded %s" % (b.shape, a.shape)
    bad = np.argwhere(_bits(a) != _bits(b))
    if not len(bad):
        return None
    i = tuple(bad[0])
    return "%d words differ, the first at %s: recorded %r, this build %r" % (len(bad), list(i), a[i], b[i])
