"""Inputs, comparison rules and tolerances of the camera tests, CPU and GPU: the free camera of the random-fly task (tests/test_fly_render.py,
tests/test_fly_image.py and their test_gpu_ siblings), the free camera of the peg-in-hole task (tests/test_peg_view.py,
tests/test_gpu_peg_view.py) and the lit images of both (tests/test_render_lit.py, tests/test_gpu_render_lit.py).  The reference they
compare against is tests/render_ref.py; the host builds of the product's per-pixel code are bound in tests/emul/render_emul.py.

Comparison rules of the packed formats of the random-fly camera (check_seg, depth_errors, colour_excess, Figures):
  class   seg 0..5 -> ARM, 6 -> OBJECT, 7 -> TABLE, 255 -> BG; against the reference's class: identical on every pixel in fp64, at most
          CLASS_SHARE of an image different in fp32 and on the GPU
  link    a pixel with seg = L < 6 and agreeing class: the reference's hit point eye + z_ref d / (d . f) lies on link L's capsule,
          |dist(point, segment L) - r_L| <= 1e-6 m; in fp32 / on the GPU the pixels where it does not count towards the same share
          (capsules overlap at the joints)
  depth   on class-agreeing pixels the depth-buffer value and the eye-space depth recovered from it; background exactly 1
  colour  on class-agreeing pixels excess = max(0, |byte - reference colour| - 0.5): what exceeds the unavoidable half step"""
import numpy as np

from peg_in_hole_gym_amd import _lib
from tests import render_ref as R
from tests.render_ref import ARM, BG, HOLE_POS, L_DIF, L_SHINE, L_SPEC, OBJECT, SEG_FINGER0, TABLE, macro, quat_matrix

SIZES = ((97, 61), (64, 64), (40, 30))          # (W, H): two tile columns, the second partial, rows no multiple of 16 | one tile column | narrower than a wave
IMAGE_SIZES = SIZES + ((5, 3),)                 # the packed formats: + narrower than a 16-byte vector, H W odd
OBJECTS = (0, 1)                                # Banana (5 spheres), Amicelli (2)
REST = np.array([0, -np.pi / 2, np.pi / 2, -np.pi / 2, -np.pi / 2, 0])
P0 = np.array([0.45, 0.1, 0.55])
HOLE_AXIS_EYE = 0.25                            # the close-up looks along the hole's axis (x) from this far
LINK_TOL = 1e-6                                 # [m]

# ------------------------------------------------------------------------------------------------ caps and tolerances
CLASS_SHARE = 0.003                             # share of an image's pixels that may differ in class (silhouette rays in fp32; tests/test_render.py)
UNDECIDED_CAP = 0.003
SHADOW_SHARE = 0.005
SHADED_P99, SHADED_MEDIAN = 0.05, 1e-3          # the project's bar for shaded colours (tests/test_render.py), grey levels

# Random-fly camera on the GPU.  The fp32 HOST build of the kernel's per-pixel code (tests/test_fly_render.py::test_host_build_matches_the_reference[f32],
# g++ -O2 -fno-fast-math, correctly rounded division and square root) differs from the fp64 reference over all scenes by at most the
# FLY_F32_HOST_* numbers below.  The library is built with -ffast-math and -fno-hip-fp32-correctly-rounded-divide-sqrt: its reciprocal square
# roots and divisions are 1-2 ulp each over a chain of about ten operations, so the GPU gets 8 x the host numbers.
#   * The relative error of the eye-space depth is recovered from the fp32 depth-buffer value 1 - near / z: one ulp of it (6e-8) is
#     6e-8 z / near of z, i.e. 6e-4 at the far plane z = 100 = 1e4 near -- the table next to the horizon sets the host number.
#   * Flat colours are products 255 x table entry: rounding of one fp32 multiplication.
#   * Shaded colours take the bar of tests/test_render.py (p99 < 0.05 and median < 1e-3 grey levels): normals at grazing hits differ in fp32
#     (host build: 8.2e-2 at the worst pixel).
FLY_F32_HOST_MAX_DEPTH_REL = 7.943e-04       # max |z - z_ref| / z_ref, fp32 host build vs fp64 reference
FLY_F32_HOST_MAX_DEPTH_VALUE = 2.026e-06     # max |depth-buffer value - reference's|
FLY_F32_HOST_MAX_FLAT_COLOUR = 5.493e-06     # max |rgb - rgb_ref| of the flat images, 0..255 scale
FLY_DEPTH_REL_TOL = 8 * FLY_F32_HOST_MAX_DEPTH_REL
FLY_DEPTH_VALUE_TOL = 8 * FLY_F32_HOST_MAX_DEPTH_VALUE
FLY_COLOUR_TOL = 8 * FLY_F32_HOST_MAX_FLAT_COLOUR

# Peg-in-hole free camera on the GPU, by the same rule (tests/test_peg_view.py::test_host_build_matches_the_reference[f32]).
#   * Depth: both host maxima come from rays that graze a capsule or the hole tube -- the root of a discriminant close to 0 carries the
#     square root of its rounding error: the overview (5.4e-4, 2.8e-6) and the hole close-up (4.7e-4, 2.6e-6) set them, the horizon has
#     2.0e-4, the wrist preset 5.2e-5, the eye-in-hand camera 1.5e-5.
#   * Flat colours are constants of the scene, no arithmetic: the host number is 0 and so is the bound.
#   * Shaded colours take the bar of tests/test_render.py (SHADED_P99, SHADED_MEDIAN): normals at grazing hits and at the edges of the
#     finger boxes differ in fp32 (host build: 3.4 at the worst pixel, p99 1.0e-3, median 1.1e-5).
PEG_F32_HOST_MAX_DEPTH_REL = 5.363e-04
PEG_F32_HOST_MAX_DEPTH_VALUE = 2.752e-06
PEG_F32_HOST_MAX_FLAT_COLOUR = 0.0
PEG_DEPTH_REL_TOL = 8 * PEG_F32_HOST_MAX_DEPTH_REL
PEG_DEPTH_VALUE_TOL = 8 * PEG_F32_HOST_MAX_DEPTH_VALUE
PEG_COLOUR_TOL = 8 * PEG_F32_HOST_MAX_FLAT_COLOUR

# Lit images: the bar for shaded colours times colour_factor(light).  The fp32 host build meets it with p99 <= 2.8e-3 and median <= 4.8e-6
# (light `low` / `shiny`); it is a bar on percentiles, and the GPU takes it as it stands.


# ------------------------------------------------------------------------------------------------ cameras
def fly_cameras(W, H):
    """name -> (13 camera words, frame)"""
    return {
        "overview": (list(_lib.FLY_CAM_DEFAULT), "env"),
        "close-up": (list(P0 + [0.25, 0.15, 0.2]) + list(P0) + [0, 0, 1, 60, 1, 0.01, 100], "env"),
        "horizon": ([1.6, 0, 0.5, 0, 0, 0.5, 0, 0, 1, 60, W / H, 0.01, 100], "env"),
        "eye-in-hand": ([0.05, 0, 0, 1.05, 0, 0, 0, 1, 0, 60, 1, 0.01, 100], "ee"),
    }


FLY_CAMERA_NAMES = ("overview", "close-up", "horizon", "eye-in-hand")


def peg_cameras(W, H):
    """name -> (13 camera words, frame)"""
    hx, hy, hz = HOLE_POS
    return {
        "wrist": (list(_lib.VIEW_CAM_WRIST), "ee_pos"),
        "overview": (list(_lib.VIEW_CAM_OVERVIEW), "env"),
        "hole close-up": ([hx + HOLE_AXIS_EYE, hy, hz, hx, hy, hz, 0, 0, 1, 15, 1, 0.01, 100], "env"),
        # forward along the tool axis (z of the grasp-target frame) from 2 cm behind the grasp target, between the pads: with closed fingers
        # the eye lies on the pad faces, with open ones (the scripted state) the pads frame the image.  (An eye 2 cm in FRONT of the grasp
        # target is under the table in the scripted state and sees nothing: replaced.)
        "eye-in-hand": ([0, 0, -0.02, 0, 0, 0.98, 1, 0, 0, 60, 1, 0.01, 100], "ee"),
        "horizon": ([1.6, 0, 0.5, 0, 0, 0.5, 0, 0, 1, 60, W / H, 0.01, 30], "env"),      # the table reaches the far plane
    }


PEG_CAMERA_NAMES = ("wrist", "overview", "hole close-up", "eye-in-hand", "horizon")
FRAME_FLAG = {"env": 0, "ee": _lib.RENDER_CAM_EE, "ee_pos": _lib.RENDER_CAM_EE_POS}

# the degenerate cameras of tests/test_gpu_fly_render.py::test_errors_and_untouched_paths and the field its message has to name
# (codes of fly::cam_degenerate: 1 eye / target, 2 up, 3 fov, 4 aspect, 5 near, 6 far)
DEGENERATE = ((dict(eye=list(_lib.FLY_CAM_DEFAULT[3:6])), 1), (dict(up=[1.6, 0.0, 1.0]), 2), (dict(up=[0.0, 0.0, 0.0]), 2), (dict(fov=0.0), 3), (dict(fov=180.0), 3),
              (dict(aspect=0.0), 4), (dict(aspect=-1.0), 4), (dict(near=0.0), 5), (dict(far=0.01), 6), (dict(far=0.005), 6))


def camera_with(**kw):
    c = list(_lib.FLY_CAM_DEFAULT)
    for k, v in kw.items():
        i = {"eye": 0, "target": 3, "up": 6, "fov": 9, "aspect": 10, "near": 11, "far": 12}[k]
        c[i:i + (3 if i < 9 else 1)] = v if i < 9 else [v]
    return c


# ------------------------------------------------------------------------------------------------ lights
_D = list(_lib.LIGHT_DEFAULT)
LIGHTS = {
    "default": _D,
    "low": [1.0, 0.3, 0.2] + _D[3:],                                    # 11 degrees above the table: long shadows
    "below": [-50.0, 30.0, -100.0] + _D[3:],                            # l.z < 0: the table occludes everything above it
    "shiny": _D[:3] + [1.0, 0.8, 0.6, 0.6, 0.35, 0.4, 32.0, 0.8],       # coloured, specular 0.4, shininess 32
}
LIGHT_NAMES = ("default", "low", "below", "shiny")
BAD_LIGHTS = (
    ("direction", 0, [0.0, 0.0, 0.0] + _D[3:]), ("direction", 1, _D[:1] + [float("inf")] + _D[2:]),
    ("colour", 4, _D[:4] + [-0.1] + _D[5:]), ("ambient", 6, _D[:6] + [-1.0] + _D[7:]), ("diffuse", 7, _D[:7] + [float("nan")] + _D[8:]),
    ("specular", 8, _D[:8] + [-0.5] + _D[9:]), ("shininess", 9, _D[:9] + [0.0] + _D[10:]), ("shadow factor", 10, _D[:10] + [1.5]), ("shadow factor", 10, _D[:10] + [-0.1]),
)


def colour_factor(light):
    """how much faster than the diffuse term the highlight moves with an error in the normal"""
    return 1.0 + light[L_SPEC] * light[L_SHINE] / light[L_DIF]


def probe_light(light, shadow):
    return list(light[:3]) + [1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 2.0, float(shadow)]


# ------------------------------------------------------------------------------------------------ states
def make_fly_states(O, obj, n, seed, eye_in_hand=False):
    """float32 [n, 48] records: q = REST + U(-0.6, 0.6) per joint, a random unit object quaternion, the object at P0 -- or, for the
    eye-in-hand camera, 0.35 m in front of the ee frame.  Rounded to float32 here, so every build and the reference see the same numbers."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, _lib.FLY_STATE_WORDS))
    for e in range(n):
        q = (REST + rng.uniform(-0.6, 0.6, 6)).astype(np.float32).astype(np.float64)
        oq = rng.normal(size=4); oq /= np.linalg.norm(oq)
        s[e, _lib.F_Q:_lib.F_Q + 6] = q; s[e, _lib.F_TARGET:_lib.F_TARGET + 6] = q
        s[e, _lib.F_OQUAT:_lib.F_OQUAT + 4] = oq
        pos = P0
        if eye_in_hand:
            p, qt = O.fk_ur5(q, 6)
            pos = p + quat_matrix(qt) @ np.array([0.35, 0.0, 0.0])
        s[e, _lib.F_OPOS:_lib.F_OPOS + 3] = pos
    return s.astype(np.float32)


def fly_handle(n, **kw):
    """a random-fly PihVecEnv with the settings of the camera tests (GPU)"""
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    kw.setdefault("max_episode_steps", 480); kw.setdefault("contact_margin", 0.02); kw.setdefault("dt", 1.0 / 120.0)
    return PihVecEnv(n, task_id=1, **kw)


# seeds of the six arm poses per (object, camera) of the GPU tests.  An eye-in-hand scene puts the object 0.35 m along the tool axis, which
# for some arm poses is under the table: such a scene shows no object and fails the conditions of fly_check_reference_scene (the
# Amicelli seeds 213 and 233 have one), so that pair takes the next seed whose six scenes meet them.
SCENE_SEED = {(obj, name): 200 + 10 * obj + ci for obj in OBJECTS for ci, name in enumerate(FLY_CAMERA_NAMES)}
SCENE_SEED[(1, "eye-in-hand")] = 253


def make_view_states(O):
    """float32 [6, 256] records from the oracle: the rest pose, three resets, a scripted episode after the fingers have closed (the eye of
    the wrist camera lies on the pad faces: the near-plane case of pih_render.h), 40 random-action steps.  Rounded to float32 here, so
    every build and the reference see the same numbers."""
    recs = [O.Oracle(1).get_state()[0]]
    for seed in (11, 12, 13):
        recs.append(O.Oracle(1, seed=seed).get_state()[0])
    o = O.Oracle(1, mode=1, dv=0.05, seed=4)
    for _ in range(1400):
        o.step(np.zeros((1, 4)))
        if o.get_state()[0, _lib.S_FSM] >= 4:
            break
    s = o.get_state()[0]
    assert s[_lib.S_FSM] >= 4 and max(s[_lib.S_QARM + 7], s[_lib.S_QARM + 8]) < 0.03, "the scripted episode has not closed the fingers"
    recs.append(s)
    o = O.Oracle(1, seed=21); rng = np.random.default_rng(5)
    for _ in range(40):
        o.step(rng.uniform(-1, 1, (1, 4)))
    recs.append(o.get_state()[0])
    out = np.zeros((len(recs), _lib.STATE_WORDS), dtype=np.float32)       # (the oracle's record is the physical state; the warm-start words stay 0)
    out[:, :O.STATE_WORDS] = np.array(recs)
    return out


# The cap on undecided pixels is a condition on the scene.  The two cameras that ride on the hand miss it in the two states that bring
# the hand down to the table: one pixel covers 0.4 mm of it there, a shadow edge moves by DELTA / l.z = 0.12 mm (default light) to 0.5 mm
# (low light) between the grown and the shrunk occluders, so most pixels ALONG an edge are undecided -- measured on the reference: wrist
# preset, scripted state 4: 0.0083 of the 64 x 64 image (default light); wrist, state 5 (40 random steps): 0.0092 (low light); eye-in-hand,
# state 5: 0.0066 (low light).  The cap stays; for these three pairs the scene changes: they take one of two further reset states, 6 and 7
# (largest share there: 0.0017).  Every other camera sees all six states.
PEG_STATE_FOR = {("wrist", 4): 6, ("wrist", 5): 7, ("eye-in-hand", 5): 7}


def make_peg_states(O):
    """float32 [8, 256]: the six states of make_view_states and two more resets (PEG_STATE_FOR)"""
    more = np.zeros((2, _lib.STATE_WORDS), dtype=np.float32)
    for i, seed in enumerate((14, 15)):
        more[i, :O.STATE_WORDS] = O.Oracle(1, seed=seed).get_state()[0]
    return np.concatenate([make_view_states(O), more])


# ------------------------------------------------------------------------------------------------ cases of the lit images
def peg_cases(O, peg_states, names=PEG_CAMERA_NAMES):
    """{key: case} of the peg-in-hole task: the six state slots x the cameras `names` x the three sizes.  case: task, rec, cam, frame, flags,
    size, obj, scene, name, env (the row of peg_states [8, 256] the slot takes, PEG_STATE_FOR)"""
    cases = {}
    scenes = {}
    for k in range(6):
        for name in names:
            env = PEG_STATE_FOR.get((name, k), k)
            if env not in scenes:
                scenes[env] = R.peg_scene(O, peg_states[env])
            for (W, H) in SIZES:
                cam, frame = peg_cameras(W, H)[name]
                cases[("peg", name, (W, H), k)] = dict(task="peg", rec=peg_states[env], cam=cam, frame=frame, flags=FRAME_FLAG[frame], size=(W, H), obj=None, scene=scenes[env],
                                                       name=name, env=env)
    return cases


def fly_cases(O, obj, name, recs):
    """{key: case} of the random-fly task: the states recs [k, 48] of object `obj` under camera `name` x the three sizes"""
    cases = {}
    for k, rec in enumerate(recs):
        scene = R.fly_scene(O, rec, obj)
        for (W, H) in SIZES:
            cam, frame = fly_cameras(W, H)[name]
            cases[("fly%d" % obj, name, (W, H), k)] = dict(task="fly", rec=rec, cam=cam, frame=frame, flags=FRAME_FLAG[frame], size=(W, H), obj=obj, scene=scene, name=name, env=k)
    return cases


def fly_host_states(O, obj, name):
    """the two arm poses per object and camera that the host builds see"""
    return make_fly_states(O, obj, 2, seed=100 + 10 * obj + FLY_CAMERA_NAMES.index(name), eye_in_hand=name == "eye-in-hand")


def make_cases(O):
    """all cases of the lit images: peg_cases of make_peg_states, and fly_cases of fly_host_states per object and camera"""
    cases = peg_cases(O, make_peg_states(O))
    for obj in OBJECTS:
        for name in FLY_CAMERA_NAMES:
            cases.update(fly_cases(O, obj, name, fly_host_states(O, obj, name)))
    return cases


def case_reference(case, light, light_exact=False):
    W, H = case["size"]
    return R.lit_reference(case["scene"], case["cam"], W, H, case["frame"], light, light_exact)


def fly_reference_scenes(O, sizes):
    """[(obj, camera name, (W, H), k, record, camera words, frame, scene, plain reference)]: fly_host_states of every object and camera at
    `sizes`, each reference checked by fly_check_reference_scene"""
    out = []
    for obj in OBJECTS:
        for name in FLY_CAMERA_NAMES:
            for k, rec in enumerate(fly_host_states(O, obj, name)):
                scene = R.fly_scene(O, rec, obj)
                for (W, H) in sizes:
                    cam, frame = fly_cameras(W, H)[name]
                    ref = R.plain_reference(scene, cam, W, H, frame)
                    fly_check_reference_scene(name, W, H, ref[2], obj)
                    out.append((obj, name, (W, H), k, rec, cam, frame, scene, ref))
    return out


def per_env_cases(O):
    """name -> dict(obj, states float32 [n, 48], cams float32 [n, 13], frame, size (W, H), checked envs, degenerate rows).  The GPU tests of
    PIH_RENDER_CAM_DEVICE render exactly these; test_per_env_cases_meet_the_caps_on_the_host puts every checked env through the fp32
    host build first."""
    W, H = 97, 61
    three = [np.array(fly_cameras(W, H)[k][0], dtype=np.float32) for k in ("overview", "close-up", "horizon")]
    cases = {"cycle": dict(obj=0, states=make_fly_states(O, 0, 70, seed=300), cams=np.stack([three[e % 3] for e in range(70)]), frame="env", size=(W, H),
                           checked=(0, 3, 4, 5, 6, 7, 63, 64, 69), degenerate=())}
    hand = np.tile(np.array(fly_cameras(64, 64)["eye-in-hand"][0], dtype=np.float32), (6, 1))
    hand[:, 9] = np.linspace(50.0, 70.0, 6)
    cases["eye-in-hand"] = dict(obj=0, states=make_fly_states(O, 0, 6, seed=SCENE_SEED[(0, "eye-in-hand")], eye_in_hand=True), cams=hand, frame="ee",
                                size=(64, 64), checked=tuple(range(6)), degenerate=())
    deg = np.stack([three[e % 3] for e in range(6)])
    deg[2, 0:3] = deg[2, 3:6]                   # eye == target
    deg[4, 9] = np.nan                          # fov = NaN
    cases["degenerate"] = dict(obj=1, states=make_fly_states(O, 1, 6, seed=SCENE_SEED[(1, "close-up")]), cams=deg, frame="env", size=(40, 30),
                               checked=(0, 1, 3, 5), degenerate=(2, 4))
    return cases


# ------------------------------------------------------------------------------------------------ rules: conditions on the reference
def fly_check_reference_scene(name, W, H, cls, obj):
    """What makes a scene worth comparing, asserted on the REFERENCE image.
    Eye-in-hand, 64 x 64: the object is 0.30 m in front of the eye, one pixel is 2 tan(30 deg) / 64 = 0.018 of the camera plane.  The Banana's
    five spheres cover 186 .. 251 pixels: at least 90.  The Amicelli's cover is two overlapping spheres of r = 21.9 mm: each a disc of
    pi (0.0219 / 0.30 / 0.018)^2 = 51 pixels, 61 .. 94 together depending on the direction its axis is seen from -- it cannot reach 90 in
    every pose; it has to show at least 40 pixels, the number the close-up asks of the object."""
    if name == "close-up" and (W, H) == (97, 61):
        assert (cls == TABLE).sum() >= 2000 and (cls == ARM).sum() >= 200 and (cls == OBJECT).sum() >= 40, [(cls == k).sum() for k in range(4)]
    if name == "eye-in-hand" and (W, H) == (64, 64):
        assert (cls == OBJECT).sum() >= (90 if obj == 0 else 40), (cls == OBJECT).sum()
    if name == "horizon":
        assert (cls == BG).mean() >= 0.25, (cls == BG).mean()


def peg_check_reference_scene(name, W, H, seg, cam):
    """What makes a scene worth comparing, asserted on the REFERENCE image"""
    owned = set(np.unique(seg).tolist())
    assert 5 not in owned, "link 5's sphere lies inside its neighbours' end spheres"
    if name == "overview":
        pipes = [s for s in owned if _lib.VIEW_SEG_PIPE0 <= s < _lib.VIEW_SEG_PIPE0 + 24]
        assert {0, 1, 2, 3, 4, 6} <= owned and (owned & {SEG_FINGER0, SEG_FINGER0 + 1}) and len(pipes) >= 3 and {_lib.VIEW_SEG_HOLE, _lib.VIEW_SEG_TABLE} <= owned, sorted(owned)
    if name == "hole close-up":
        # the eye is on the hole's axis: the rays that clear the far rim of the bore by a fifth of its radius look through it, at whatever
        # lies behind -- in some states the hand; background or table must be among it
        T = np.tan(np.radians(cam[9]) / 2)
        xc = (2 * (np.arange(W) + 0.5) / W - 1) * T * cam[10]; yc = (1 - 2 * (np.arange(H) + 0.5) / H) * T
        bore = np.hypot(xc[None, :], yc[:, None]) < 0.8 * float(macro("PIH_HOLE_RIN")) / (HOLE_AXIS_EYE + float(macro("PIH_HOLE_HALFLEN")))
        assert bore.sum() >= 4 and (seg[bore] != _lib.VIEW_SEG_HOLE).all() and np.isin(seg[bore], (_lib.VIEW_SEG_TABLE, _lib.SEG_NONE)).any(), seg[bore]
        assert (seg == _lib.VIEW_SEG_HOLE).sum() >= 20 * bore.sum() // 16, (seg == _lib.VIEW_SEG_HOLE).sum()
    if name == "eye-in-hand":
        assert any(s > 6 and s != _lib.SEG_NONE for s in owned), sorted(owned)
    if name == "horizon":
        assert {_lib.VIEW_SEG_TABLE, _lib.SEG_NONE} <= owned, sorted(owned)


# ------------------------------------------------------------------------------------------------ rules: an image against the reference
def linear_depth(depth_value, cam):
    near, far = [float(x) for x in np.asarray(cam, dtype=np.float32)[11:13]]
    return near * far / (far - np.asarray(depth_value, dtype=np.float64) * (far - near))


def compare(img, cls, ref_img, ref_cls, ref_z, cam, none, exact_class):
    """-> (max relative error of the eye-space depth, max absolute error of the depth-buffer value, array of absolute colour errors) over
    the pixels whose class agrees; asserts the class rule: identical everywhere (exact_class) or at most CLASS_SHARE of the image
    different.  cls: the image's classes -- its seg bytes (peg-in-hole) or R.classify of its flat image (random-fly); none: the class of a
    pixel that shows nothing (SEG_NONE, BG)"""
    same = cls == ref_cls
    if exact_class:
        assert same.all(), "%d pixels differ in class" % (~same).sum()
    else:
        assert (~same).mean() <= CLASS_SHARE, "%.4f of the pixels differ in class" % (~same).mean()
    hit = same & (ref_cls != none)
    assert (img[..., 0][same & (ref_cls == none)] == 1.0).all()
    z = linear_depth(img[..., 0], cam)
    zerr = (np.abs(z - ref_z)[hit] / ref_z[hit]).max() if hit.any() else 0.0
    derr = np.abs(img[..., 0] - ref_img[..., 0])[hit].max() if hit.any() else 0.0
    return zerr, derr, np.abs(img[..., 1:] - ref_img[..., 1:])[same].reshape(-1)


def link_failures(scene, seg, same, cam, frame, ref_z):
    """number of class-agreeing ARM pixels whose reference hit point does not lie on the capsule of the link the seg byte names"""
    H, W = seg.shape
    eye, d, df, _, _ = R.camera_rays(scene, cam, W, H, frame)
    same, seg, ref_z = same.reshape(-1), seg.reshape(-1), ref_z.reshape(-1)
    bad = 0
    for L in range(6):
        m = same & (seg == L)
        if not m.any():
            continue
        a, b, r = (scene.prims[L].p[k] for k in "abr")
        ph = eye + (ref_z[m] / df[m])[:, None] * d[m]
        q = np.clip(((ph - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
        dist = np.linalg.norm(ph - (a + q[:, None] * (b - a)), axis=-1)
        bad += int((np.abs(dist - r) > LINK_TOL).sum())
    return bad


def check_seg(scene, seg, cam, frame, ref, exact):
    """asserts the class and link rules on one random-fly image; -> mask of the class-agreeing pixels"""
    rflat, rlit, rcls, rz = ref
    same = R.class_of_seg("fly", seg) == rcls
    nlink = link_failures(scene, seg, same, cam, frame, rz)
    if exact:
        assert same.all() and nlink == 0, "%d pixels differ in class, %d name the wrong link" % ((~same).sum(), nlink)
    else:
        share = ((~same).sum() + nlink) / same.size
        assert share <= CLASS_SHARE, "%.4f of the pixels differ in class or link (%d class, %d link)" % (share, (~same).sum(), nlink)
    return same


def depth_errors(depth, same, ref, cam):
    """-> (max relative error of the eye-space depth, max absolute error of the depth-buffer value) over the class-agreeing hit pixels;
    asserts that the class-agreeing background is exactly 1"""
    rflat, rlit, rcls, rz = ref
    depth = np.asarray(depth, dtype=np.float64)
    assert np.isfinite(depth).all()
    assert (depth[same & (rcls == BG)] == 1.0).all()
    hit = same & (rcls != BG)
    if not hit.any():
        return 0.0, 0.0
    z = linear_depth(depth, cam)
    return (np.abs(z - rz)[hit] / rz[hit]).max(), np.abs(depth - rflat[..., 0])[hit].max()


def colour_excess(rgb, same, ref_img):
    """what |byte - reference colour| exceeds the half step by, over the class-agreeing pixels (flat array)"""
    return np.maximum(0.0, np.abs(rgb.astype(np.float64) - ref_img[..., 1:]) - 0.5)[same].reshape(-1)


class Figures:
    """running maxima / samples over many images of the random-fly camera; limits() asserts the fp32 / GPU caps"""
    def __init__(self):
        self.z = self.d = self.flat = 0.0; self.shaded = []

    def add_depth(self, zd):
        self.z = max(self.z, zd[0]); self.d = max(self.d, zd[1])

    def add_colour(self, excess, shaded):
        if shaded:
            self.shaded.append(excess)
        elif excess.size:
            self.flat = max(self.flat, excess.max())

    def text(self):
        sh = np.concatenate(self.shaded) if self.shaded else np.zeros(1)
        return ("max relative depth error %.3e (bound %.3e), depth-buffer value %.3e (%.3e), flat colour excess %.3e (%.3e), shaded colour excess p99 %.3e median %.3e max %.3e"
                % (self.z, FLY_DEPTH_REL_TOL, self.d, FLY_DEPTH_VALUE_TOL, self.flat, FLY_COLOUR_TOL, np.percentile(sh, 99), np.median(sh), sh.max()))

    def limits(self):
        assert self.z <= FLY_DEPTH_REL_TOL and self.d <= FLY_DEPTH_VALUE_TOL and self.flat <= FLY_COLOUR_TOL
        if self.shaded:
            sh = np.concatenate(self.shaded)
            assert np.percentile(sh, 99) < SHADED_P99 and np.median(sh) < SHADED_MEDIAN


def check_image(ref, task, render, light, exact):
    """The comparison rules of the lit images, for the host builds and the GPU.  render(light words) -> (float4 image [H, W, 4], seg bytes [H, W]).
    -> (colour errors on the compared pixels, share of pixels whose class differs).  Asserts the class rule and the shadow rule."""
    img, seg = render(light)
    img = np.asarray(img, dtype=np.float64)
    same = R.class_of_seg(task, seg) == ref["cls"]
    if exact:
        assert same.all(), "%d pixels differ in class" % (~same).sum()
    else:
        assert (~same).mean() <= CLASS_SHARE, "%.4f of the pixels differ in class" % (~same).mean()
    assert (img[..., 0][same & ~ref["hit"]] == 1.0).all()
    a, _ = render(probe_light(light, 0.5)); b, _ = render(probe_light(light, 1.0))
    state = (np.asarray(a)[..., 1:] != np.asarray(b)[..., 1:]).any(-1)
    use = same & ref["decided"]
    wrong = use & (state != ref["shadow"])
    if wrong.any():
        i, j = np.argwhere(wrong)[0]
        raise AssertionError("%d decided pixels have the wrong shadow state, the first at (%d, %d): seg %d, reference state %s with ndl %.3e, probe pixels %r and %r"
                             % (wrong.sum(), i, j, ref["seg"][i, j], ref["shadow"][i, j], ref["ndl"][i, j], np.asarray(a)[i, j].tolist(), np.asarray(b)[i, j].tolist()))
    return np.abs(img[..., 1:] - ref["img"][..., 1:])[use].reshape(-1), (~same).mean()
