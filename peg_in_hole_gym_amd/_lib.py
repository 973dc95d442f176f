"""ctypes binding of the C ABI in include/pih.h (libpih_hip.so).  There is no CPU fallback: if the HIP library is
missing or no GPU is present this module raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIH_LIB_PATH") or os.path.join(_HERE, "csrc", "libpih_hip.so")   # override: A/B of builds on one box

# sizes, fields, tasks and word offsets of include/pih.h, named as there minus "PIH_" (tests/test_abi_exports.py compares all of them with the header)
ABI_VERSION = 4
STATE_WORDS, DEBUG_WORDS, ACTION_DIM, OBS_DIM = 256, 1024, 4, 5
FLY_STATE_WORDS, FLY_ACTION_DIM, FLY_OBS_DIM = 48, 6, 6
CAM_WORDS = 13     # pih_render_cam: eye xyz, target xyz, up xyz, fov [deg, vertical], aspect, near, far
FLY_CAM_DEFAULT = (1.6, 0.0, 1.2, 0.0, 0.0, 0.2, 0.0, 0.0, 1.0, 60.0, 1.0, 0.01, 100.0)    # PIH_FLY_CAM_DEFAULT
RENDER_SHADED, RENDER_CAM_EE = 1, 2                # flags of pih_render_ex / pih_render_cam
RENDER_OUT_RGBA8, RENDER_OUT_DEPTH, RENDER_CAM_DEVICE = 4, 8, 16     # pih_render_cam: output format (at most one), per-env cameras in device memory
SEG_OBJECT, SEG_TABLE, SEG_NONE = 6, 7, 255        # seg byte of RENDER_OUT_RGBA8: UR5 links are 0 .. 5
# pih_render_view (peg-in-hole from any viewpoint): the frame flag of the reference's wrist camera, the seg bytes, the two preset cameras
RENDER_CAM_EE_POS = 32                             # eye and target offset by the grasp-target's position, axes env-local
VIEW_SEG_HOLE, VIEW_SEG_TABLE, VIEW_SEG_PIPE0 = 9, 10, 32     # arm links are 0 .. 6 (the hand is 6), fingers 7 and 8, pipe capsule s is VIEW_SEG_PIPE0 + s
VIEW_CAM_WRIST = (0.0, 0.0, 0.0, 0.0, 0.0, -10.0, 0.0, 1.0, 0.0, 60.0, 1.0, 0.001, 1000.0)     # PIH_VIEW_CAM_WRIST, with RENDER_CAM_EE_POS: PegInHole.render's camera
VIEW_CAM_OVERVIEW = (1.33, -0.02, 1.05, 0.05, -0.25, 0.3, 0.0, 0.0, 1.0, 40.0, 1.0, 0.01, 100.0)  # PIH_VIEW_CAM_OVERVIEW
# pih_render_lit (include/pih_render_light.h): both free cameras under a caller-given light, with a specular term and cast shadows
LIGHT_WORDS = 11   # direction xyz (towards the light, env-local), colour rgb, ambient, diffuse, specular, shininess, shadow factor (1 = no shadows)
LIGHT_DEFAULT = (-50.0, 30.0, 100.0, 1.0, 1.0, 1.0, 0.6, 0.35, 0.05, 2.0, 0.8)     # PIH_LIGHT_DEFAULT
RENDER_LIGHT_DEVICE = 64                           # the light argument is a device pointer float[env_count, LIGHT_WORDS], one light per env
# batched robot-model queries (include/pih_robot.h): link states, Jacobians, mass matrix, inverse dynamics
LINK_STATE_WORDS = 13   # pos xyz, quat xyzw, linear velocity of the frame origin, angular velocity
ROBOT_PANDA, ROBOT_UR5 = 0, 1                      # PIH_ROBOT_*: 9 DOF / 10 frames (9 = grasp-target), 6 DOF / 7 frames (6 = ee_link)
# batched ray tests (pih_ray_test of include/pih_robot.h): a ray is from xyz, to xyz; a record is hit fraction, seg, position xyz, normal xyz
RAY_WORDS, RAY_HIT_WORDS = 6, 8
# batched closest-point queries (pih_closest_points): a query is x, y, z, reach; a record is signed distance, seg, closest point xyz, normal xyz
POINT_WORDS, CLOSEST_WORDS = 4, 8
GROUP_ARM, GROUP_FINGERS, GROUP_OBJECT, GROUP_HOLE, GROUP_TABLE, GROUP_ALL = 1, 2, 4, 8, 16, 31    # PIH_GROUP_*: what a point is measured against
# robot clearance for many joint configurations (pih_robot_clearance): a record per probe is signed distance, obstacle seg, point on the probe xyz,
# point on the obstacle xyz, unit normal on the obstacle xyz, probe seg; the probes are 7 arm capsules + 4 hand spheres (Panda), 6 capsules (UR5)
CLEAR_WORDS, CLEAR_PROBES_PANDA, CLEAR_PROBES_UR5 = 12, 11, 6
CLEAR_GROUPS = GROUP_OBJECT | GROUP_TABLE          # what pih_robot_clearance measures against
GROUPS = {"arm": GROUP_ARM, "fingers": GROUP_FINGERS, "object": GROUP_OBJECT, "hole": GROUP_HOLE, "table": GROUP_TABLE}
RAY_FRAME_EE, RAY_SHARED, RAY_IGNORE_ROBOT = 1, 2, 4    # PIH_RAY_*: rays in the end-effector frame | one ray set for all envs | the arm is transparent
FIELD_STATE, FIELD_TIP_POSE, FIELD_CONTACT_FORCE, FIELD_DEBUG, FIELD_EE_POS = 0, 1, 2, 3, 4
TASK_PEG_IN_HOLE, TASK_RANDOM_FLY = 0, 1
# state record word offsets (PIH_S_*)
S_QARM, S_QDARM, S_POS, S_QUAT, S_VLIN, S_VANG, S_QJ, S_QDJ, S_TARGET = 0, 9, 18, 21, 25, 28, 31, 54, 77
S_FSM, S_FSMT, S_DONE, S_GRASP, S_RANDY, S_RNG_HI, S_RNG, S_STEPS, S_OFFSET = 86, 87, 88, 89, 90, 91, 92, 93, 94
S_SPARE, S_TIP, S_CFORCE, S_NCONTACT, S_PGS_ITERS, S_EE, S_GRASP_ANGLE, S_INVALID, S_ATTACH_QZ, S_SOLVER = 97, 98, 105, 106, 107, 108, 111, 112, 113, 114
S_CACHE_N, S_CACHE_KEY, S_CACHE_LAMBDA = 128, 129, 177
# random-fly record word offsets (PIH_F_*)
F_Q, F_QD, F_TARGET, F_OPOS, F_OQUAT, F_OVLIN, F_OVANG, F_DONE, F_STEPS, F_RNG, F_RNG_HI, F_OFFSET, F_SPARE, F_INVALID, F_EE, F_CFORCE, F_NCONTACT = \
    0, 6, 12, 18, 21, 25, 28, 31, 32, 33, 34, 35, 38, 39, 40, 43, 44
# debug buffer word offsets (PIH_DBG_*; the tables are in include/pih.h and DESIGN.md): peg-in-hole, random-fly, the timing words of both
DBG_UDOT, DBG_NCONTACT, DBG_PGS_ITERS, DBG_CONTACT, DBG_CONTACT_STRIDE, DBG_CONTACT_KEY, DBG_CONTACT_LAMBDA, DBG_DINV = 0, 38, 39, 40, 12, 10, 11, 640
DBG_FLY_UDOT, DBG_FLY_NCONTACT, DBG_FLY_PGS_ITERS, DBG_FLY_LIMIT_ROWS, DBG_FLY_CAND, DBG_FLY_CAND_STRIDE, DBG_FLY_LAMBDA = 0, 12, 13, 14, 16, 10, 200
DBG_CYCLES, DBG_T_START, DBG_T_END, DBG_HW_ID, DBG_XCC_ID = 900, 940, 943, 946, 947

EXPORTS = ["pih_default_config", "pih_abi_version", "pih_task_dims", "pih_object_name", "pih_create", "pih_destroy", "pih_reset", "pih_reseed", "pih_step", "pih_step_n",
           "pih_get_state", "pih_set_state", "pih_ik", "pih_ik_ur5", "pih_render", "pih_render_ex", "pih_render_cam", "pih_grasp_labels", "pih_timing", "pih_timing2", "pih_set_timing", "pih_last_error"]
LIGHT_EXPORTS = ["pih_render_lit"]      # what include/pih_render_light.h declares (tests/test_render_lit.py compares it with that header)
ROBOT_EXPORTS = ["pih_robot_dims", "pih_link_states_frames", "pih_robot_fk", "pih_robot_jacobian", "pih_robot_mass_matrix", "pih_robot_inverse_dynamics",
                 "pih_link_states", "pih_ray_test", "pih_closest_points", "pih_robot_clearance_probes", "pih_robot_clearance"]      # what include/pih_robot.h declares (tests/test_robot_query.py compares it with that header)
VIEW_EXPORTS = ["pih_render_view"]      # what include/pih_render_view.h declares on top of that (tests/test_peg_view.py compares it with that header)


class PihConfig(C.Structure):
    """struct pih_config (include/pih.h)"""
    _fields_ = [("n_envs", C.c_int32), ("env_index0", C.c_int32), ("mode", C.c_int32), ("solver_iters", C.c_int32),
                ("ik_iters", C.c_int32), ("max_episode_steps", C.c_int32), ("auto_reset", C.c_int32),
                ("enable_self_collision", C.c_int32), ("debug", C.c_int32), ("schedule", C.c_int32), ("enable_arm_collision", C.c_int32), ("task_id", C.c_int32), ("solver_path", C.c_int32), ("attach_ball", C.c_int32), ("exit_check_stride", C.c_int32), ("object_id", C.c_int32), ("seed", C.c_uint64),
                ("dt", C.c_float), ("residual_threshold", C.c_float), ("erp", C.c_float), ("warmstart", C.c_float),
                ("contact_margin", C.c_float), ("linear_slop", C.c_float), ("ik_damping", C.c_float), ("ik_residual", C.c_float),
                ("dv", C.c_float), ("reserved_f", C.c_float * 3)]


class PihError(RuntimeError):
    pass


_lib = None


def load():
    """Load libpih_hip.so; raises PihError if it has not been built (python peg_in_hole_gym_amd/csrc/build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PihError("HIP extension %s is missing: build it with `python peg_in_hole_gym_amd/csrc/build.py` "
                       "(there is no CPU fallback)" % LIB_PATH)
    # torch must be in the process BEFORE libpih_hip.so: both link libamdhip64, and the process has to end up with ONE HIP
    # runtime (the one torch ships) -- loaded the other way round, pih_create sees no device
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.pih_default_config.argtypes = [C.POINTER(PihConfig)]
    L.pih_default_config.restype = None
    L.pih_abi_version.restype = C.c_int
    L.pih_task_dims.argtypes = [C.c_int, C.POINTER(C.c_int32 * 3)]
    L.pih_object_name.argtypes = [C.c_int, C.c_int]
    L.pih_object_name.restype = C.c_char_p
    L.pih_create.argtypes = [C.POINTER(PihConfig), vp, C.POINTER(vp)]
    L.pih_destroy.argtypes = [vp]
    L.pih_reset.argtypes = [vp, vp, C.c_int, C.c_uint64, vp]
    L.pih_step.argtypes = [vp, vp, vp, vp, vp, vp]
    L.pih_step_n.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.pih_get_state.argtypes = [vp, C.c_int, vp, vp]
    L.pih_set_state.argtypes = [vp, C.c_int, vp, vp]
    L.pih_ik.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.pih_ik_ur5.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.pih_render.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.pih_render_ex.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.pih_render_cam.argtypes = [vp, vp, vp,      # (camera: a (c_float * CAM_WORDS) array, None, or with RENDER_CAM_DEVICE a device address)
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.pih_render_view.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]      # (camera: as pih_render_cam; None = the wrist preset)
    L.pih_render_lit.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]      # (camera as above; light: a (c_float * LIGHT_WORDS) array, None = LIGHT_DEFAULT, or with RENDER_LIGHT_DEVICE a device address)
    L.pih_robot_dims.argtypes = [C.c_int, C.POINTER(C.c_int32 * 2)]
    L.pih_link_states_frames.argtypes = [C.c_int]
    L.pih_robot_fk.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]                      # (h, robot, n, q, qd or None, out, stream)
    L.pih_robot_jacobian.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]       # (h, robot, n, q, frame, local_pos or None, out, stream)
    L.pih_robot_mass_matrix.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.pih_robot_inverse_dynamics.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.pih_link_states.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.pih_closest_points.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]      # (h, out, points, points_per_env, groups, env_begin, env_count, flags, stream)
    L.pih_robot_clearance_probes.argtypes = [C.c_int]
    L.pih_robot_clearance.argtypes = [vp, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, vp]      # (h, out, q or None, configs_per_env, reach, groups, env_begin, env_count, flags, stream)
    L.pih_ray_test.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]        # (h, out, rays, rays_per_env, env_begin, env_count, flags, stream)
    L.pih_grasp_labels.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.pih_reseed.argtypes = [vp, C.c_uint64]
    L.pih_timing.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.pih_timing2.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.pih_set_timing.argtypes = [vp, C.c_int]
    L.pih_last_error.argtypes = [vp]
    L.pih_last_error.restype = C.c_char_p
    if L.pih_abi_version() != ABI_VERSION:
        raise PihError("%s has ABI version %d, this package expects %d: rebuild it" % (LIB_PATH, L.pih_abi_version(), ABI_VERSION))
    _lib = L
    return L


def task_dims(task_id):
    """(action dim, obs dim, state words per env) of a task, from the library"""
    out = (C.c_int32 * 3)()
    if load().pih_task_dims(int(task_id), C.byref(out)) != 0:
        raise PihError("unknown task_id %r" % (task_id,))
    return int(out[0]), int(out[1]), int(out[2])


def robot_dims(robot):
    """(ndof, nframes) of a robot (ROBOT_PANDA / ROBOT_UR5), from the library"""
    out = (C.c_int32 * 2)()
    if load().pih_robot_dims(int(robot), C.byref(out)) != 0:
        raise PihError("unknown robot %r" % (robot,))
    return int(out[0]), int(out[1])


def link_states_frames(task_id):
    """frames per env of PihVecEnv.link_states for a task (peg-in-hole: 10 Panda frames + 24 pipe links; random-fly: 7 UR5 frames + the object)"""
    k = load().pih_link_states_frames(int(task_id))
    if k < 0:
        raise PihError("unknown task_id %r" % (task_id,))
    return k


def clearance_probes(task_id):
    """probes per configuration of PihVecEnv.robot_clearance for a task (peg-in-hole: 11, random-fly: 6)"""
    k = load().pih_robot_clearance_probes(int(task_id))
    if k < 0:
        raise PihError("unknown task_id %r" % (task_id,))
    return k


def object_names(task_id):
    """names of the objects compiled into the library for a task (random-fly: generated from the reference's asset files), index = object_id"""
    L = load(); out = []
    while True:
        n = L.pih_object_name(int(task_id), len(out))
        if n is None:
            return out
        out.append(n.decode())


def default_config(**kw):
    c = PihConfig()
    load().pih_default_config(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError("pih_config has no field %r" % k)
        setattr(c, k, v)
    return c
