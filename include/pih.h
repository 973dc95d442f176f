/* pih.h -- C ABI of the MI355X-native vectorised peg-in-hole environment (libpih_hip.so).
 *
 * This is the drop-in boundary for the hot path of guodashun/peg-in-hole-gym: the per-env PyBullet calls the
 * reference makes from BaseEnv.step / PegInHole.* (paths relative to /root/reference/peg_in_hole_gym/):
 *
 *   pih_step      replaces  envs/base_env.py:60-75 (apply_action + stepSimulation + get_info for every agent), i.e.
 *                           p.stepSimulation (envs/base_env.py:64, envs/peg_in_hole.py:108),
 *                           p.calculateInverseKinematics + p.setJointMotorControlArray via panda_execute
 *                           (envs/utils.py:60-68), p.getLinkState (envs/utils.py:62, envs/peg_in_hole.py:58,115,123)
 *                           and the Python multiprocessing scatter/gather of envs/base_env_mp.py:40-51,75-87
 *   pih_reset     replaces  envs/base_env.py:84-94 + envs/peg_in_hole.py:227-274 (loadURDF/resetJointState scene build)
 *   pih_ik / pih_ik_ur5  replace  p.calculateInverseKinematics stand-alone for the Panda / UR5 chain
 *                           (envs/utils.py:67,79; envs/meta_env.py:92,104)
 *   pih_render    replaces  p.computeViewMatrix / computeProjectionMatrixFOV / getCameraImage of PegInHole.render
 *                           (envs/peg_in_hole.py:276-304) with an analytic ray caster over the primitive scene
 *   pih_render_cam replaces p.computeViewMatrix / computeProjectionMatrixFOV / getCameraImage for the 'random-fly' task (README.md:38; the
 *                           task class and with it its camera are not in the snapshot): a caller-given camera over the UR5's collision
 *                           capsules, the object's sphere cover and the table plane
 *   pih_render_view        the same three calls for the peg-in-hole task from ANY viewpoint: the scene of pih_render plus a stand-in arm,
 *                           with the packed output formats and per-env cameras of pih_render_cam
 *   pih_get_state replaces  p.getLinkState / p.getJointState / (north_star) getContactPoints normal force read-backs
 *
 * Conventions: every call returns 0 on success, <0 on error (pih_last_error gives the text).  All *_dev pointers
 * are DEVICE pointers owned by the caller (PyTorch-ROCm tensors); the library borrows them for the call and owns
 * only its internal per-env state.  Work is enqueued on the caller's HIP stream (`stream` = hipStream_t, 0 =
 * default stream) and is asynchronous.  One handle per device; a handle is not thread-safe; handles are independent.
 * There is NO CPU fallback: creation fails if no HIP device is present.
 */
#ifndef PIH_H
#define PIH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PIH_ABI_VERSION 4
#define PIH_STATE_WORDS 256   /* float words per env record: [0,128) physical state, [128,256) warm-start contact cache */
#define PIH_ACTION_DIM 4      /* envs/peg_in_hole.py:12 */
#define PIH_OBS_DIM 5         /* envs/peg_in_hole.py:13: finger1, finger2, ee x, y, z */
#define PIH_DEBUG_WORDS 1024

/* debug buffer word offsets (float32; PIH_FIELD_DEBUG, PIH_DEBUG_WORDS per env, written while config.debug != 0).  The two tasks lay
 * out the words below 900 differently; the timing words from 900 on (config.debug = 2, GPU only) are common. */
enum {
  /* peg-in-hole */
  PIH_DBG_UDOT = 0,            /* free acceleration per DOF (38) */
  PIH_DBG_NCONTACT = 38,
  PIH_DBG_PGS_ITERS = 39,
  PIH_DBG_CONTACT = 40,        /* + PIH_DBG_CONTACT_STRIDE c: contact c = link a, link b, point (3), normal (3), depth, mu, key, normal multiplier */
  PIH_DBG_CONTACT_STRIDE = 12,
  PIH_DBG_CONTACT_KEY = 10,    /* word of a contact record: warm-start key */
  PIH_DBG_CONTACT_LAMBDA = 11, /* word of a contact record: normal multiplier after the solve */
  PIH_DBG_DINV = 640,          /* + r: dinv of contact row r (3 rows per contact: n, t1, t2) */
  /* random-fly */
  PIH_DBG_FLY_UDOT = 0,        /* free acceleration per DOF (12: 6 joints + the object's twist) */
  PIH_DBG_FLY_NCONTACT = 12,
  PIH_DBG_FLY_PGS_ITERS = 13,
  PIH_DBG_FLY_LIMIT_ROWS = 14, /* 0: no joint-limit row; 1: limit rows of some joint from the start; 2: the solve was repeated with every limit row */
  PIH_DBG_FLY_CAND = 16,       /* + PIH_DBG_FLY_CAND_STRIDE k: contact candidate k = valid (0 / 1), link, point (3), normal (3), depth, compacted index */
  PIH_DBG_FLY_CAND_STRIDE = 10,
  PIH_DBG_FLY_LAMBDA = 200,    /* + c: normal multiplier of compacted contact c */
  /* both tasks, config.debug = 2 */
  PIH_DBG_CYCLES = 900,        /* + k: shader-clock cycles of phase k.  peg-in-hole: 0 fk, 1 controller rows, 2 collide, 3 aba, 4 rows, 5 pgs,
                                  6 integrate, 7 fk2, the sub-phase stamps 8, 9, 10, 15 of aba, and those of collide: 16 its entry, 17 constants,
                                  sample positions and the candidates of the sample tests, 18 slots of table, tube, attach, weld, arm spheres vs
                                  table, 19 slots of the pads, 20 of arm spheres vs pipe, 21 pairs (collide<W>, the nine-pass form: 17 samples +
                                  table + tube, 18 attach + weld + arm spheres vs table, 19 pads, 20 arm spheres vs pipe, 21 pairs); random-fly: 0 kinematics + candidates, 1 aba, 2 motor rows,
                                  3 contact rows, 4 IK targets, 5 pgs, 6 integrate */
  PIH_DBG_T_START = 940,       /* start of the env's wavefront on the chip-wide 100 MHz clock, as bits 0..15, 16..31, 32..47 (3) */
  PIH_DBG_T_END = 943,         /* its end, the same way (3).  random-fly writes 940 .. 947 on the wavefront's first env only */
  PIH_DBG_HW_ID = 946,         /* HW_ID register of the wavefront, low 16 bits */
  PIH_DBG_XCC_ID = 947
};

/* state record word offsets (float32) */
enum {
  PIH_S_QARM = 0, PIH_S_QDARM = 9, PIH_S_POS = 18, PIH_S_QUAT = 21, PIH_S_VLIN = 25, PIH_S_VANG = 28,
  PIH_S_QJ = 31, PIH_S_QDJ = 54, PIH_S_TARGET = 77,
  PIH_S_FSM = 86, PIH_S_FSMT = 87, PIH_S_DONE = 88, PIH_S_GRASP = 89, PIH_S_RANDY = 90,
  PIH_S_RNG_HI = 91,       /* draw counter of the env's RNG = RNG_HI * 2^24 + RNG (two exact fp32 integers: 2^48 draws) */
  PIH_S_RNG = 92, PIH_S_STEPS = 93, PIH_S_OFFSET = 94,
  PIH_S_SPARE = 97,        /* number of times this env was reset because its state became non-finite */
  PIH_S_TIP = 98,          /* peg-tip pose xyz + quat(xyzw) after the last step (7) */
  PIH_S_CFORCE = 105,      /* sum of contact normal impulses / dt of the last step [N] */
  PIH_S_NCONTACT = 106,
  PIH_S_PGS_ITERS = 107,   /* PGS iterations actually executed in the last step */
  PIH_S_EE = 108,          /* world position of the grasp-target frame (pybullet link 11) after the last step / reset (3) */
  PIH_S_GRASP_ANGLE = 111, /* scripted mode: atan2 of the rotated grasp offset when the state machine entered state 2 (envs/peg_in_hole.py:72) */
  PIH_S_ATTACH_QZ = 113,   /* scripted mode: z component of the grasped link's quaternion when the state machine entered state 4 (the
                              reference passes it as targetOrn[2] into childFrameOrientation, envs/peg_in_hole.py:101) */
  PIH_S_SOLVER = 114,      /* which PGS variant solved the last step: 0 DOF space, 1 / 2 row space without / with the limit rows of arm joints
                              0..6, 4 row space re-run with all limit rows and every motor row clamped, after an arm motor row clamped or the
                              verification of the residual-form motor rows failed (a pipe or arm motor multiplier came within 2^-7 of its
                              bound, or turned non-finite), 5 row space with two rows per lane (11..32 contacts).  Variants 1 and 2 run the
                              pipe motor rows (1: also arm motor rows 0..6) unclamped in residual form, unless schedule + 64 */
  PIH_S_INVALID = 112,     /* 1: the state became non-finite while auto_reset = 0; the env was re-initialised, marked done and stays frozen until pih_reset */
  PIH_S_CACHE_N = 128, PIH_S_CACHE_KEY = 129, PIH_S_CACHE_LAMBDA = 129 + 48
};

/* ---- 'random-fly' task (PIH_TASK_RANDOM_FLY; README.md:38, ur_execute envs/utils.py:70-82, banana.urdf): record of
 * PIH_FLY_STATE_WORDS float words per env.  Inside the library the fly state is structure-of-arrays [word][env] (one env per
 * lane, coalesced loads); pih_get_state / pih_set_state(PIH_FIELD_STATE) exchange it env-major, float[n, PIH_FLY_STATE_WORDS]. */
#define PIH_FLY_STATE_WORDS 48
#define PIH_FLY_ACTION_DIM 6   /* ee target xyz (world) + euler rpy, envs/utils.py:71-72 */
#define PIH_FLY_OBS_DIM 6      /* ee xyz + object xyz (world); build-defined, SURVEY.md 8d */
enum {
  PIH_F_Q = 0, PIH_F_QD = 6, PIH_F_TARGET = 12,                       /* UR5 joints 1..6 (envs/utils.py:46,82), their rates, IK targets */
  PIH_F_OPOS = 18, PIH_F_OQUAT = 21, PIH_F_OVLIN = 25, PIH_F_OVANG = 28,   /* object pose (env-local) and twist */
  PIH_F_DONE = 31, PIH_F_STEPS = 32, PIH_F_RNG = 33, PIH_F_RNG_HI = 34, PIH_F_OFFSET = 35, PIH_F_SPARE = 38, PIH_F_INVALID = 39,
  PIH_F_EE = 40,          /* world position of ee_link after the last step / reset (3) */
  PIH_F_CFORCE = 43,      /* sum of contact normal impulses / dt of the last step [N] */
  PIH_F_NCONTACT = 44
};

/* pih_get_state / pih_set_state fields */
enum {
  PIH_FIELD_STATE = 0,         /* float[n, PIH_STATE_WORDS] (random-fly: float[n, PIH_FLY_STATE_WORDS]) */
  PIH_FIELD_TIP_POSE = 1,      /* float[n, 7]  (get only)  envs/peg_in_hole.py:58,115 */
  PIH_FIELD_CONTACT_FORCE = 2, /* float[n]     (get only)  north_star contact-normal force */
  PIH_FIELD_DEBUG = 3,         /* float[n, PIH_DEBUG_WORDS] (get only; filled when config.debug != 0) */
  PIH_FIELD_EE_POS = 4         /* float[n, 3]  (get only)  envs/utils.py:62 getLinkState(panda, 11)[0] */
};

/* tasks (the reference's TASK_LIST registry, envs/base_env.py:9-11; README.md:38 names 'random-fly') */
enum {
  PIH_TASK_PEG_IN_HOLE = 0,   /* Panda + 25-link pipe + hole tube + table (envs/peg_in_hole.py) */
  PIH_TASK_RANDOM_FLY = 1     /* UR5 + one free-flying object (README.md:38; ur_execute, envs/utils.py:70-82); see pih_fly.h */
};

typedef struct pih_config {
  int32_t n_envs;             /* envs on THIS device (mp_num * sub_num / world_size) */
  int32_t env_index0;         /* global index of this device's first env (block partition; seeds = seed+1000+global index) */
  int32_t mode;               /* 0 = action mode (panda_execute, envs/utils.py:60-68); 1 = scripted episode (envs/peg_in_hole.py:53-112) */
  int32_t solver_iters;       /* 50 */
  int32_t ik_iters;           /* 20 */
  int32_t max_episode_steps;  /* action mode: done after this many steps (2227) */
  int32_t auto_reset;         /* 1: finished envs are reset inside pih_step */
  int32_t enable_self_collision;
  int32_t debug;              /* 1: fill the debug buffer each step; roctx ranges "pih_step(...)" / "pih_reset" around the launches (when a roctx library is loadable) */
  int32_t schedule;           /* 1 (default): longest-job-first dispatch order from the previous step's contact counts; 0: block i = env i;
                                 +4: do not raise the issue priority of the wavefronts of contact-heavy envs (measurement switch);
                                 +8: no fused launch -- peg-in-hole: the two-launch step of rounds 1-3 (pih_pre_kernel: dispatch order +
                                 controller one env per lane, then the physics launch; the step a hipGraph can capture); random-fly: the IK
                                 inside the step wavefront;
                                 +32 (random-fly): one env per LANE in the step wavefronts (default: one env per QUAD of lanes, 16 envs per
                                 wavefront, the PGS sweep split over the quad; fused with the IK controller wavefronts while all workgroups
                                 are resident together, n <= 13 104 on 256 CUs); +64 (random-fly): every joint-limit row in every sweep
                                 (default: limit rows of joints farther than 0.25 rad from their limits are skipped and verified -- same
                                 results bit for bit); +64 (peg-in-hole): no residual-form motor rows in the one-row-per-lane PGS, every
                                 motor row is clamped in every sweep (default: the pipe motor rows and, without limit rows, arm motor rows
                                 0..6 run unclamped and are verified after the solve -- the same solve in another rounding, a failed
                                 verification re-runs it clamped: PIH_S_SOLVER = 4) (measurement switches).
                                 pih_create rejects every other value (-2), among them the retired 2 / 3 and + 16 */
  int32_t enable_arm_collision; /* arm collision spheres (pih_model.h PIH_ARM_SPH_*): bit 0 vs the table plane, bit 1 vs the pipe (hand /
                                   flange / wrist spheres against the pipe's sample spheres); default 3 */
  int32_t task_id;            /* PIH_TASK_*: which task of TASK_LIST (envs/base_env.py:9-11) the handle simulates */
  int32_t solver_path;        /* 0 (default): row-space PGS -- one row per lane for <= 10 contacts, two rows per lane for 11..32 -- and the DOF-space
                                 PGS beyond; 1: DOF-space PGS for every env (A/B runs and tests; same row sequence, results equal to rounding) */
  int32_t attach_ball;        /* p7 attach (createConstraint, envs/peg_in_hole.py:99-104): 0 (default) = 6-row weld honouring childFrameOrientation,
                                 1 = 3-row ball joint between the grasp point and the grasp-target origin (round-1 behaviour) */
  int32_t exit_check_stride;  /* cadence of the PGS early-exit test (Bullet: largest squared row residual <= residual_threshold, evaluated after
                                 EVERY iteration).  1 = Bullet's cadence; s > 1 = the test runs in iterations 1..4, then in iterations 4 + s k and in
                                 the last one (an env that meets the threshold between two tests runs at most s - 1 further iterations, each of
                                 whose row updates is below the threshold).  Both tasks.  Default 16; the oracle has the same switch, tests/test_gpu_defaults.py
                                 bounds the difference against Bullet's cadence; bench.py reports the value it ran with */
  int32_t object_id;          /* random-fly: which free-flying object (index into PIH_FLY_OBJ_NAMES of include/pih_model.h, generated from the
                                 reference's asset files; args[0] of README.md:38): 0 'Banana', 1 'Amicelli' */
  uint64_t seed;
  float dt;                   /* 1/240 */
  float residual_threshold;   /* 1e-7 */
  float erp;                  /* 0.2 */
  float warmstart;            /* 0.85 */
  float contact_margin;       /* 0.005 */
  float linear_slop;          /* 1e-5 */
  float ik_damping;           /* 0.5 */
  float ik_residual;          /* 1e-4 */
  float dv;                   /* 2/240 (action mode) or 0.05 (scripted) */
  float reserved_f[3];
} pih_config;

typedef struct pih_handle pih_handle;

void pih_default_config(pih_config* cfg);
int pih_abi_version(void);
/* per-task sizes of the tensors the caller owns: out[0] = action dim, out[1] = obs dim, out[2] = state words per env */
int pih_task_dims(int task_id, int32_t out[3]);
/* name of object `object_id` of a task (random-fly: the free-flying objects compiled in from envs/assets/urdf), NULL past the end */
const char* pih_object_name(int task_id, int object_id);
/* offsets_host: HOST float[n_envs,3] (envs/base_env.py:35-55 placement) or NULL for zeros */
int pih_create(const pih_config* cfg, const float* offsets_host, pih_handle** out);
int pih_destroy(pih_handle* h);
/* mask_dev: uint8[n] (nonzero = reset that env) or NULL = all.
 * hard != 0 = resetSimulation + reload (envs/base_env.py:85-86, envs/peg_in_hole.py:227-274): like the reference, a hard reset draws a
 *   NEW scene -- every env keeps advancing its own RNG draw sequence (the reference keeps drawing from the global `random`); it only also
 *   clears the env's non-finite-reset count and invalid flag.
 * seed != 0: explicit replay -- the handle's base seed becomes `seed` (env seed = seed + 1000 + global env index) and every env
 *   restarts its draw sequence from its beginning; needs mask_dev = NULL (returns -2 otherwise: an unmasked env would keep its draw
 *   counter on another seed's stream).  seed == 0: keep the seed and continue the sequence.
 * (The reference never seeds: envs/peg_in_hole.py:239-267 use the global `random`.) */
int pih_reset(pih_handle* h, const uint8_t* mask_dev, int hard, uint64_t seed, void* stream);
/* new base seed for all later resets; the NEXT pih_reset call restarts every env's draw sequence from its beginning (same as passing
 * `seed` to that call: it must reset all envs, mask_dev = NULL, and returns -2 otherwise) */
int pih_reseed(pih_handle* h, uint64_t seed);
/* actions_dev float[n,4]; obs_dev float[n,5]; reward_dev float[n]; done_dev uint8[n]
 * (PIH_TASK_RANDOM_FLY: actions float[n,6], obs float[n,6]).
 * peg-in-hole: ONE kernel launch (controller wavefronts + env wavefronts; pih_config.schedule + 8: the two launches of rounds 1-3).
 * Returns -5 (and keeps returning it) if in an earlier step of this handle an env wavefront timed out waiting for its controller wavefront. */
int pih_step(pih_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);
/* k consecutive steps with the same action buffer (scripted mode ignores actions: may be NULL) in one call */
int pih_step_n(pih_handle* h, int k, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);
int pih_get_state(pih_handle* h, int field, void* out_dev, void* stream);
int pih_set_state(pih_handle* h, int field, const void* in_dev, void* stream);
/* stand-alone batched IK: q0 float[n,9], tpos float[n,3], tquat float[n,4] (xyzw) -> qout float[n,9] */
int pih_ik(pih_handle* h, int n, const float* q0_dev, const float* tpos_dev, const float* tquat_dev, float* qout_dev, void* stream);
/* the same for the UR5 chain of envs/assets/urdf/ur5.urdf (ur_execute, envs/utils.py:70-82): q0/qout float[n,6] */
int pih_ik_ur5(pih_handle* h, int n, const float* q0_dev, const float* tpos_dev, const float* tquat_dev, float* qout_dev, void* stream);
/* wrist camera of PegInHole.render (envs/peg_in_hole.py:276-304; eye = link 11, looking straight down, fov 60, near 0.001,
 * far 1000; the reference uses 300 x 300): out_dev float[env_count, height, width, 4] = (OpenGL depth-buffer value, r, g, b)
 * for envs env_begin .. env_begin+env_count-1, from the CURRENT state.  RGB is a flat value per object (table 153, pipe and
 * hole 232, fingers 77, background 255, the reference's uint8 scale), unshaded; pih_render_ex adds TinyRenderer's ambient + diffuse
 * terms.  out_dev must be 16-byte aligned. */
int pih_render(pih_handle* h, float* out_dev, int width, int height, int env_begin, int env_count, void* stream);
/* the same with options: flags = PIH_RENDER_SHADED multiplies the per-object RGB value by ambient + diffuse x max(0, n . l) of
 * TinyRenderer's default light (getCameraImage without light arguments; specular term and shadow map not reproduced); any other bit,
 * the output formats of pih_render_cam included, returns -2: the wrist camera has the one format */
#define PIH_RENDER_SHADED 1
int pih_render_ex(pih_handle* h, float* out_dev, int width, int height, int env_begin, int env_count, int flags, void* stream);
/* free camera of the 'random-fly' task (fly handles only; a peg-in-hole handle gets -2, and pih_render / pih_render_ex keep rejecting fly
 * handles).  The camera is given as p.computeViewMatrix (eye, target, up) and p.computeProjectionMatrixFOV (fov, aspect, near, far) take
 * it, the image comes back as p.getCameraImage's (envs/peg_in_hole.py:276-304): out_dev float[env_count, height, width, 4] = (OpenGL
 * depth-buffer value, r, g, b), row 0 on top, from the CURRENT state, 16-byte aligned, env_count <= 65535.  Scene: the six UR5 collision
 * capsules (255 x PIH_UR5_RGB), the object's sphere cover (255 x PIH_FLY_OBJ_RGB), the table plane (153), background 255 at depth 1; a hit
 * outside [near, far] is clipped.  flags: PIH_RENDER_SHADED as in pih_render_ex (same light, ambient and diffuse terms);
 * PIH_RENDER_CAM_EE = eye, target and up are given in the ee_link frame of each env's UR5 (eye-in-hand) instead of the env-local frame
 * (the env's offset does not enter either way).  cam: HOST float[PIH_CAM_WORDS], read during the call, one camera for all envs of
 * the call; NULL = PIH_FLY_CAM_DEFAULT.  A degenerate camera (eye == target, up parallel to the view axis, fov outside (0, 180),
 * aspect <= 0, near <= 0, far <= near) returns -2 and pih_last_error names the field.
 * Output formats (at most one; both: -2; none: the float4 image above; out_dev is 16-byte aligned for each, any width, height >= 1):
 *   PIH_RENDER_OUT_RGBA8  out_dev uint8[env_count, height, width, 4] = (r, g, b, seg): the r, g, b of the float4 image (flat or
 *                         PIH_RENDER_SHADED) as bytes min(255, (int)(v + 0.5f)) -- rounded half up, the arm's flat 178.5 is 179 -- and
 *                         the segmentation value of what the ray hit: the link index 0 .. 5, PIH_SEG_OBJECT, PIH_SEG_TABLE, PIH_SEG_NONE
 *   PIH_RENDER_OUT_DEPTH  out_dev float[env_count, height, width]: the depth-buffer value alone (PIH_RENDER_SHADED has no effect)
 * PIH_RENDER_CAM_DEVICE: the camera argument is a DEVICE pointer float[env_count, PIH_CAM_WORDS], row e = the camera of env
 * env_begin + e, read by the kernel (no host copy, no synchronisation); NULL: -2.  Combines with PIH_RENDER_CAM_EE and every format.
 * The host cannot see these cameras, so the kernel applies the same test per env: an env whose camera is degenerate (or holds a NaN)
 * gets the background image -- depth 1, rgb 255, seg PIH_SEG_NONE -- and the call returns 0. */
#define PIH_CAM_WORDS 13        /* eye xyz, target xyz, up xyz, fov [deg, vertical], aspect, near, far */
#define PIH_FLY_CAM_DEFAULT {1.6f, 0.f, 1.2f,  0.f, 0.f, 0.2f,  0.f, 0.f, 1.f,  60.f, 1.f, 0.01f, 100.f}
#define PIH_RENDER_CAM_EE 2     /* camera given in the ee_link frame of each env's UR5 (eye-in-hand) instead of the env-local frame */
#define PIH_RENDER_OUT_RGBA8 4  /* out_dev is uint8[env_count, height, width, 4] = (r, g, b, seg) */
#define PIH_RENDER_OUT_DEPTH 8  /* out_dev is float[env_count, height, width] = the depth-buffer value */
#define PIH_RENDER_CAM_DEVICE 16 /* the camera argument is a device pointer float[env_count, PIH_CAM_WORDS], one camera per env */
#define PIH_SEG_OBJECT 6        /* seg byte of PIH_RENDER_OUT_RGBA8: links are 0 .. 5 (PIH_SEG_OBJECT = PIH_UR5_NJ), then the object, */
#define PIH_SEG_TABLE 7         /* the table */
#define PIH_SEG_NONE 255        /* and nothing (background) */
int pih_render_cam(pih_handle* h, float* out_dev, const float* cam /* [PIH_CAM_WORDS] on the host, NULL = default; PIH_RENDER_CAM_DEVICE: [env_count][PIH_CAM_WORDS] on the device */,
                   int width, int height, int env_begin, int env_count, int flags, void* stream);
/* free camera of the peg-in-hole task -- the scene of pih_render plus a stand-in arm from any viewpoint, with the output formats and the
 * per-env cameras above: declared in pih_render_view.h, which the end of this header includes */
/* grasp-rectangle label images of random_grasp (envs/peg_in_hole.py:72-99,116) from the angle each env recorded when its
 * state machine entered state 2 (PIH_S_GRASP_ANGLE): out_dev float[env_count, 4, size, size] = pos (50 inside the rectangle),
 * sin(2 angle), cos(2 angle), width in pixels; meta_dev (may be NULL) float[env_count, 5] = x, y, angle [deg], width, length.
 * The reference rasterises with skimage.draw.polygon (absent here: parity unpinned); restated as its even-odd crossing test. */
int pih_grasp_labels(pih_handle* h, float* out_dev, float* meta_dev, int size, int env_begin, int env_count, void* stream);
/* kernel timing with HIP events on the launch stream: average ms per step since the last call with reset=1.  pih_timing2 splits it
 * at the event recorded right before the step kernel's launch: step_ms is the step kernel; pre_ms is the kernel before it (controller +
 * dispatch order) in the two-launch peg-in-hole step (schedule + 8), and under the fused launch -- where no such kernel runs and the
 * controller is part of the step kernel -- only the gap between two event records, close to 0 */
int pih_timing(pih_handle* h, int reset, double* avg_ms_out, int64_t* launches_out);
int pih_timing2(pih_handle* h, int reset, double* pre_ms_out, double* step_ms_out, int64_t* launches_out);
/* enable = 0: off; 1: every step launch is bracketed by events; k > 1: every k-th launch only.  (Three hipEventRecord per step drain
 * the queue between the two kernels of a step: +30 us on a 430 us step measured on the MI355X -- a throughput measurement that also
 * wants kernel times samples them.) */
int pih_set_timing(pih_handle* h, int enable);
const char* pih_last_error(pih_handle* h);

#ifdef __cplusplus
}
#endif
#include "pih_render_view.h"
/* words of a light of the lit image call declared in pih_render_light.h (direction xyz, colour rgb, ambient, diffuse, specular, shininess, shadow factor).
 * Defined here and not there because tests/test_abi_exports.py compares every *_WORDS name of _lib.py with THIS file */
#define PIH_LIGHT_WORDS 11
#include "pih_render_light.h"
/* words of a link state of the robot-model queries declared in pih_robot.h: pos (3), quat xyzw (4), linear velocity of the frame origin (3),
 * angular velocity (3).  Defined here for the same reason */
#define PIH_LINK_STATE_WORDS 13
/* words of a ray (from xyz, to xyz) and of a ray's record (hit fraction, seg, hit position xyz, normal xyz) of the batched ray test declared
 * in pih_robot.h.  Defined here for the same reason */
#define PIH_RAY_WORDS 6
#define PIH_RAY_HIT_WORDS 8
/* words of a closest-point query (x, y, z, reach [m]) and of its record (signed distance, seg, closest point xyz, outward unit normal xyz) of
 * pih_closest_points, declared in pih_robot.h.  Defined here for the same reason */
#define PIH_POINT_WORDS 4
#define PIH_CLOSEST_WORDS 8
/* words of a probe's record of pih_robot_clearance, declared in pih_robot.h (signed distance, obstacle seg, point on the probe xyz, point on
 * the obstacle xyz, unit normal on the obstacle xyz, probe seg).  Defined here for the same reason */
#define PIH_CLEAR_WORDS 12
#include "pih_robot.h"
#endif
