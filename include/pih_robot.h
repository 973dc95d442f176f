/* pih_robot.h -- C ABI of the batched robot-model and scene queries (libpih_hip.so); an addition to pih.h, which includes this file: include pih.h.
 * The ABI version stays PIH_ABI_VERSION (the change is additive).  Declared here and not in pih.h for the reason pih_render_view.h
 * states: tests pin the list of functions pih.h itself declares; tests/test_robot_query.py compares _lib.ROBOT_EXPORTS with THIS file.
 *
 * What replaces what (pybullet, per env and on the host -> one call for n problems on the device):
 *   pih_robot_fk / pih_link_states     p.getLinkState(s)(computeLinkVelocity=1): [4:6] = the URDF link frame, [6:8] = its velocity
 *   pih_robot_jacobian                 p.calculateJacobian(body, link, localPosition, q, ...)
 *   pih_robot_mass_matrix              p.calculateMassMatrix(body, q)
 *   pih_robot_inverse_dynamics         p.calculateInverseDynamics(body, q, qd, qdd)  -- see the damping note below
 *   pih_ray_test                       p.rayTestBatch(from, to, parentObjectUniqueId, parentLinkIndex)  -- the scene query, at the end
 *   pih_closest_points                 p.getClosestPoints(bodyA, bodyB, distance) for a point against the scene  -- after it
 *   pih_robot_clearance                p.resetJointState(robot, q) + p.getClosestPoints(robot, body, distance, linkIndexA) per link, for
 *                                      many joint configurations per env  -- the last one
 *
 * Conventions: n problems, independent of the handle's env count (as pih_ik); both robots work on a handle of either task (as pih_ik /
 * pih_ik_ur5).  Every pointer is a DEVICE pointer to float32, row-major, contiguous.  Nothing synchronises: the work is enqueued on the
 * caller's stream.  n == 0 returns 0 without a launch.  Errors: -2, and pih_last_error names the argument, for an unknown robot, a frame
 * out of range, n < 0, n > 2^30 or a NULL required pointer (pih_last_error(NULL) when the handle itself is NULL).
 *
 * Frames: the URDF link frames (not the centres of mass), indexed as the oracle's fk_arm / fk_ur5 index them:
 *   PIH_ROBOT_PANDA  0 .. 8 = the merged links of pih_model.h (joints 1 .. 7, the two fingers), 9 = grasp-target (pybullet link 11)
 *   PIH_ROBOT_UR5    0 .. 5 = the links of joints 1 .. 6, 6 = ee_link
 * Positions are robot-base-local = env-local (the frame pih_ik's targets live in; no env offset).
 *
 * Joint values are caller data: the trigonometry is the full-range sincosf.  The accuracy figures of DESIGN.md 6.6 hold for |q| <= 2 pi;
 * beyond that the outputs stay finite and lose accuracy as fp32 sin / cos of a large argument do (about |q| x 6e-8 in the rotation
 * entries).  A NaN / Inf input gives non-finite outputs for THAT problem only: no table is indexed by anything derived from q.
 */
#ifndef PIH_ROBOT_H
#define PIH_ROBOT_H
#include "pih.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PIH_ROBOT_PANDA 0   /* 9 DOF (7 revolute + 2 finger prismatic); frames 0..8 = the merged links of pih_model.h, 9 = grasp-target (pybullet link 11) */
#define PIH_ROBOT_UR5   1   /* 6 DOF; frames 0..5 = links, 6 = ee_link */

/* out[0] = ndof, out[1] = nframes of a robot */
int pih_robot_dims(int robot, int32_t out[2]);
/* frames per env that pih_link_states writes for a task: peg-in-hole 10 Panda frames + PIH_OBJ_NL (24) pipe links = 34; random-fly 7 UR5
 * frames + the object = 8; < 0 for an unknown task.  (pih_task_dims keeps its three outputs.) */
int pih_link_states_frames(int task_id);

/* link states: out_dev float[n, nframes, PIH_LINK_STATE_WORDS] = pos (3), quat xyzw (4), linear velocity of the frame ORIGIN (3), angular
 * velocity (3), all in the base-local frame's axes.  qd_dev float[n, ndof] or NULL: the velocity words are 0. */
int pih_robot_fk(pih_handle* h, int robot, int n, const float* q_dev, const float* qd_dev, float* out_dev, void* stream);
/* out_dev float[n, 6, ndof]: rows 0..2 linear, 3..5 angular, for the point local_pos (in the frame's coordinates; local_pos_dev float[n, 3]
 * or NULL = the frame's origin) of frame `frame`.  Columns of joints that are not ancestors of the frame are 0; a finger column is
 * (axis, 0).  J qd = the velocity words of pih_robot_fk. */
int pih_robot_jacobian(pih_handle* h, int robot, int n, const float* q_dev, int frame, const float* local_pos_dev, float* out_dev, void* stream);
/* out_dev float[n, ndof, ndof]: the arm's joint-space inertia (Panda: 9 x 9, the two finger DOF on the hand's branch included).  Both
 * triangles are written from the same value: the output is bitwise symmetric. */
int pih_robot_mass_matrix(pih_handle* h, int robot, int n, const float* q_dev, float* out_dev, void* stream);
/* tau_dev float[n, ndof] = M(q) qdd + Coriolis / centrifugal + gravity (PIH_GRAVITY_Z) + damping: the exact inverse of the FREE dynamics of
 * pih_step, tau(q, qd, the step's free acceleration at (q, qd)) = 0.  Damping is what the step applies: the joint damping
 * PIH_LINK_DAMPING / PIH_UR5_DAMPING x qd, and Bullet's per-link damping (every link's m v (k + k |v|) at its centre of mass and
 * I w (k + k |w|), k = 0.04), which the step's free dynamics contain for both robots.
 * PyBullet's calculateInverseDynamics leaves BOTH out.  PIH_LINK_DAMPING is all zero for the Panda; for the UR5 the caller subtracts
 * PIH_UR5_DAMPING x qd for the joint part.  The link part has no closed form in qd; it is the odd part of tau in qd minus the joint part:
 * (tau(q, qd, qdd) - tau(q, -qd, qdd)) / 2 - PIH_UR5_DAMPING x qd, so PyBullet's value is (tau(q, qd, qdd) + tau(q, -qd, qdd)) / 2. */
int pih_robot_inverse_dynamics(pih_handle* h, int robot, int n, const float* q_dev, const float* qd_dev, const float* qdd_dev, float* tau_dev, void* stream);
/* every frame of the envs' CURRENT state in WORLD coordinates (env offset added, as PIH_S_EE / PIH_F_EE are):
 * out_dev float[env_count, pih_link_states_frames(task), PIH_LINK_STATE_WORDS] for envs env_begin .. env_begin + env_count - 1.
 *   peg-in-hole: the 10 Panda frames, then the 24 pipe links (pipe link 0 = the state's base pose; velocities from the joint rates and the
 *                base twist of the state)
 *   random-fly:  the 7 UR5 frames, then the object
 * env_begin < 0, env_count <= 0 or env_begin + env_count > n_envs: -2, as pih_render_cam. */
int pih_link_states(pih_handle* h, float* out_dev, int env_begin, int env_count, void* stream);

/* Batched ray tests against the scene the task's free camera draws, at the envs' CURRENT state: rays_per_env rays for each of the envs
 * env_begin .. env_begin + env_count - 1, on handles of both tasks.
 *   peg-in-hole  the 38 primitives of pih_render_view -- 7 arm capsules, 4 hand spheres, 2 finger boxes, 24 pipe capsules, the hole
 *                tube -- and the table plane
 *   random-fly   the 6 UR5 capsules, the object's spheres and the table plane of pih_render_cam
 * A ray is PIH_RAY_WORDS floats: the segment from (words 0..2) to (words 3..5) in the env-local frame (the env's offset does not enter,
 * as for the cameras), or with PIH_RAY_FRAME_EE in the end-effector frame of each env.  rays_dev float[env_count, rays_per_env, 6], or
 * with PIH_RAY_SHARED float[rays_per_env, 6].
 * out_dev float[env_count, rays_per_env, PIH_RAY_HIT_WORDS], per ray:
 *   word 0      hit fraction in (0, 1]: where along from -> to the nearest hit lies; 1 = no hit, as p.rayTestBatch reports it
 *   word 1      what was hit, the task's segmentation value as a float -- peg-in-hole: arm link 0 .. 6 (the hand is 6), fingers 7 and 8,
 *               PIH_VIEW_SEG_HOLE, PIH_VIEW_SEG_TABLE, PIH_VIEW_SEG_PIPE0 + pipe capsule; random-fly: link 0 .. 5, PIH_SEG_OBJECT,
 *               PIH_SEG_TABLE; PIH_SEG_NONE for no hit
 *   words 2..4  hit position, words 5..7 outward unit normal, both env-local whatever frame the ray came in
 *   no hit      1, PIH_SEG_NONE, position = to (env-local), normal 0
 * Hits are entry hits of front faces with ray parameter 0 < t <= |to - from|: a ray that starts inside a sphere, a capsule or a box does
 * not hit it (but a ray from inside a long capsule along its axis reports the end sphere it runs into); the hole's bore wall is hit from
 * inside the bore; the table plane is two-sided, its normal +z.  The nearest hit wins;
 * among the peg-in-hole arm's overlapping capsules the rule of pih_render_view decides, so a ray through a pixel centre names the link
 * the rgba8 image's seg byte names.
 * A ray with a word that is NaN, infinite or beyond 1e15, or shorter than 1e-15, gets the no-hit record with the position words = its
 * `to` words as given; no other ray is affected, and no table is indexed by anything derived from ray data.
 * Errors: -2, and pih_last_error names the argument: a NULL handle (pih_last_error(NULL)), NULL out_dev or rays_dev, rays_per_env < 1 or
 * > 2^20, env_begin / env_count outside the handle's envs (as pih_link_states) or env_count > 65535, an unknown flag bit, out_dev or
 * rays_dev not 16-byte aligned.  Nothing synchronises: the work is enqueued on the caller's stream. */
#define PIH_RAY_FRAME_EE     1  /* rays are given in the end-effector frame of each env: peg-in-hole the grasp-target frame
                                   (as PIH_RENDER_CAM_EE of pih_render_view), random-fly ee_link (as PIH_RENDER_CAM_EE) */
#define PIH_RAY_SHARED       2  /* rays_dev is float[rays_per_env, 6], the same rays for every env of the call
                                   (default: float[env_count, rays_per_env, 6]) */
#define PIH_RAY_IGNORE_ROBOT 4  /* the arm is transparent: peg-in-hole arm capsules, hand spheres and finger boxes;
                                   random-fly the six UR5 capsules (a sensor mounted on the hand looks out through it) */
int pih_ray_test(pih_handle* h, float* out_dev, const float* rays_dev, int rays_per_env,
                 int env_begin, int env_count, int flags, void* stream);

/* Batched closest-point queries against the same scene, at the envs' CURRENT state: for each of points_per_env points per env, how far it
 * is from the nearest selected primitive, which one that is, the closest point on its surface and the outward normal there.
 * A query is PIH_POINT_WORDS floats: the point x, y, z in the env-local frame, or with PIH_RAY_FRAME_EE in the end-effector frame of each
 * env (the frames of pih_ray_test), and reach [m], the `distance` argument of p.getClosestPoints: only what is nearer than reach is
 * reported.  points_dev float[env_count, points_per_env, 4], or with PIH_RAY_SHARED float[points_per_env, 4].  flags: these two bits.
 * groups: a mask of PIH_GROUP_*, what the point is measured against.  A group the task does not have selects nothing.
 * out_dev float[env_count, points_per_env, PIH_CLOSEST_WORDS], per query:
 *   word 0      the smallest signed distance over the selected primitives, each the primitive's exact signed distance, negative inside it:
 *               sphere and capsule |p - axis| - r; oriented box Euclidean outside, -(distance to the nearest face) inside; the hole tube
 *               the 2-D box distance of the rectangle [-halflen, halflen] x [rin, rout] in (axial, radial) coordinates -- the bore counts
 *               as outside, the hole's centre is +rin away; the table plane z - PIH_TABLE_Z, a half space
 *   word 1      that primitive's segmentation value as a float, the values pih_ray_test reports
 *   words 2..4  the closest point on its surface, words 5..7 the outward unit normal there, both env-local:
 *               query point = closest point + distance x normal, inside and outside alike
 *   miss        nothing selected is nearer than reach: reach, PIH_SEG_NONE, the query point (env-local), normal 0
 * The primitives are walked in the order table, pipe capsules, tube, finger boxes, hand spheres, arm links (1, 5, 0, 2, 3, 4, 6; random-fly:
 * table, links, object spheres) and a later one takes the query only if it is strictly nearer: an exact tie keeps the first.  Where the
 * closest point is not unique (a sphere's centre, a capsule's axis, the tube's axis) one of them is reported, with its finite unit normal.
 * A query with a word that is NaN, infinite or beyond 1e15, or with reach <= 0, gets the miss record with words 0 and 2..4 as given; no
 * other query is affected, and no table is indexed by anything derived from query data.
 * Errors: -2, and pih_last_error names the argument: a NULL handle (pih_last_error(NULL)), NULL out_dev or points_dev, points_per_env < 1
 * or > 2^20, env_begin / env_count outside the handle's envs or env_count > 65535, groups with a bit outside PIH_GROUP_ALL or selecting
 * nothing in the handle's task, an unknown flag bit, out_dev or points_dev not 16-byte aligned.  Nothing synchronises. */
/* (PIH_POINT_WORDS = 4 and PIH_CLOSEST_WORDS = 8 are defined in pih.h, beside PIH_RAY_WORDS) */
#define PIH_GROUP_ARM     1   /* peg-in-hole: 7 arm capsules + 4 hand spheres; random-fly: the 6 UR5 capsules */
#define PIH_GROUP_FINGERS 2   /* peg-in-hole: the two finger-pad boxes */
#define PIH_GROUP_OBJECT  4   /* peg-in-hole: the 24 pipe capsules; random-fly: the object's spheres */
#define PIH_GROUP_HOLE    8   /* peg-in-hole: the hole tube */
#define PIH_GROUP_TABLE   16  /* the table plane z = PIH_TABLE_Z, a half space: negative below it */
#define PIH_GROUP_ALL     31
int pih_closest_points(pih_handle* h, float* out_dev, const float* points_dev, int points_per_env,
                       int groups, int env_begin, int env_count, int flags, void* stream);

/* Robot clearance for many joint configurations: the body-to-body form of p.getClosestPoints.  For each of configs_per_env joint
 * configurations q per env, how far every link of the handle's task's robot -- the Panda on peg-in-hole, the UR5 on random-fly -- placed
 * at q is from the pipe / the flying object and the table AT THE ENV'S CURRENT STATE, and where the two closest points are.
 *   q_dev     float[env_count, configs_per_env, ndof], or with PIH_RAY_SHARED float[configs_per_env, ndof]; ndof as pih_robot_dims reports
 *             it (Panda 9: the two finger words are read and checked but move no probe; UR5 6).  Rows need only float alignment.
 *             NULL, allowed only with configs_per_env == 1: every env is measured at its own current joint state --
 *             p.getClosestPoints(robot, body, distance) as PyBullet answers it
 *   probes    the round primitives the task's free camera draws for the arm and pih_closest_points measures as PIH_GROUP_ARM, placed by
 *             the forward kinematics of pih_robot_fk at q.  Panda, PIH_CLEAR_PROBES_PANDA = 11: the capsules of links 0 .. 6 (from the
 *             parent's origin to the link's), then the four hand spheres (seg 6).  UR5, PIH_CLEAR_PROBES_UR5 = 6: the link capsules.
 *             A sphere is a capsule of zero length
 *   groups    PIH_GROUP_OBJECT (peg-in-hole: the 24 pipe capsules; random-fly: the object's spheres) and / or PIH_GROUP_TABLE (the half
 *             space below z = PIH_TABLE_Z)
 *   reach     [m] > 0, the `distance` argument of p.getClosestPoints: only what is nearer than reach is reported
 * out_dev float[env_count, configs_per_env, probes, PIH_CLEAR_WORDS], 16-byte aligned, per probe:
 *   word 0       the signed distance between the two surfaces, negative for an overlap.  Exact: capsule - capsule the distance of the two
 *                axis segments minus both radii, capsule - sphere the point - segment distance minus both radii, capsule - table
 *                z - r - PIH_TABLE_Z of the lower end point
 *   word 1       the nearest obstacle primitive's segmentation value as a float, the values pih_ray_test reports
 *   words 2..4   the closest point on the probe's surface, words 5..7 the closest point on the obstacle's surface, env-local
 *   words 8..10  the unit normal on the obstacle, towards the probe (contactNormalOnB):
 *                point on probe = point on obstacle + distance x normal, for overlapping and separated pairs alike
 *   word 11      the probe's own segmentation value (its link), always
 *   miss         nothing selected is nearer than reach: reach, PIH_SEG_NONE, the probe's first axis end point in both point slots, normal 0
 * Where the closest pair is not unique (parallel axes, a horizontal capsule over the table, intersecting axes) one closest pair is reported
 * with a finite unit normal; where the axes touch, the normal is a perpendicular of both.  The obstacles are walked in the order table,
 * then the object's primitives by index, and a later one replaces the running nearest only if it is strictly nearer.
 * A configuration with a word that is NaN, infinite or beyond 1e15 gets the miss record with the point words 0 for all its probes; no
 * other configuration is affected, and no table is indexed by anything derived from q.
 * Not measured: the finger-pad boxes as probes (box - capsule has no short exact form); PIH_GROUP_HOLE (the capsule - tube
 * distance is a quartic, and the step never collides the arm with the hole fixture: pih_closest_points on chosen points measures against
 * the hole); the arm against itself (it needs an allowed-pair table); a GRASPED pipe stays where the env's state has it and does not move
 * with q -- callers who plan with the pipe in hand leave PIH_GROUP_OBJECT out.
 * Errors: -2, and pih_last_error names the argument: a NULL handle (pih_last_error(NULL)) or out_dev, q_dev == NULL with
 * configs_per_env != 1, configs_per_env < 1 or > 2^20, reach not finite or <= 0, env_begin / env_count outside the handle's envs or
 * env_count > 65535, a flag bit other than PIH_RAY_SHARED, a groups bit outside PIH_GROUP_OBJECT | PIH_GROUP_TABLE or a mask that selects
 * nothing, out_dev not 16-byte aligned.  Nothing synchronises. */
/* (PIH_CLEAR_WORDS = 12 is defined in pih.h, beside PIH_CLOSEST_WORDS) */
#define PIH_CLEAR_PROBES_PANDA 11   /* arm capsules of links 0..6, then the 4 hand spheres (seg 6) */
#define PIH_CLEAR_PROBES_UR5   6    /* the six link capsules */
int pih_robot_clearance_probes(int task_id);   /* 11 / 6, < 0 for an unknown task */
int pih_robot_clearance(pih_handle* h, float* out_dev, const float* q_dev, int configs_per_env, float reach,
                        int groups, int env_begin, int env_count, int flags, void* stream);
#ifdef __cplusplus
}
#endif
#endif
