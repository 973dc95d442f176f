// pih_launch.h -- every function the C ABI (pih_hip.hip) calls in a kernel translation unit.  Included by pih_hip.hip AND by the translation
// unit that defines the function: one declaration, compiled on both sides, where there used to be a hand-written copy in the caller.
// A kernel translation unit owns its kernels' grid shapes, dynamic-LDS sizes, instantiation choice and function attributes; the caller has
// validated every argument and hands over what it owns: device pointers, the batch size, the launch epoch, the bin buffers, the stream.
// None of these report an error: the caller reads hipGetLastError() after the launch (fly_step_prepare returns its own).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace pih {
struct Params;
namespace fly { struct FlyCam; }

// what a step launch of either task reads and writes (obs / reward / done / dbg may be nullptr)
struct StepIO { float* state; const float* actions; float* obs; float* reward; unsigned char* done; float* dbg; };
// the fused launch's handshake (pih_mailbox.h): controller mailbox, one flag per group of 64 envs, the error word, this launch's epoch
struct Mailbox { float* mail; int* flags; int* err; int epoch; };
// the three bin buffers of the in-kernel dispatch order, in this launch's rotation; all nullptr: block b = env b
struct Bins { const int* cur; int* next; int* zero; };

// ---- pih_peg.hip: the peg-in-hole task's kernels
size_t peg_mail_words(int n);                 // floats of the controller mailbox of n envs
size_t peg_bin_ints(int n);                   // ints of ONE bin buffer of n envs
void peg_init_offsets_launch(hipStream_t stream, float* state, const float* offsets, int n);
void peg_reset_launch(hipStream_t stream, const Params& P, float* state, const unsigned char* mask, int hard, int rewind, int n);
void peg_bins_init_launch(hipStream_t stream, const float* state, int* bins, int n);
void peg_pre_launch(hipStream_t stream, const Params& P, float* state, const float* actions, int* order, int n);      // launch 1 of the two-launch step
void peg_step_launch(hipStream_t stream, const Params& P, const StepIO& io, float* ovf, const int* order, int n);      // launch 2 of the two-launch step
void peg_step_fused_launch(hipStream_t stream, const Params& P, const StepIO& io, float* ovf, int n, const Mailbox& mb, const Bins& bins);
void peg_gather_launch(hipStream_t stream, const float* state, float* out, int n, int word0, int nwords);
void ik_launch(bool ur5, hipStream_t stream, const Params& P, int n, const float* q0, const float* tpos, const float* tquat, float* qout);
void render_launch(dim3 grid, hipStream_t stream, const float* state, float* out, int env_begin, int W, int H, int rows_per_strip, int flags);
void labels_launch(hipStream_t stream, const float* state, float* out, float* meta, int env_begin, int env_count, int S);

// ---- pih_fly.hip: the random-fly task's step, reset and state-layout kernels
size_t fly_mail_words(int n);                 // floats of the controller mailbox of n envs
bool fly_fused_fits(int n, bool quad, int cus);      // are ALL workgroups of the fused launch resident at once on `cus` compute units?
hipError_t fly_step_prepare(bool quad);       // the dynamic-LDS limit of the layout's step kernels, fused and not (once per handle)
void fly_step_launch(hipStream_t stream, const Params& P, const StepIO& io, int n, bool quad, const Mailbox* mb);      // mb = nullptr: the IK inside the step wavefront
void fly_init_offsets_launch(hipStream_t stream, float* state, const float* offsets, int n);
void fly_reset_launch(hipStream_t stream, const Params& P, float* state, const unsigned char* mask, int hard, int rewind, int n);
void fly_get_words_launch(hipStream_t stream, const float* soa, float* aos, int n, int word0, int nwords);      // words [word0, word0 + nwords) env-major
void fly_set_state_launch(hipStream_t stream, const float* aos, float* soa, int n);

// ---- pih_fly_image.hip: the free camera of the random-fly task, every output format, one host camera or per-env cameras in device memory
void fly_image_launch(int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                      int n, int object, int env_begin, int W, int H, int rows_per_strip, int flags);
// ---- pih_view.hip: the free camera of the peg-in-hole task
void view_launch(int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                 int env_begin, int W, int H, int rows_per_strip, int flags);
// ---- pih_lit.hip: both cameras under a caller-given light, with a specular term and cast shadows
int lit_light_check(const float* words, const char** what);
void lit_launch(bool fly_task, int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                const float* light, const float* light_dev, int n, int object, int env_begin, int W, int H, int rows_per_strip, int flags);
// ---- pih_robot.hip: the batched robot-model queries of include/pih_robot.h
void robot_fk_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, const float* qd, float* out);
void robot_jacobian_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, int frame, const float* local_pos, float* out);
void robot_mass_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, float* out);
void robot_invdyn_launch(int robot, hipStream_t stream, int n, const float* q, const float* qd, const float* qdd, float* tau);
void link_states_launch(bool fly_task, hipStream_t stream, const float* state, float* out, int n_envs, int env_begin, int env_count);
int robot_dims(int robot, int* ndof, int* nframes);
int link_states_frames(int task_id);
// ---- pih_rays.hip: the batched ray tests of include/pih_robot.h
void ray_test_launch(bool fly_task, hipStream_t stream, const float* state, float* out, const float* rays_dev, int rays_per_env,
                     int n_envs, int object, int env_begin, int env_count, int flags);
// ---- pih_dist.hip: the batched closest-point queries of include/pih_robot.h
void closest_points_launch(bool fly_task, hipStream_t stream, const float* state, float* out, const float* points, int points_per_env,
                           int groups, int n_envs, int object, int env_begin, int env_count, int flags);
// ---- pih_clear.hip: the robot clearance queries of include/pih_robot.h (q = nullptr: each env's own joint state)
void robot_clearance_launch(bool fly_task, hipStream_t stream, const float* state, float* out, const float* q, int configs_per_env, float reach,
                            int groups, int n_envs, int object, int env_begin, int env_count, int flags);
int robot_clearance_probes(int task_id);
}  // namespace pih
