// pih_robot.hip -- kernels of the batched robot-model queries (pih_robot.h; the calls of include/pih_robot.h).  A translation unit of its
// own: the step kernels' code stays what tools/isa_fingerprint.py shows for it whatever changes here.
// Mapping: one problem per lane, one wavefront per workgroup (64 problems), plain scalar code per lane; grid = ceil(n / 64).
//   STAGED = false   every lane stores its own output rows: a store instruction of the wavefront touches 64 rows, W words apart
//   STAGED = true    the lanes write their rows to LDS (row stride W | 1: odd, conflict-free), then the wavefront stores the 64 rows --
//                    contiguous in the output -- as runs of 64 consecutive words (256 bytes per store instruction).  33.5 KB of LDS per
//                    wavefront for the largest output (Panda link states, 64 x 131 words)
// Bounds: problem i = blockIdx.x * 64 + lane runs only when i < n; the staged copy stores words [64 W blockIdx.x, 64 W blockIdx.x + cnt W)
// with cnt = min(64, n - 64 blockIdx.x) rows, and reads LDS words below cnt (W | 1) <= 64 (W | 1).
#include <hip/hip_runtime.h>
#include "pih_robot.h"
#include "pih_launch.h"

using namespace pih;
using namespace pih::robot;

namespace {

constexpr int LANES = 64;

// runs `f(real* rows)` for the lane's problem and delivers its W output words to out[i * W ..]
template <int W, bool STAGED, class F> __device__ __forceinline__ void per_lane_output(int n, float* __restrict__ out, F f) {
  const int lane = threadIdx.x, base = blockIdx.x * LANES, i = base + lane;
  if constexpr (STAGED) {
    constexpr int WP = W | 1;
    __shared__ float buf[LANES * WP];
    if (i < n) f(buf + lane * WP);
    __syncthreads();
    const int cnt = min(LANES, n - base);
    float* dst = out + (size_t)base * W;
    for (int k = lane; k < cnt * W; k += LANES) { const int r = k / W; dst[k] = buf[r * WP + (k - r * W)]; }
  } else {
    if (i < n) f(out + (size_t)i * W);
  }
}

template <int N> __device__ __forceinline__ void load_row(const float* __restrict__ p, int i, float* v) {
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = p[(size_t)i * N + k];
}

}  // namespace

template <class Rb, bool STAGED> __global__ void __launch_bounds__(64) pih_robot_fk_kernel(int n, const float* __restrict__ q, const float* __restrict__ qd, float* __restrict__ out) {
  per_lane_output<Rb::NF * LSW, STAGED>(n, out, [&](float* rows) __attribute__((always_inline)) {
    const int i = blockIdx.x * LANES + threadIdx.x;
    float qv[Rb::ND], qdv[Rb::ND];
    load_row<Rb::ND>(q, i, qv);
    if (qd) load_row<Rb::ND>(qd, i, qdv);
    else {
#pragma unroll
      for (int k = 0; k < Rb::ND; k++) qdv[k] = 0;
    }
    fk_states<Rb>(qv, qdv, mk(0, 0, 0), rows);
  });
}

template <class Rb, bool STAGED> __global__ void __launch_bounds__(64) pih_robot_jacobian_kernel(int n, const float* __restrict__ q, int frame, const float* __restrict__ local_pos, float* __restrict__ out) {
  per_lane_output<6 * Rb::ND, STAGED>(n, out, [&](float* rows) __attribute__((always_inline)) {
    const int i = blockIdx.x * LANES + threadIdx.x;
    float qv[Rb::ND], lp[3] = {0, 0, 0};
    load_row<Rb::ND>(q, i, qv);
    if (local_pos) load_row<3>(local_pos, i, lp);
    jacobian<Rb>(qv, frame, mk(lp[0], lp[1], lp[2]), rows);
  });
}

template <class Rb, bool STAGED> __global__ void __launch_bounds__(64) pih_robot_mass_kernel(int n, const float* __restrict__ q, float* __restrict__ out) {
  per_lane_output<Rb::ND * Rb::ND, STAGED>(n, out, [&](float* rows) __attribute__((always_inline)) {
    const int i = blockIdx.x * LANES + threadIdx.x;
    float qv[Rb::ND];
    load_row<Rb::ND>(q, i, qv);
    mass_matrix<Rb>(qv, rows);
  });
}

// (6 .. 9 output words per problem: staging them was never faster, so there is the one variant)
template <class Rb> __global__ void __launch_bounds__(64) pih_robot_invdyn_kernel(int n, const float* __restrict__ q, const float* __restrict__ qd, const float* __restrict__ qdd, float* __restrict__ out) {
  per_lane_output<Rb::ND, false>(n, out, [&](float* rows) __attribute__((always_inline)) {
    const int i = blockIdx.x * LANES + threadIdx.x;
    float qv[Rb::ND], qdv[Rb::ND], qddv[Rb::ND];
    load_row<Rb::ND>(q, i, qv); load_row<Rb::ND>(qd, i, qdv); load_row<Rb::ND>(qdd, i, qddv);
    inverse_dynamics<Rb>(qv, qdv, qddv, rows);
  });
}

// link states of the envs' state: one env per lane, every lane stores its own rows (34 x 13 words per env would be 113 KB of staging).
// peg-in-hole: env-major records of PIH_STATE_WORDS words
__global__ void __launch_bounds__(64) pih_link_states_kernel(const float* __restrict__ state, float* __restrict__ out, int env_begin, int env_count) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= env_count) return;
  const float* rec = state + (size_t)(env_begin + e) * PIH_STATE_WORDS;
  peg_link_states([&](int w) __attribute__((always_inline)) { return rec[w]; }, out + (size_t)e * PEG_FRAMES * LSW);
}
// random-fly: structure-of-arrays state [word][env] of n_envs envs
__global__ void __launch_bounds__(64) pih_fly_link_states_kernel(const float* __restrict__ state, float* __restrict__ out, int n_envs, int env_begin, int env_count) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= env_count) return;
  const float* col = state + (env_begin + e);
  fly_link_states([&](int w) __attribute__((always_inline)) { return col[(size_t)w * n_envs]; }, out + (size_t)e * FLY_FRAMES * LSW);
}

namespace pih {
// Called by the entry points of include/pih_robot.h (pih_hip.hip), which have validated every argument: robot is PIH_ROBOT_PANDA or
// PIH_ROBOT_UR5, 1 <= n <= 2^30 (the grid and the problem index are int), frame within the robot's frames; `staged` is their choice by n.
#define PIH_ROBOT_LAUNCH(KERNEL, ...)                                                                                   \
  do {                                                                                                                  \
    const dim3 grid((n + LANES - 1) / LANES), block(LANES);                                                             \
    if (robot == PIH_ROBOT_PANDA) {                                                                                     \
      if (staged) hipLaunchKernelGGL((KERNEL<Panda, true>), grid, block, 0, stream, __VA_ARGS__);                       \
      else hipLaunchKernelGGL((KERNEL<Panda, false>), grid, block, 0, stream, __VA_ARGS__);                             \
    } else {                                                                                                            \
      if (staged) hipLaunchKernelGGL((KERNEL<Ur5, true>), grid, block, 0, stream, __VA_ARGS__);                         \
      else hipLaunchKernelGGL((KERNEL<Ur5, false>), grid, block, 0, stream, __VA_ARGS__);                               \
    }                                                                                                                   \
  } while (0)

void robot_fk_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, const float* qd, float* out) {
  PIH_ROBOT_LAUNCH(pih_robot_fk_kernel, n, q, qd, out);
}
void robot_jacobian_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, int frame, const float* local_pos, float* out) {
  PIH_ROBOT_LAUNCH(pih_robot_jacobian_kernel, n, q, frame, local_pos, out);
}
void robot_mass_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, float* out) {
  PIH_ROBOT_LAUNCH(pih_robot_mass_kernel, n, q, out);
}
void robot_invdyn_launch(int robot, hipStream_t stream, int n, const float* q, const float* qd, const float* qdd, float* tau) {
  const dim3 grid((n + LANES - 1) / LANES), block(LANES);
  if (robot == PIH_ROBOT_PANDA) hipLaunchKernelGGL(pih_robot_invdyn_kernel<Panda>, grid, block, 0, stream, n, q, qd, qdd, tau);
  else hipLaunchKernelGGL(pih_robot_invdyn_kernel<Ur5>, grid, block, 0, stream, n, q, qd, qdd, tau);
}
#undef PIH_ROBOT_LAUNCH
void link_states_launch(bool fly_task, hipStream_t stream, const float* state, float* out, int n_envs, int env_begin, int env_count) {
  const dim3 grid((env_count + LANES - 1) / LANES), block(LANES);
  if (fly_task) hipLaunchKernelGGL(pih_fly_link_states_kernel, grid, block, 0, stream, state, out, n_envs, env_begin, env_count);
  else hipLaunchKernelGGL(pih_link_states_kernel, grid, block, 0, stream, state, out, env_begin, env_count);
}
int robot_dims(int robot, int* ndof, int* nframes) {
  if (robot == PIH_ROBOT_PANDA) { *ndof = Panda::ND; *nframes = Panda::NF; return 0; }
  if (robot == PIH_ROBOT_UR5) { *ndof = Ur5::ND; *nframes = Ur5::NF; return 0; }
  return -2;
}
int link_states_frames(int task_id) {
  return task_id == PIH_TASK_PEG_IN_HOLE ? PEG_FRAMES : (task_id == PIH_TASK_RANDOM_FLY ? FLY_FRAMES : -2);
}
}  // namespace pih
