// pih_clear.hip -- kernels of the robot clearance queries (pih_clear.h; pih_robot_clearance of include/pih_robot.h).  A translation unit
// of its own beside the closest-point queries', whose set-up and grid it shares.
// Mapping: grid = (work-item chunks, envs), 256 threads (4 waves).  The workgroup does the ray kernels' per-env set-up once -- peg-in-hole:
// state record -> LDS, fk_all, the primitives' poses, their bounding spheres (four barriers); random-fly: pose words, the poses, the
// spheres (two) -- and then walks its chunk of `chunk` work items (a multiple of 256), one per lane and pass.  LDS is the closest-point
// kernels': nothing is staged.
//   SPLIT = false  a work item is a CONFIGURATION: the lane reads its q row, runs the forward kinematics once and loops over the NP probes;
//                  its NP records of 48 bytes lie together, NP x 48 bytes from its neighbour's
//   SPLIT = true   a work item is a (configuration, probe) pair: the lane runs the forward kinematics of its configuration -- NP lanes
//                  repeat it -- and answers one probe; a wave stores 3 KB contiguous
// Every lane walks the obstacles in the same order; the scene reads are same-address LDS broadcasts.
//   q        NULL: one configuration per env, the env's own joint words from its state; PIH_RAY_SHARED: float[C, ndof], every workgroup
//            of the call reads the same rows; else float[count, C, ndof].  Scalar 4-byte loads: rows need only float alignment
//   out      float[count, C, NP, 12]: three 16-byte stores per record
// Bounds: work item r = blockIdx.x * chunk + i * 256 + tid runs only when r < min(items, (blockIdx.x + 1) * chunk), items = C or C x NP;
// its configuration c = r or r / NP is < C: it reads words [ndof c, ndof c + ndof) of its env's (or the shared) rows and writes records
// [NP c, NP c + NP) (SPLIT: record r) of its env's C x NP.  C <= 2^20, NP <= 11 and chunk <= 2^10 keep the products in int, the env
// strides are size_t.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "pih_clear.h"
#include "pih_launch.h"

using namespace pih;

namespace {

__device__ __forceinline__ void store_record(float* __restrict__ records, size_t index, const clear::Record& rec) {
  float4* o = reinterpret_cast<float4*>(records) + 3 * index;
  o[0] = make_float4(rec.w[0], rec.w[1], rec.w[2], rec.w[3]);
  o[1] = make_float4(rec.w[4], rec.w[5], rec.w[6], rec.w[7]);
  o[2] = make_float4(rec.w[8], rec.w[9], rec.w[10], rec.w[11]);
}

// the work items of this workgroup's chunk.  own(i) = word i of the env's own joint state (q == nullptr); record(P, ok, p) -> clear::Record
template <class Rb, bool SPLIT, class Own, class F>
__device__ __forceinline__ void chunk_walk(float* __restrict__ out, const float* __restrict__ q, int C, int chunk, int flags, const Own& own, const F& record) {
  constexpr int NP = Rb::NP, ND = Rb::ND;
  const int e = blockIdx.y;
  const float* rows = q ? q + ((flags & PIH_RAY_SHARED) ? (size_t)0 : (size_t)e * C * ND) : nullptr;
  float* records = out + (size_t)e * C * NP * clear::CW;
  const int items = SPLIT ? C * NP : C;
  const int r1 = min(items, ((int)blockIdx.x + 1) * chunk);
  for (int r = (int)blockIdx.x * chunk + (int)threadIdx.x; r < r1; r += RENDER_THREADS) {
    const int c = SPLIT ? r / NP : r;
    float w[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) w[i] = rows ? rows[(size_t)c * ND + i] : own(i);
    real qv[ND];
    const bool ok = clear::load_q<Rb>(w, qv);
    clear::Probes<NP> P;
    clear::place_probes<Rb>(qv, ok, P);
    if (SPLIT) {
      store_record(records, (size_t)r, record(P, ok, r - c * NP));
    } else {
#pragma unroll 1
      for (int p = 0; p < NP; p++) store_record(records, (size_t)c * NP + p, record(P, ok, p));
    }
  }
}

}  // namespace

// CULL: an obstacle whose bounding sphere is not within reach of the probe's running nearest is skipped (pih_clear.h).
// peg-in-hole: env-major records of PIH_STATE_WORDS words
template <bool CULL, bool SPLIT> __global__ void __launch_bounds__(RENDER_THREADS) pih_clear_view_kernel(const float* __restrict__ state, float* __restrict__ out, const float* __restrict__ q,
                                                                                      int C, int chunk, int env_begin, int flags, int groups, float reach) {
  __shared__ Shared sh;
  __shared__ view::ViewScene sc;
  const int tid = threadIdx.x;
  Wave w; w.l = tid; w.counter = 0;
  const float* rec = state + (size_t)(env_begin + blockIdx.y) * PIH_STATE_WORDS;
  for (int i = tid; i < PIH_STATE_WORDS; i += RENDER_THREADS) sh.S[i] = rec[i];
  __syncthreads();
  fk_all(w, sh);
  __syncthreads();
  rays::view_setup_poses(sh, sc, tid);
  __syncthreads();
  rays::view_setup_balls(sc, tid);
  __syncthreads();
  chunk_walk<clear::PandaRobot, SPLIT>(out, q, C, chunk, flags, [&](int i) __attribute__((always_inline)) { return sh.S[PIH_S_QARM + i]; },
      [&](const clear::Probes<clear::PandaRobot::NP>& P, bool ok, int p) __attribute__((always_inline)) { return clear::view_record<CULL>(sc, P, ok, p, reach, groups); });
}

// random-fly: structure-of-arrays state [word][env] of n envs
template <bool CULL, bool SPLIT> __global__ void __launch_bounds__(RENDER_THREADS) pih_clear_fly_kernel(const float* __restrict__ state, float* __restrict__ out, const float* __restrict__ q,
                                                                                     int C, int chunk, int n, int object, int env_begin, int flags, int groups, float reach) {
  __shared__ fly::FlyScene sc;
  const int tid = threadIdx.x;
  const int env = env_begin + blockIdx.y;
  if (tid < 16) rays::fly_setup_poses(sc, fly::load_fly_pose(state, env, n), object, tid);
  __syncthreads();
  rays::fly_setup_balls(sc, tid);
  __syncthreads();
  const int nsph = fly::R_NSPH[object];
  chunk_walk<clear::Ur5Robot, SPLIT>(out, q, C, chunk, flags, [&](int i) __attribute__((always_inline)) { return state[(size_t)(PIH_F_Q + i) * n + env]; },
      [&](const clear::Probes<clear::Ur5Robot::NP>& P, bool ok, int p) __attribute__((always_inline)) { return clear::fly_record<CULL>(sc, nsph, P, ok, p, reach, groups); });
}

namespace pih {
int robot_clearance_probes(int task_id) {
  return task_id == PIH_TASK_PEG_IN_HOLE ? PIH_CLEAR_PROBES_PANDA : (task_id == PIH_TASK_RANDOM_FLY ? PIH_CLEAR_PROBES_UR5 : -1);
}
// Called by pih_robot_clearance (pih_hip.hip), which has validated every argument: 1 <= configs <= 2^20 (1 with q == nullptr),
// 1 <= env_count <= 65535 inside the handle's envs, known flags, groups inside OBJECT | TABLE that select something, reach > 0 and finite,
// out 16-byte aligned.
// The three choices below are measured ones (tools/clearance_bench.py at 4096 envs, DESIGN.md 6.9 has the table):
// Work item: a (configuration, probe) pair below CLEAR_SPLIT_BELOW configurations per env, a configuration from there on.  With few
// configurations a workgroup has few lanes to give them, and each walks its 11 probes one after the other: peg-in-hole 210 against 53 us
// at 1, 293 against 71 us at 16 configurations; at 256 every lane has one and the repeated forward kinematics
// lose, 516 against 592 us (random-fly: 32 / 17, 35 / 22, 113 / 129 us).  Between 16 and 256 the two were not timed: 256 is where every
// lane of a workgroup has a configuration, not a measured crossover.
// Rejection: on, except for random-fly's per-probe instance: peg-in-hole 211 against 517 us and 516 against 668 us per configuration, 53 / 64 and
// 592 / 710 us per probe; random-fly's 2 to 5 spheres repay it per configuration (113 against 126 us) and not per probe (129 / 128, 176 / 173 us).
// Chunk: the closest-point queries' policy -- k x 256 work items, k = min(4, ceil(items / 256)), less while the grid would stay below
// CLEAR_MIN_GRID workgroups; k = 1 / 2 / 4 measure 516 / 517 / 518 us on peg-in-hole and 132 / 127 / 126 us on random-fly at 256 configurations.
// PIH_CLEAR_CHUNK = 1 .. 4 in the environment fixes k, PIH_CLEAR_CULL = 0 | 1 and PIH_CLEAR_SPLIT = 0 | 1 the kernel instance: the
// measurement switches of tools/clearance_bench.py, not part of the ABI.  None changes which obstacle a record names; the chunk size
// changes no bit.
constexpr int CLEAR_MAX_PER_LANE = 4, CLEAR_MIN_GRID = 1024;
constexpr int CLEAR_SPLIT_BELOW = 256;
template <bool CULL, bool SPLIT>
static void launch(bool fly_task, dim3 grid, hipStream_t stream, const float* state, float* out, const float* q, int C, int chunk, float reach, int groups,
                   int n_envs, int object, int env_begin, int flags) {
  const dim3 block(RENDER_THREADS);
  if (fly_task) hipLaunchKernelGGL((pih_clear_fly_kernel<CULL, SPLIT>), grid, block, 0, stream, state, out, q, C, chunk, n_envs, object, env_begin, flags, groups, reach);
  else hipLaunchKernelGGL((pih_clear_view_kernel<CULL, SPLIT>), grid, block, 0, stream, state, out, q, C, chunk, env_begin, flags, groups, reach);
}
void robot_clearance_launch(bool fly_task, hipStream_t stream, const float* state, float* out, const float* q, int configs_per_env, float reach,
                            int groups, int n_envs, int object, int env_begin, int env_count, int flags) {
  bool split = configs_per_env < CLEAR_SPLIT_BELOW;
  if (const char* e = getenv("PIH_CLEAR_SPLIT")) split = atoi(e) != 0;
  bool cull = !(fly_task && split);
  if (const char* e = getenv("PIH_CLEAR_CULL")) cull = atoi(e) != 0;
  const int items = configs_per_env * (split ? (fly_task ? PIH_CLEAR_PROBES_UR5 : PIH_CLEAR_PROBES_PANDA) : 1);
  const int passes = (items + RENDER_THREADS - 1) / RENDER_THREADS;
  int k = passes < CLEAR_MAX_PER_LANE ? passes : CLEAR_MAX_PER_LANE;
  while (k > 1 && (long long)env_count * ((passes + k - 1) / k) < CLEAR_MIN_GRID) k--;
  if (const char* e = getenv("PIH_CLEAR_CHUNK")) {
    const int v = atoi(e);
    if (v >= 1 && v <= CLEAR_MAX_PER_LANE) k = v;
  }
  const int chunk = k * RENDER_THREADS;
  const dim3 grid((items + chunk - 1) / chunk, env_count);
  if (cull) {
    if (split) launch<true, true>(fly_task, grid, stream, state, out, q, configs_per_env, chunk, reach, groups, n_envs, object, env_begin, flags);
    else launch<true, false>(fly_task, grid, stream, state, out, q, configs_per_env, chunk, reach, groups, n_envs, object, env_begin, flags);
  } else {
    if (split) launch<false, true>(fly_task, grid, stream, state, out, q, configs_per_env, chunk, reach, groups, n_envs, object, env_begin, flags);
    else launch<false, false>(fly_task, grid, stream, state, out, q, configs_per_env, chunk, reach, groups, n_envs, object, env_begin, flags);
  }
}
}  // namespace pih
