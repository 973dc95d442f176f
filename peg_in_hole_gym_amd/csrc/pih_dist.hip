// pih_dist.hip -- kernels of the batched closest-point queries (pih_dist.h; pih_closest_points of include/pih_robot.h).  A translation
// unit of its own beside the ray tests', whose set-up and mapping it shares.
// Mapping: grid = (query chunks, envs), 256 threads (4 waves).  The workgroup does the ray kernels' per-env set-up once -- peg-in-hole:
// state record -> LDS, fk_all, the primitives' poses, their bounding spheres (four barriers); random-fly: pose words, the poses, the
// spheres (two) -- and then one query per lane, in a loop over its chunk of `chunk` queries (a multiple of 256; the launch function says
// how it is chosen).  Every lane walks the primitive list in the same order: the primitive mask of `groups` is a kernel argument, the scene
// reads are same-address LDS broadcasts; lanes diverge on whether a primitive's bounding sphere is within reach of their running best.
//   points   PIH_RAY_SHARED: float[P, 4], every workgroup of the call reads the same rows (from L2 after the first); else float[count, P, 4].
//            A query is one 16-byte load per lane, a wave loads 1 KB contiguous
//   out      float[count, P, 8]: two 16-byte stores per lane, a wave stores 2 KB contiguous
// Bounds: query r = blockIdx.x * chunk + i * 256 + tid runs only when r < min(P, (blockIdx.x + 1) * chunk); it reads words
// [4 r, 4 r + 4) of its env's (or the shared) rows and writes words [8 r, 8 r + 8) of its env's records; P <= 2^20 and chunk <= 2^10 keep
// the products in int, the env strides are size_t.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "pih_dist.h"
#include "pih_launch.h"

using namespace pih;

namespace {

static_assert(PIH_POINT_WORDS == 4 && PIH_CLOSEST_WORDS == 8, "a query is one float4, a record two");
// the queries of this workgroup's chunk, one per lane and pass: record(query words) -> dist::Record
template <class F> __device__ __forceinline__ void chunk_walk(float* __restrict__ out, const float* __restrict__ points, int P, int chunk, int flags, const F& record) {
  const int e = blockIdx.y;
  const float4* rows = reinterpret_cast<const float4*>(points + ((flags & PIH_RAY_SHARED) ? (size_t)0 : (size_t)e * P * PIH_POINT_WORDS));
  float4* records = reinterpret_cast<float4*>(out + (size_t)e * P * PIH_CLOSEST_WORDS);
  const int r1 = min(P, ((int)blockIdx.x + 1) * chunk);
  for (int r = (int)blockIdx.x * chunk + (int)threadIdx.x; r < r1; r += RENDER_THREADS) {
    const float4 q = rows[r];
    const float w[PIH_POINT_WORDS] = {q.x, q.y, q.z, q.w};
    const dist::Record rec = record(w);
    records[2 * (size_t)r] = make_float4(rec.w[0], rec.w[1], rec.w[2], rec.w[3]);
    records[2 * (size_t)r + 1] = make_float4(rec.w[4], rec.w[5], rec.w[6], rec.w[7]);
  }
}

}  // namespace

// CULL: a primitive whose bounding sphere is not within reach of the running best is skipped (pih_dist.h).  The same primitive wins either
// way; the two instances are two compilations under -ffast-math, and a record of one can differ from the other's in its last bits.
// peg-in-hole: env-major records of PIH_STATE_WORDS words
template <bool CULL> __global__ void __launch_bounds__(RENDER_THREADS) pih_dist_view_kernel(const float* __restrict__ state, float* __restrict__ out, const float* __restrict__ points,
                                                                       int P, int chunk, int env_begin, int flags, int groups) {
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
  const unsigned long long prims = dist::view_prims(groups);
  chunk_walk(out, points, P, chunk, flags, [&](const float* words) __attribute__((always_inline)) { return dist::view_record<CULL>(sc, words, flags, prims); });
}

// random-fly: structure-of-arrays state [word][env] of n envs
template <bool CULL> __global__ void __launch_bounds__(RENDER_THREADS) pih_dist_fly_kernel(const float* __restrict__ state, float* __restrict__ out, const float* __restrict__ points,
                                                                      int P, int chunk, int n, int object, int env_begin, int flags, int groups) {
  __shared__ fly::FlyScene sc;
  const int tid = threadIdx.x;
  if (tid < 16) rays::fly_setup_poses(sc, fly::load_fly_pose(state, env_begin + blockIdx.y, n), object, tid);
  __syncthreads();
  rays::fly_setup_balls(sc, tid);
  __syncthreads();
  const unsigned prims = dist::fly_prims(object, groups);
  chunk_walk(out, points, P, chunk, flags, [&](const float* words) __attribute__((always_inline)) { return dist::fly_record<CULL>(sc, words, flags, prims); });
}

namespace pih {
// Called by pih_closest_points (pih_hip.hip), which has validated every argument: 1 <= points_per_env <= 2^20, 1 <= env_count <= 65535
// inside the handle's envs, known flags, groups that select something in the task, both pointers 16-byte aligned.
// Chunk: the ray tests' policy (ray_test_launch) -- k x 256 queries, k = min(4, ceil(P / 256)), less while the grid would stay below
// DIST_MIN_GRID workgroups.
// Rejection: the kernels with it are the default for peg-in-hole calls of at most DIST_CULL_MAX_POINTS queries per env, the kernels
// without it for larger calls and for random-fly.  A wave skips a primitive only if all its lanes do: the few probe points of a reward
// term lie together and skip most of the 38 primitives (measured 34 against 42 us at 4096 envs x 16 or 64 queries), 1024 points spread
// over the workspace skip next to nothing and pay for the test (240 against 202 us); random-fly's 8 to 11 primitives never repay it
// (10.7 against 10.4 us, 61 against 55 us).  DESIGN.md 6.8 has the table.
// PIH_DIST_CHUNK = 1 .. 4 in the environment fixes k, PIH_DIST_CULL = 0 | 1 the kernels without / with the rejection: the measurement
// switches of tools/dist_bench.py, not part of the ABI.  Neither changes which primitive a record names; the chunk size changes no bit.
constexpr int DIST_MAX_PER_LANE = 4, DIST_MIN_GRID = 1024, DIST_CULL_MAX_POINTS = 256;
void closest_points_launch(bool fly_task, hipStream_t stream, const float* state, float* out, const float* points, int points_per_env,
                           int groups, int n_envs, int object, int env_begin, int env_count, int flags) {
  const int passes = (points_per_env + RENDER_THREADS - 1) / RENDER_THREADS;
  int k = passes < DIST_MAX_PER_LANE ? passes : DIST_MAX_PER_LANE;
  while (k > 1 && (long long)env_count * ((passes + k - 1) / k) < DIST_MIN_GRID) k--;
  if (const char* e = getenv("PIH_DIST_CHUNK")) {
    const int v = atoi(e);
    if (v >= 1 && v <= DIST_MAX_PER_LANE) k = v;
  }
  bool cull = !fly_task && points_per_env <= DIST_CULL_MAX_POINTS;
  if (const char* e = getenv("PIH_DIST_CULL")) cull = atoi(e) != 0;
  const int chunk = k * RENDER_THREADS;
  const dim3 grid((points_per_env + chunk - 1) / chunk, env_count), block(RENDER_THREADS);
  if (fly_task) {
    if (cull) hipLaunchKernelGGL(pih_dist_fly_kernel<true>, grid, block, 0, stream, state, out, points, points_per_env, chunk, n_envs, object, env_begin, flags, groups);
    else hipLaunchKernelGGL(pih_dist_fly_kernel<false>, grid, block, 0, stream, state, out, points, points_per_env, chunk, n_envs, object, env_begin, flags, groups);
  } else {
    if (cull) hipLaunchKernelGGL(pih_dist_view_kernel<true>, grid, block, 0, stream, state, out, points, points_per_env, chunk, env_begin, flags, groups);
    else hipLaunchKernelGGL(pih_dist_view_kernel<false>, grid, block, 0, stream, state, out, points, points_per_env, chunk, env_begin, flags, groups);
  }
}
}  // namespace pih
