// pih_rays.hip -- kernels of the batched ray tests (pih_rays.h; pih_ray_test of include/pih_robot.h).  A translation unit of its own
// beside the step kernels'; its kernels' records are held to tests/golden/scene_bits.npz by tests/test_gpu_scene_bits.py.
// Mapping: grid = (ray chunks, envs), 256 threads (4 waves).  The workgroup does the cameras' per-env set-up once, without a camera --
// peg-in-hole: state record -> LDS, fk_all, the primitives' poses, their bounding spheres (four barriers); random-fly: pose words, the
// poses, the spheres (two) -- and then one ray per lane, in a loop over its chunk of `chunk` rays (a multiple of 256; the launch function says how it is chosen).
// Every lane walks the whole primitive list in the same order: the scene reads are same-address LDS broadcasts, the branches on the
// primitive kind are wave-uniform; lanes diverge only inside a primitive function (hit or miss) and on the kind of the nearest hit,
// where the normal is taken.
//   rays     PIH_RAY_SHARED: float[R, 6], every workgroup of the call reads the same rows (from L2 after the first); else float[count, R, 6].
//            A ray is 24 bytes: three 8-byte loads per lane (a row is 8-byte aligned: rays_dev is 16-byte aligned)
//   out      float[count, R, 8]: two 16-byte stores per lane, a wave stores 2 KB contiguous
// Bounds: ray r = blockIdx.x * chunk + i * 256 + tid runs only when r < min(R, (blockIdx.x + 1) * chunk); it reads words
// [6 r, 6 r + 6) of its env's (or the shared) rows and writes words [8 r, 8 r + 8) of its env's records; R <= 2^20 and chunk <= 2^10 keep
// the products in int, the env strides are size_t.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "pih_rays.h"
#include "pih_launch.h"

using namespace pih;

namespace {

__device__ __forceinline__ void load_ray(const float* __restrict__ rows, int r, float* w) {
  const float2* p = reinterpret_cast<const float2*>(rows + (size_t)r * PIH_RAY_WORDS);
  const float2 a = p[0], b = p[1], c = p[2];
  w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y; w[4] = c.x; w[5] = c.y;
}
__device__ __forceinline__ void store_record(float* __restrict__ records, int r, const rays::Record& rec) {
  float4* p = reinterpret_cast<float4*>(records + (size_t)r * PIH_RAY_HIT_WORDS);
  p[0] = make_float4(rec.w[0], rec.w[1], rec.w[2], rec.w[3]);
  p[1] = make_float4(rec.w[4], rec.w[5], rec.w[6], rec.w[7]);
}
// the rays of this workgroup's chunk, one per lane and pass: record(ray words) -> rays::Record
template <class F> __device__ __forceinline__ void chunk_walk(float* __restrict__ out, const float* __restrict__ rays_dev, int R, int chunk, int flags, const F& record) {
  const int e = blockIdx.y;
  const float* rows = rays_dev + ((flags & PIH_RAY_SHARED) ? (size_t)0 : (size_t)e * R * PIH_RAY_WORDS);
  float* records = out + (size_t)e * R * PIH_RAY_HIT_WORDS;
  const int r1 = min(R, ((int)blockIdx.x + 1) * chunk);
  for (int r = (int)blockIdx.x * chunk + (int)threadIdx.x; r < r1; r += RENDER_THREADS) {
    float w[PIH_RAY_WORDS];
    load_ray(rows, r, w);
    store_record(records, r, record(w));
  }
}

}  // namespace

// CULL: a ray that misses a primitive's bounding sphere skips the primitive function (pih_rays.h).  The same hits either way; the two
// instances are two compilations under -ffast-math, and a record of one can differ from the other's in its last bits.
// peg-in-hole: env-major records of PIH_STATE_WORDS words
template <bool CULL> __global__ void __launch_bounds__(RENDER_THREADS) pih_ray_view_kernel(const float* __restrict__ state, float* __restrict__ out, const float* __restrict__ rays_dev,
                                                                      int R, int chunk, int env_begin, int flags) {
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
  chunk_walk(out, rays_dev, R, chunk, flags, [&](const float* words) __attribute__((always_inline)) { return rays::view_record<CULL>(sc, words, flags); });
}

// random-fly: structure-of-arrays state [word][env] of n envs
template <bool CULL> __global__ void __launch_bounds__(RENDER_THREADS) pih_ray_fly_kernel(const float* __restrict__ state, float* __restrict__ out, const float* __restrict__ rays_dev,
                                                                     int R, int chunk, int n, int object, int env_begin, int flags) {
  __shared__ fly::FlyScene sc;
  const int tid = threadIdx.x;
  if (tid < 16) rays::fly_setup_poses(sc, fly::load_fly_pose(state, env_begin + blockIdx.y, n), object, tid);
  __syncthreads();
  rays::fly_setup_balls(sc, tid);
  __syncthreads();
  chunk_walk(out, rays_dev, R, chunk, flags, [&](const float* words) __attribute__((always_inline)) { return rays::fly_record<CULL>(sc, object, words, flags); });
}

namespace pih {
// Called by pih_ray_test (pih_hip.hip), which has validated every argument: 1 <= rays_per_env <= 2^20, 1 <= env_count <= 65535 inside the
// handle's envs, known flags, both pointers 16-byte aligned.
// Chunk: k x 256 rays, k rays per lane.  The set-up is paid once per workgroup, so k = min(4, ceil(R / 256)) where the call has
// workgroups to spare, and less -- down to 1 -- while the grid would stay below RAY_MIN_GRID workgroups (a few per compute unit): a call
// of few envs and many rays spreads its rays.  PIH_RAY_CHUNK = 1 .. 4 in the environment fixes k, PIH_RAY_CULL = 0 | 1 picks the kernels
// without / with the bounding-sphere rejection (default: with): the measurement switches of tools/ray_bench.py, not part of the ABI.
// The chunk size does not change a bit of the output.
constexpr int RAY_MAX_PER_LANE = 4, RAY_MIN_GRID = 1024;
void ray_test_launch(bool fly_task, hipStream_t stream, const float* state, float* out, const float* rays_dev, int rays_per_env,
                     int n_envs, int object, int env_begin, int env_count, int flags) {
  const int passes = (rays_per_env + RENDER_THREADS - 1) / RENDER_THREADS;
  int k = passes < RAY_MAX_PER_LANE ? passes : RAY_MAX_PER_LANE;
  while (k > 1 && (long long)env_count * ((passes + k - 1) / k) < RAY_MIN_GRID) k--;
  if (const char* e = getenv("PIH_RAY_CHUNK")) {
    const int v = atoi(e);
    if (v >= 1 && v <= RAY_MAX_PER_LANE) k = v;
  }
  bool cull = true;
  if (const char* e = getenv("PIH_RAY_CULL")) cull = atoi(e) != 0;
  const int chunk = k * RENDER_THREADS;
  const dim3 grid((rays_per_env + chunk - 1) / chunk, env_count), block(RENDER_THREADS);
  if (fly_task) {
    if (cull) hipLaunchKernelGGL(pih_ray_fly_kernel<true>, grid, block, 0, stream, state, out, rays_dev, rays_per_env, chunk, n_envs, object, env_begin, flags);
    else hipLaunchKernelGGL(pih_ray_fly_kernel<false>, grid, block, 0, stream, state, out, rays_dev, rays_per_env, chunk, n_envs, object, env_begin, flags);
  } else {
    if (cull) hipLaunchKernelGGL(pih_ray_view_kernel<true>, grid, block, 0, stream, state, out, rays_dev, rays_per_env, chunk, env_begin, flags);
    else hipLaunchKernelGGL(pih_ray_view_kernel<false>, grid, block, 0, stream, state, out, rays_dev, rays_per_env, chunk, env_begin, flags);
  }
}
}  // namespace pih
