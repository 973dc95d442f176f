// pih_fly_image.hip -- the free camera of the random-fly task (pih_fly_render.h; pih_render_cam): every output format, one host camera
// or per-env cameras.  A translation unit of its own beside pih_fly.hip: the fly step kernels' code stays what tools/isa_fingerprint.py
// shows for it whatever changes here.
//   FMT       0: float4 (depth, r, g, b) | PIH_RENDER_OUT_RGBA8: one 32-bit word (r, g, b, seg) | PIH_RENDER_OUT_DEPTH: one float
//   cam_dev   != nullptr (PIH_RENDER_CAM_DEVICE): float[count, PIH_CAM_WORDS], row blockIdx.y is this workgroup's camera -- 13 more
//             wave-uniform loads, like the state words; nullptr: `cam`, by value, which has passed pih_render_cam's test (the kernel's
//             own test of it costs nothing measurable: profiles/camera_refactor_bench.txt, profiles/scene_share_bench.txt)
// Mapping: grid = (strips, envs), 256 threads (4 waves).  The kernel is two calls of pih_fly_render.h:
// fly::camera_setup (pose and camera row, camera_or_preset, the scene's two phases in LDS; with fly::NoLight) and fly::render_image (the
// tile walk render_strip in the format FMT, one pixel per lane: a wave instruction stores 256 contiguous bytes of an image row in the two
// packed formats, 1 KB in float4); pih_lit_fly_kernel (pih_lit.hip) is the same two calls with the light hooked in.
#include <hip/hip_runtime.h>
#include "pih_fly_render.h"
#include "pih_launch.h"

using namespace pih;

template <int FMT> __global__ void __launch_bounds__(RENDER_THREADS) pih_fly_image_kernel(const float* __restrict__ state, void* __restrict__ out, fly::FlyCam cam,
                                                                                           const float* __restrict__ cam_dev, int n, int object, int env_begin,
                                                                                           int W, int H, int rows_per_strip, int flags) {
  using namespace fly;
  __shared__ FlyScene sc;
  __shared__ int cam_bad;
  const int tid = threadIdx.x, e = blockIdx.y;
  const int r0 = blockIdx.x * rows_per_strip, r1 = min(H, r0 + rows_per_strip);
  const bool bad = camera_setup(sc, cam_bad, NoLight(), state, cam, cam_dev, n, object, env_begin + e, e, flags, tid);
  render_image<FMT, unsigned>(sc, FlyGrid(sc, W, H), out, (size_t)e * H, W, r0, r1, tid, Pixels<FlyScene, unsigned>{sc, flags, bad});
}

namespace pih {
// called by pih_render_cam (pih_hip.hip), which has validated every argument; fmt = 0, PIH_RENDER_OUT_RGBA8 or PIH_RENDER_OUT_DEPTH
void fly_image_launch(int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                      int n, int object, int env_begin, int W, int H, int rows_per_strip, int flags) {
  fly::dispatch_fmt(fmt, [&](auto FMT) {
    hipLaunchKernelGGL(pih_fly_image_kernel<decltype(FMT)::value>, grid, dim3(RENDER_THREADS), 0, stream, state, out, cam, cam_dev, n, object, env_begin, W, H, rows_per_strip, flags);
  });
}
}  // namespace pih
