// pih_view.hip -- the free camera of the peg-in-hole task (pih_view.h; pih_render_view of include/pih_render_view.h).  A translation unit of its own
// beside pih_peg.hip, whose step kernel's code is held by tools/isa_fingerprint.py; this kernel is held by tests/test_gpu_scene_bits.py.
//   FMT       0: float4 (depth, r, g, b) | PIH_RENDER_OUT_RGBA8: one 32-bit word (r, g, b, seg) | PIH_RENDER_OUT_DEPTH: one float
//   cam_dev   != nullptr (PIH_RENDER_CAM_DEVICE): float[count, PIH_CAM_WORDS], row blockIdx.y is this workgroup's camera -- 13 wave-uniform
//             loads; nullptr: `cam`, by value
// Mapping as pih_render_kernel and pih_fly_image_kernel: grid = (strips, envs), 256 threads (4 waves).  The kernel is two calls:
// view::camera_setup (pih_view.h: state record -> LDS, fk_all, camera row and fly::camera_or_preset with the wrist preset, the scene's two
// phases; with fly::NoLight) and fly::render_image (pih_fly_render.h: the tile walk render_strip with a 64-bit ballot, in the format FMT);
// pih_lit_view_kernel (pih_lit.hip) is the same two calls with the light hooked in.
#include <hip/hip_runtime.h>
#include "pih_view.h"
#include "pih_launch.h"

using namespace pih;

template <int FMT> __global__ void __launch_bounds__(RENDER_THREADS) pih_view_kernel(const float* __restrict__ state, void* __restrict__ out, fly::FlyCam cam,
                                                                                      const float* __restrict__ cam_dev, int env_begin, int W, int H,
                                                                                      int rows_per_strip, int flags) {
  using namespace view;
  __shared__ Shared sh;
  __shared__ ViewScene sc;
  __shared__ int cam_bad;
  const int tid = threadIdx.x, e = blockIdx.y;
  const int r0 = blockIdx.x * rows_per_strip, r1 = min(H, r0 + rows_per_strip);
  const bool bad = camera_setup(sh, sc, cam_bad, fly::NoLight(), state, cam, cam_dev, env_begin + e, e, flags, tid);
  fly::render_image<FMT, unsigned long long>(sc, FlyGrid(sc, W, H), out, (size_t)e * H, W, r0, r1, tid, fly::Pixels<ViewScene, unsigned long long>{sc, flags, bad});
}

namespace pih {
// called by pih_render_view (pih_hip.hip), which has validated every argument; fmt = 0, PIH_RENDER_OUT_RGBA8 or PIH_RENDER_OUT_DEPTH
void view_launch(int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                 int env_begin, int W, int H, int rows_per_strip, int flags) {
  fly::dispatch_fmt(fmt, [&](auto FMT) {
    hipLaunchKernelGGL(pih_view_kernel<decltype(FMT)::value>, grid, dim3(RENDER_THREADS), 0, stream, state, out, cam, cam_dev, env_begin, W, H, rows_per_strip, flags);
  });
}
}  // namespace pih
