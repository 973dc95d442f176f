// pih_lit.hip -- lit camera images of both tasks (pih_lit.h; pih_render_lit of include/pih_render_light.h).
//   FMT        0: float4 (depth, r, g, b) | PIH_RENDER_OUT_RGBA8: one 32-bit word (r, g, b, seg) | PIH_RENDER_OUT_DEPTH: one float
//   cam_dev    as in pih_fly_image_kernel / pih_view_kernel
//   light_dev  != nullptr (PIH_RENDER_LIGHT_DEVICE): float[count, PIH_LIGHT_WORDS], row blockIdx.y is this workgroup's light -- 11
//              wave-uniform loads by the thread that tests it; nullptr: `light`, by value
// Mapping as those two kernels, and their two calls: the task's camera_setup (pih_view.h, pih_fly_render.h) with lit::LightHook in the
// place of fly::NoLight -- thread 14 of the workgroup reads and tests the light (light_degenerate), builds its frame in LDS and replaces a
// degenerate one by the default, so that everything stays finite; the threads that compute the screen bounds then fill the light-space
// table of the shadow ray (pih_lit.h) -- and fly::render_image with lit::LitPixels (ballot tile lists for the primary ray).  An env whose
// camera or light is degenerate gets the background.
// Both kernels are those two calls.  Their images are held to the bits of tests/golden/scene_bits.npz (tests/test_gpu_scene_bits.py) and
// their times to a measurement against the build before (profiles/scene_share_bench.txt).
#include <hip/hip_runtime.h>
#include "pih_lit.h"
#include "pih_launch.h"

using namespace pih;

template <int FMT> __global__ void __launch_bounds__(RENDER_THREADS) pih_lit_view_kernel(const float* __restrict__ state, void* __restrict__ out, fly::FlyCam cam,
                                                                                          const float* __restrict__ cam_dev, lit::LightWords light,
                                                                                          const float* __restrict__ light_dev, int env_begin, int W, int H,
                                                                                          int rows_per_strip, int flags) {
  using namespace view;
  __shared__ Shared sh;
  __shared__ ViewScene sc;
  __shared__ lit::ViewLit le;
  __shared__ int cam_bad;
  const int tid = threadIdx.x, e = blockIdx.y;
  const int r0 = blockIdx.x * rows_per_strip, r1 = min(H, r0 + rows_per_strip);
  const bool bad = camera_setup(sh, sc, cam_bad, lit::LightHook<lit::ViewLit>{le, light, light_dev, e}, state, cam, cam_dev, env_begin + e, e, flags, tid);
  fly::render_image<FMT, unsigned long long>(sc, FlyGrid(sc, W, H), out, (size_t)e * H, W, r0, r1, tid, lit::LitPixels<ViewScene, lit::ViewLit, unsigned long long>{sc, le, true, bad});
}

template <int FMT> __global__ void __launch_bounds__(RENDER_THREADS) pih_lit_fly_kernel(const float* __restrict__ state, void* __restrict__ out, fly::FlyCam cam,
                                                                                         const float* __restrict__ cam_dev, lit::LightWords light,
                                                                                         const float* __restrict__ light_dev, int n, int object, int env_begin,
                                                                                         int W, int H, int rows_per_strip, int flags) {
  using namespace fly;
  __shared__ FlyScene sc;
  __shared__ lit::FlyLit le;
  __shared__ int cam_bad;
  const int tid = threadIdx.x, e = blockIdx.y;
  const int r0 = blockIdx.x * rows_per_strip, r1 = min(H, r0 + rows_per_strip);
  const bool bad = camera_setup(sc, cam_bad, lit::LightHook<lit::FlyLit>{le, light, light_dev, e}, state, cam, cam_dev, n, object, env_begin + e, e, flags, tid);
  render_image<FMT, unsigned>(sc, FlyGrid(sc, W, H), out, (size_t)e * H, W, r0, r1, tid, lit::LitPixels<FlyScene, lit::FlyLit, unsigned>{sc, le, true, bad});
}

namespace pih {
// the host's test of a light it can read -> 0, or light_degenerate's code and in *what the text for pih_last_error
int lit_light_check(const float* words, const char** what) {
  static const char* const names[] = LIT_LIGHT_FIELD_NAMES;
  const int code = lit::light_degenerate(lit::light_words(words));
  *what = names[code];
  return code;
}
// called by pih_render_lit (pih_hip.hip), which has validated every argument; fmt = 0, PIH_RENDER_OUT_RGBA8 or PIH_RENDER_OUT_DEPTH;
// light: PIH_LIGHT_WORDS floats on the host (used unless light_dev is set)
void lit_launch(bool fly_task, int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                const float* light, const float* light_dev, int n, int object, int env_begin, int W, int H, int rows_per_strip, int flags) {
  const lit::LightWords lw = lit::light_words(light);
  fly::dispatch_fmt(fmt, [&](auto FMT) {
    if (fly_task)
      hipLaunchKernelGGL(pih_lit_fly_kernel<decltype(FMT)::value>, grid, dim3(RENDER_THREADS), 0, stream, state, out, cam, cam_dev, lw, light_dev, n, object, env_begin, W, H, rows_per_strip, flags);
    else
      hipLaunchKernelGGL(pih_lit_view_kernel<decltype(FMT)::value>, grid, dim3(RENDER_THREADS), 0, stream, state, out, cam, cam_dev, lw, light_dev, env_begin, W, H, rows_per_strip, flags);
  });
}
}  // namespace pih
