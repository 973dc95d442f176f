// pih_lit.hip -- lit camera images of both tasks (pih_lit.h; pih_render_lit of include/pih_render_light.h).  A translation unit of its own, for the
// reason pih_fly_image.hip states: tools/isa_fingerprint.py is to show every older kernel unchanged.
//   FMT        0: float4 (depth, r, g, b) | PIH_RENDER_OUT_RGBA8: one 32-bit word (r, g, b, seg) | PIH_RENDER_OUT_DEPTH: one float
//   cam_dev    as in pih_fly_image_kernel / pih_view_kernel
//   light_dev  != nullptr (PIH_RENDER_LIGHT_DEVICE): float[count, PIH_LIGHT_WORDS], row blockIdx.y is this workgroup's light -- 11
//              wave-uniform loads by the thread that tests it; nullptr: `light`, by value
// Mapping as those two kernels, and their two calls: the task's camera_setup (pih_view.h, pih_fly_render.h) with lit::LightHook in the
// place of fly::NoLight -- thread 14 of the workgroup reads and tests the light (light_degenerate), builds its frame in LDS and replaces a
// degenerate one by the default, so that everything stays finite; the threads that compute the screen bounds then fill the light-space
// table of the shadow ray (pih_lit.h) -- and fly::render_image with lit::LitPixels (ballot tile lists for the primary ray).  An env whose
// camera or light is degenerate gets the background.
// pih_lit_fly_kernel is those two calls.  pih_lit_view_kernel keeps its set-up and its walk written out, as they were before the shared
// pieces existed: on the shared pieces its rgba8 instance measured 1.0 - 1.1 % slower at 4096 envs (14.77 against 14.60 ms), more than
// the old code's own spread (profiles/camera_refactor_bench.txt), with equal registers and +29 instructions; written out, the three
// instances are instruction for instruction what they were.  A change to render_strip or view::camera_setup has to be made here too.
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
  const int tid = threadIdx.x, e = blockIdx.y, env = env_begin + e;
  const int r0 = blockIdx.x * rows_per_strip, r1 = min(H, r0 + rows_per_strip);
  Wave w; w.l = tid; w.counter = 0;
  const float* rec = state + (size_t)env * PIH_STATE_WORDS;
  for (int i = tid; i < PIH_STATE_WORDS; i += RENDER_THREADS) sh.S[i] = rec[i];
  __syncthreads();
  fk_all(w, sh);
  __syncthreads();
  if (tid == 15) {
    if (cam_dev) {
#pragma unroll
      for (int i = 0; i < PIH_CAM_WORDS; i++) cam.w[i] = cam_dev[(size_t)e * PIH_CAM_WORDS + i];
    }
    const int code = fly::cam_degenerate(cam.w);
    cam_bad = code;
    if (code != fly::CAM_OK) { cam = FlyCam{PIH_VIEW_CAM_WRIST}; flags = (flags & ~PIH_RENDER_CAM_EE) | PIH_RENDER_CAM_EE_POS; }
  }
  if (tid == 14) {
    if (light_dev) {
#pragma unroll
      for (int i = 0; i < PIH_LIGHT_WORDS; i++) light.w[i] = reinterpret_cast<const unsigned*>(light_dev)[(size_t)e * PIH_LIGHT_WORDS + i];      // (as integers: pih_lit.h)
    }
    lit::light_setup(le, light, all_prims());
  }
  scene_setup_poses(sh, sc, cam, flags, tid);
  __syncthreads();
  scene_setup_bounds(sc, tid);
  lit::light_table(sc, le, tid);
  __syncthreads();
  const bool bad = cam_bad != fly::CAM_OK || le.bad != lit::LIGHT_OK;
  const FlyGrid g(sc, W, H);
  const size_t img0 = (size_t)e * H * W;
  const int lane = tid & 63, wave = tid >> 6;
  const int tcols = (W + TILE_COLS - 1) / TILE_COLS, trows = (r1 - r0 + TILE_ROWS - 1) / TILE_ROWS;
  for (int tile = wave; tile < tcols * trows; tile += RENDER_THREADS / 64) {
    const int ti = tile / tcols, tj = tile - ti * tcols;
    const int i0 = r0 + ti * TILE_ROWS, i1 = min(r1, i0 + TILE_ROWS), j0 = tj * TILE_COLS, j1 = min(W, j0 + TILE_COLS);
    const unsigned long long prims = __ballot(prim_on_tile(sc, lane, g.xedge(j0), g.xedge(j1), g.yedge(i1), g.yedge(i0)));
    const int j = j0 + lane;
    if (j < j1) {
      const float xc = g.xc(j);
      for (int i = i0; i < i1; i++) {
        const size_t px = img0 + (size_t)i * W + j;
        if (FMT == PIH_RENDER_OUT_RGBA8) {
          static_cast<unsigned*>(out)[px] = lit::pixel_rgba8(sc, le, prims, xc, g.yc(i), true, bad);
        } else if (FMT == PIH_RENDER_OUT_DEPTH) {
          static_cast<float*>(out)[px] = lit::pixel_depth(sc, prims, xc, g.yc(i), bad);
        } else {
          const real4 c = lit::pixel_float4(sc, le, prims, xc, g.yc(i), true, bad);
          static_cast<float4*>(out)[px] = make_float4(c.x, c.y, c.z, c.w);
        }
      }
    }
  }
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
