// pih_view.hip -- the free camera of the peg-in-hole task (pih_view.h; pih_render_view of include/pih_render_view.h).  A translation unit of its own,
// for the reason pih_fly_image.hip states: tools/isa_fingerprint.py is to show every older kernel unchanged.
//   FMT       0: float4 (depth, r, g, b) | PIH_RENDER_OUT_RGBA8: one 32-bit word (r, g, b, seg) | PIH_RENDER_OUT_DEPTH: one float
//   cam_dev   != nullptr (PIH_RENDER_CAM_DEVICE): float[count, PIH_CAM_WORDS], row blockIdx.y is this workgroup's camera -- 13 wave-uniform
//             loads; nullptr: `cam`, by value
// Mapping as pih_render_kernel and pih_fly_image_kernel: grid = (strips, envs), 256 threads (4 waves); the env's state record goes to LDS,
// fk_all runs once per workgroup, the scene and the camera are built once per workgroup in LDS, tile lists by 64-bit ballot.  The thread
// that builds the camera basis tests the camera first (cam_degenerate); a degenerate one is replaced by the wrist preset, so that the
// scene stays finite, and every pixel of the env gets the background.  One pixel per lane: a wave instruction stores 256 contiguous bytes
// of an image row in the two packed formats (1 KB in float4).
#include <hip/hip_runtime.h>
#include "pih_view.h"

using namespace pih;

template <int FMT> __global__ void __launch_bounds__(RENDER_THREADS) pih_view_kernel(const float* __restrict__ state, void* __restrict__ out, fly::FlyCam cam,
                                                                                      const float* __restrict__ cam_dev, int env_begin, int W, int H,
                                                                                      int rows_per_strip, int flags) {
  using namespace view;
  __shared__ Shared sh;
  __shared__ ViewScene sc;
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
  scene_setup_poses(sh, sc, cam, flags, tid);
  __syncthreads();
  scene_setup_bounds(sc, tid);
  __syncthreads();
  const bool bad = cam_bad != fly::CAM_OK;
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
          static_cast<unsigned*>(out)[px] = pixel_rgba8(sc, prims, xc, g.yc(i), flags, bad);
        } else if (FMT == PIH_RENDER_OUT_DEPTH) {
          static_cast<float*>(out)[px] = pixel_depth(sc, prims, xc, g.yc(i), bad);
        } else {
          const real4 c = pixel_float4(sc, prims, xc, g.yc(i), flags, bad);
          static_cast<float4*>(out)[px] = make_float4(c.x, c.y, c.z, c.w);
        }
      }
    }
  }
}

namespace pih {
// called by pih_render_view (pih_hip.hip), which has validated every argument; fmt = 0, PIH_RENDER_OUT_RGBA8 or PIH_RENDER_OUT_DEPTH
void view_launch(int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                 int env_begin, int W, int H, int rows_per_strip, int flags) {
#define PIH_VIEW(FMT) hipLaunchKernelGGL(pih_view_kernel<FMT>, grid, dim3(RENDER_THREADS), 0, stream, state, out, cam, cam_dev, env_begin, W, H, rows_per_strip, flags)
  if (fmt == PIH_RENDER_OUT_RGBA8) PIH_VIEW(PIH_RENDER_OUT_RGBA8);
  else if (fmt == PIH_RENDER_OUT_DEPTH) PIH_VIEW(PIH_RENDER_OUT_DEPTH);
  else PIH_VIEW(0);
#undef PIH_VIEW
}
}  // namespace pih
