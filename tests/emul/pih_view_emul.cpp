// TEST-ONLY: host build of the free camera of the peg-in-hole task (peg_in_hole_gym_amd/csrc/pih_view.h), real = PIH_REAL (double or
// float).  Renders ONE env's state record the way pih_view_kernel (pih_view.hip) does: the camera is tested first, a degenerate one is
// replaced by the wrist preset and gives the background; forward kinematics with the host wave layer's fk_all; then the product's
// per-scene and per-pixel code over the product's 16 x 64 tiling, with every primitive on for every tile (cull = 0) or with the tile lists
// of the product's screen-bound test (cull = 1).
// tests/test_peg_view.py compiles it into a temporary directory (this file is not part of the Makefile's libraries).
#include "pih_host_platform.h"
#include "pih_wave_host.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_view.h"

using namespace pih;
using namespace pih::view;

extern "C" {

int pihv_real_bytes(void) { return (int)sizeof(real); }
int pihv_pack_byte(double v) { return (int)fly::pack_byte((real)v); }

// rec: double[PIH_STATE_WORDS]; cam: float[PIH_CAM_WORDS]; out: double[H][W][4] = depth, r, g, b or NULL; rgba: uint8[H][W][4] = r, g, b,
// seg or NULL; depth: double[H][W] or NULL.  -> the code of cam_degenerate (0: the camera was used), -2 for bad arguments
int pihv_render(const double* rec, const float* cam_words, int W, int H, int flags, int cull, double* out, unsigned char* rgba, double* depth) {
  if (!rec || !cam_words || W <= 0 || H <= 0) return -2;
  FlyCam cam;
  for (int i = 0; i < PIH_CAM_WORDS; i++) cam.w[i] = cam_words[i];
  const int code = fly::cam_degenerate(cam.w);
  if (code != fly::CAM_OK) { cam = FlyCam{PIH_VIEW_CAM_WRIST}; flags = (flags & ~PIH_RENDER_CAM_EE) | PIH_RENDER_CAM_EE_POS; }
  const bool bad = code != fly::CAM_OK;
  static Shared sh;
  static Wave w;
  for (int i = 0; i < PIH_STATE_WORDS; i++) sh.S[i] = (real)rec[i];
  fk_all(w, sh);
  ViewScene sc;
  // the two phases of the workgroup's scene set-up, a barrier between them
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_poses(sh, sc, cam, flags, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_bounds(sc, tid);
  const FlyGrid g(sc, W, H);
  for (int i0 = 0; i0 < H; i0 += TILE_ROWS)
    for (int j0 = 0; j0 < W; j0 += TILE_COLS) {
      const int i1 = i0 + TILE_ROWS < H ? i0 + TILE_ROWS : H, j1 = j0 + TILE_COLS < W ? j0 + TILE_COLS : W;
      unsigned long long prims = all_prims();
      if (cull) {
        prims = 0;
        for (int lane = 0; lane < 64; lane++)      // (the kernel's ballot: lanes past VIEW_NPRIM are off)
          if (prim_on_tile(sc, lane, g.xedge(j0), g.xedge(j1), g.yedge(i1), g.yedge(i0))) prims |= 1ull << lane;
      }
      for (int i = i0; i < i1; i++)
        for (int j = j0; j < j1; j++) {
          const size_t px = (size_t)i * W + j;
          if (out) {
            const real4 c = pixel_float4(sc, prims, g.xc(j), g.yc(i), flags, bad);
            double* o = out + px * 4;
            o[0] = (double)c.x; o[1] = (double)c.y; o[2] = (double)c.z; o[3] = (double)c.w;
          }
          if (rgba) {
            const unsigned v = pixel_rgba8(sc, prims, g.xc(j), g.yc(i), flags, bad);
            for (int k = 0; k < 4; k++) rgba[4 * px + k] = (unsigned char)((v >> (8 * k)) & 255u);
          }
          if (depth) depth[px] = (double)pixel_depth(sc, prims, g.xc(j), g.yc(i), bad);
        }
    }
  return code;
}

}  // extern "C"
