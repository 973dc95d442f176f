// TEST-ONLY: host build of the packed output formats and the camera test of the random-fly camera (peg_in_hole_gym_amd/csrc/
// pih_fly_render.h: pixel_rgba8, pixel_depth, pack_byte, seg_of_kind, cam_degenerate), real = PIH_REAL (double or float).
// Renders ONE env's state record the way pih_fly_image_kernel (pih_fly_image.hip) does: the camera is tested first, a degenerate one is
// replaced by the default camera and gives the background; then the product's per-pixel code over the product's 16 x 64 tiling, with
// every primitive on for every tile (cull = 0) or with the tile lists of the product's screen-bound test (cull = 1).
// tests/test_fly_image.py compiles it into a temporary directory (this file is not part of the Makefile's libraries).
#include "pih_host_platform.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_common.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_fly_render.h"

using namespace pih;
using namespace pih::fly;

extern "C" {

int pihfi_real_bytes(void) { return (int)sizeof(real); }
int pihfi_pack_byte(double v) { return (int)pack_byte((real)v); }
int pihfi_seg_of_kind(int kind) { return (int)seg_of_kind(kind); }
int pihfi_kind(int which) { return which == 0 ? KIND_OBJECT : (which == 1 ? KIND_TABLE : KIND_NONE); }
int pihfi_cam_degenerate(const float* cam_words) { return cam_degenerate(cam_words); }

// rec: double[PIH_FLY_STATE_WORDS] (env-major record); cam: float[PIH_CAM_WORDS]; rgba: uint8[H][W][4] = r, g, b, seg or NULL;
// depth: double[H][W] or NULL.  -> the code of cam_degenerate (0: the camera was used), -2 for bad arguments
int pihfi_render(const double* rec, const float* cam_words, int object, int W, int H, int flags, int cull, unsigned char* rgba, double* depth) {
  if (!rec || !cam_words || W <= 0 || H <= 0 || object < 0 || object >= PIH_FLY_NOBJ) return -2;
  FlyCam cam;
  for (int i = 0; i < PIH_CAM_WORDS; i++) cam.w[i] = cam_words[i];
  const int code = cam_degenerate(cam.w);
  if (code != CAM_OK) cam = FlyCam{PIH_FLY_CAM_DEFAULT};
  const bool bad = code != CAM_OK;
  FlyPose ps;
  for (int i = 0; i < RCAP; i++) ps.q[i] = (real)rec[PIH_F_Q + i];
  for (int i = 0; i < 3; i++) ps.opos[i] = (real)rec[PIH_F_OPOS + i];
  for (int i = 0; i < 4; i++) ps.oquat[i] = (real)rec[PIH_F_OQUAT + i];
  FlyScene sc;
  for (int tid = 0; tid < 16; tid++) scene_setup_poses(sc, ps, cam, object, flags, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_bounds(sc, object, tid);
  const FlyGrid g(sc, W, H);
  for (int i0 = 0; i0 < H; i0 += TILE_ROWS)
    for (int j0 = 0; j0 < W; j0 += TILE_COLS) {
      const int i1 = i0 + TILE_ROWS < H ? i0 + TILE_ROWS : H, j1 = j0 + TILE_COLS < W ? j0 + TILE_COLS : W;
      unsigned prims = all_prims(object);
      if (cull) {
        prims = 0;
        for (int lane = 0; lane < 32; lane++)
          if (prim_on_tile(sc, lane, g.xedge(j0), g.xedge(j1), g.yedge(i1), g.yedge(i0))) prims |= 1u << lane;
      }
      for (int i = i0; i < i1; i++)
        for (int j = j0; j < j1; j++) {
          const size_t px = (size_t)i * W + j;
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
