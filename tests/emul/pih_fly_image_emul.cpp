// TEST-ONLY: host build of the packed output formats and the camera test of the random-fly camera (peg_in_hole_gym_amd/csrc/
// pih_fly_render.h: pixel_rgba8, pixel_depth, pack_byte, seg_of_kind, cam_degenerate), real = PIH_REAL (double or float).
// Renders ONE env's state record the way pih_fly_image_kernel (pih_fly_image.hip) does: the camera is tested first, a degenerate one is
// replaced by the default camera and gives the background (camera_or_preset); then the product's per-pixel code over the product's 16 x 64
// tiling (pih_host_tiles.h), with
// every primitive on for every tile (cull = 0) or with the tile lists of the product's screen-bound test (cull = 1).
// tests/test_fly_image.py compiles it into a temporary directory (this file is not part of the Makefile's libraries).
#include "pih_host_platform.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_common.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_fly_render.h"
#include "pih_host_tiles.h"

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
  const int code = camera_or_preset(cam, FlyCam{PIH_FLY_CAM_DEFAULT});
  const FlyPose ps = load_fly_pose(rec, 0, 1);
  FlyScene sc;
  for (int tid = 0; tid < 16; tid++) scene_setup_poses(sc, ps, cam, object, flags, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_bounds(sc, object, tid);
  const Pixels<FlyScene, unsigned> p = {sc, flags, code != CAM_OK};
  host_tiles(sc, W, H, cull, all_prims(object), [&](unsigned prims, real xc, real yc, size_t px) { host_store(p, prims, xc, yc, px, nullptr, rgba, depth); });
  return code;
}

}  // extern "C"
