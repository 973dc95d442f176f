// TEST-ONLY: host build of the free camera of the peg-in-hole task (peg_in_hole_gym_amd/csrc/pih_view.h), real = PIH_REAL (double or
// float).  Renders ONE env's state record the way pih_view_kernel (pih_view.hip) does: the camera is tested first, a degenerate one is
// replaced by the wrist preset and gives the background (camera_or_preset); forward kinematics with the host wave layer's fk_all; then the product's
// per-scene and per-pixel code over the product's 16 x 64 tiling (pih_host_tiles.h), with every primitive on for every tile (cull = 0) or with the tile lists
// of the product's screen-bound test (cull = 1).
// tests/test_peg_view.py compiles it into a temporary directory (this file is not part of the Makefile's libraries).
#include "pih_host_platform.h"
#include "pih_wave_host.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_view.h"
#include "pih_host_tiles.h"

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
  const int code = fly::camera_or_preset(cam, FlyCam{PIH_VIEW_CAM_WRIST}, &flags);
  static Shared sh;
  static Wave w;
  for (int i = 0; i < PIH_STATE_WORDS; i++) sh.S[i] = (real)rec[i];
  fk_all(w, sh);
  ViewScene sc;
  // the two phases of the workgroup's scene set-up, a barrier between them
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_poses(sh, sc, cam, flags, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_bounds(sc, tid);
  const fly::Pixels<ViewScene, unsigned long long> p = {sc, flags, code != fly::CAM_OK};
  host_tiles(sc, W, H, cull, all_prims(), [&](unsigned long long prims, real xc, real yc, size_t px) { host_store(p, prims, xc, yc, px, out, rgba, depth); });
  return code;
}

}  // extern "C"
