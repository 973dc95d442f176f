// TEST-ONLY: host build of the lit camera images of both tasks (peg_in_hole_gym_amd/csrc/pih_lit.h), real = PIH_REAL (double or float).
// Renders ONE env's state record the way pih_lit_view_kernel / pih_lit_fly_kernel (pih_lit.hip) do: camera and light are tested first, a
// degenerate one is replaced by its default and gives the background; then the product's per-scene and per-pixel code over the product's
// 16 x 64 tiling (pih_host_tiles.h), with the tile lists of the product's screen-bound test, and with the light-space table of the shadow ray on (lcull = 1)
// or off (lcull = 0: every occluder is intersected).
// tests/test_render_lit.py compiles it into a temporary directory (this file is not part of the Makefile's libraries).
#include "pih_host_platform.h"
#include "pih_wave_host.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_lit.h"
#include "pih_host_tiles.h"

using namespace pih;

extern "C" {

int pihl_real_bytes(void) { return (int)sizeof(real); }
int pihl_pack_byte(double v) { return (int)fly::pack_byte((real)v); }
// -> the code of light_degenerate; *what = the text pih_last_error carries for it (NULL for 0)
int pihl_light_degenerate(const float* words, const char** what) {
  static const char* const names[] = LIT_LIGHT_FIELD_NAMES;
  const int code = lit::light_degenerate(lit::light_words(words));
  if (what) *what = names[code];
  return code;
}

// rec: double[PIH_STATE_WORDS]; cam: float[PIH_CAM_WORDS]; light: float[PIH_LIGHT_WORDS]; out: double[H][W][4] = depth, r, g, b or NULL;
// rgba: uint8[H][W][4] = r, g, b, seg or NULL; depth: double[H][W] or NULL.  -> 16 x the code of light_degenerate + the code of
// cam_degenerate (0: both were used), -2 for bad arguments
int pihl_view_render(const double* rec, const float* cam_words, const float* light_words, int W, int H, int flags, int lcull, double* out, unsigned char* rgba, double* depth) {
  using namespace view;
  if (!rec || !cam_words || !light_words || W <= 0 || H <= 0) return -2;
  FlyCam cam;
  for (int i = 0; i < PIH_CAM_WORDS; i++) cam.w[i] = cam_words[i];
  const int code = fly::camera_or_preset(cam, FlyCam{PIH_VIEW_CAM_WRIST}, &flags);
  const lit::LightWords lw = lit::light_words(light_words);
  static Shared sh;
  static Wave w;
  for (int i = 0; i < PIH_STATE_WORDS; i++) sh.S[i] = (real)rec[i];
  fk_all(w, sh);
  ViewScene sc;
  lit::ViewLit le;
  // the phases of the workgroup's scene set-up, a barrier between them
  lit::light_setup(le, lw, all_prims());
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_poses(sh, sc, cam, flags, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) { scene_setup_bounds(sc, tid); lit::light_table(sc, le, tid); }
  const lit::LitPixels<ViewScene, lit::ViewLit, unsigned long long> p = {sc, le, lcull != 0, code != fly::CAM_OK || le.bad != lit::LIGHT_OK};
  host_tiles(sc, W, H, 1, 0ull, [&](unsigned long long prims, real xc, real yc, size_t px) { host_store(p, prims, xc, yc, px, out, rgba, depth); });
  return 16 * le.bad + code;
}

// rec: double[PIH_FLY_STATE_WORDS] (env-major record); the rest as above
int pihl_fly_render(const double* rec, const float* cam_words, const float* light_words, int object, int W, int H, int flags, int lcull, double* out, unsigned char* rgba, double* depth) {
  using namespace fly;
  if (!rec || !cam_words || !light_words || W <= 0 || H <= 0 || object < 0 || object >= PIH_FLY_NOBJ) return -2;
  FlyCam cam;
  for (int i = 0; i < PIH_CAM_WORDS; i++) cam.w[i] = cam_words[i];
  const int code = camera_or_preset(cam, FlyCam{PIH_FLY_CAM_DEFAULT});
  const lit::LightWords lw = lit::light_words(light_words);
  const FlyPose ps = load_fly_pose(rec, 0, 1);
  FlyScene sc;
  lit::FlyLit le;
  lit::light_setup(le, lw, all_prims(object));
  for (int tid = 0; tid < 16; tid++) scene_setup_poses(sc, ps, cam, object, flags, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) { scene_setup_bounds(sc, object, tid); lit::light_table(sc, le, tid); }
  const lit::LitPixels<FlyScene, lit::FlyLit, unsigned> p = {sc, le, lcull != 0, code != CAM_OK || le.bad != lit::LIGHT_OK};
  host_tiles(sc, W, H, 1, 0u, [&](unsigned prims, real xc, real yc, size_t px) { host_store(p, prims, xc, yc, px, out, rgba, depth); });
  return 16 * le.bad + code;
}

}  // extern "C"
