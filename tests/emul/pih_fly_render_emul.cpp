// TEST-ONLY: host build of the random-fly camera (peg_in_hole_gym_amd/csrc/pih_fly_render.h), real = PIH_REAL (double or float).
// Renders ONE env's state record with the product's per-scene and per-pixel code over the product's 16 x 64 tiling (pih_host_tiles.h),
// either with every primitive on for every tile (cull = 0) or with the tile lists of the product's screen-bound test (cull = 1).
// tests/test_fly_render.py compiles it into a temporary directory (this file is not part of the Makefile's libraries).
#include "pih_host_platform.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_common.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_fly_render.h"
#include "pih_host_tiles.h"

using namespace pih;
using namespace pih::fly;

extern "C" {

int pihfr_real_bytes(void) { return (int)sizeof(real); }

// rec: double[PIH_FLY_STATE_WORDS] (env-major record); cam: float[PIH_CAM_WORDS]; out: double[H][W][4] = depth, r, g, b
int pihfr_render(const double* rec, const float* cam_words, int object, int W, int H, int flags, int cull, double* out) {
  if (!rec || !cam_words || !out || W <= 0 || H <= 0 || object < 0 || object >= PIH_FLY_NOBJ) return -2;
  FlyCam cam;
  for (int i = 0; i < PIH_CAM_WORDS; i++) cam.w[i] = cam_words[i];
  const FlyPose ps = load_fly_pose(rec, 0, 1);
  FlyScene sc;
  // the two phases of the workgroup's scene set-up, a barrier between them
  for (int tid = 0; tid < 16; tid++) scene_setup_poses(sc, ps, cam, object, flags, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_bounds(sc, object, tid);
  host_tiles(sc, W, H, cull, all_prims(object), [&](unsigned prims, real xc, real yc, size_t px) {
    const real4 c = shade(sc, prims, xc, yc, flags);
    double* o = out + px * 4;
    o[0] = (double)c.x; o[1] = (double)c.y; o[2] = (double)c.z; o[3] = (double)c.w;
  });
  return 0;
}

}  // extern "C"
