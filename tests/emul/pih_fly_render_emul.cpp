// TEST-ONLY: host build of the random-fly camera (peg_in_hole_gym_amd/csrc/pih_fly_render.h), real = PIH_REAL (double or float).
// Renders ONE env's state record with the product's per-scene and per-pixel code over the product's 16 x 64 tiling, either with every
// primitive on for every tile (cull = 0) or with the tile lists of the product's screen-bound test (cull = 1).
// tests/test_fly_render.py compiles it into a temporary directory (this file is not part of the Makefile's libraries).
#include "pih_host_platform.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_common.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_fly_render.h"

using namespace pih;
using namespace pih::fly;

extern "C" {

int pihfr_real_bytes(void) { return (int)sizeof(real); }

// rec: double[PIH_FLY_STATE_WORDS] (env-major record); cam: float[PIH_CAM_WORDS]; out: double[H][W][4] = depth, r, g, b
int pihfr_render(const double* rec, const float* cam_words, int object, int W, int H, int flags, int cull, double* out) {
  if (!rec || !cam_words || !out || W <= 0 || H <= 0 || object < 0 || object >= PIH_FLY_NOBJ) return -2;
  FlyCam cam;
  for (int i = 0; i < PIH_CAM_WORDS; i++) cam.w[i] = cam_words[i];
  FlyPose ps;
  for (int i = 0; i < RCAP; i++) ps.q[i] = (real)rec[PIH_F_Q + i];
  for (int i = 0; i < 3; i++) ps.opos[i] = (real)rec[PIH_F_OPOS + i];
  for (int i = 0; i < 4; i++) ps.oquat[i] = (real)rec[PIH_F_OQUAT + i];
  FlyScene sc;
  // the two phases of the workgroup's scene set-up, a barrier between them
  for (int tid = 0; tid < 16; tid++) scene_setup_poses(sc, ps, cam, object, flags, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) scene_setup_bounds(sc, object, tid);
  const FlyGrid g(sc, W, H);
  for (int i0 = 0; i0 < H; i0 += TILE_ROWS)
    for (int j0 = 0; j0 < W; j0 += TILE_COLS) {
      const int i1 = i0 + TILE_ROWS < H ? i0 + TILE_ROWS : H, j1 = j0 + TILE_COLS < W ? j0 + TILE_COLS : W;
      unsigned prims = all_prims(object);
      if (cull) {
        prims = 0;
        for (int lane = 0; lane < 32; lane++)    // (the kernel's ballot: lanes past FLY_NPRIM are off)
          if (prim_on_tile(sc, lane, g.xedge(j0), g.xedge(j1), g.yedge(i1), g.yedge(i0))) prims |= 1u << lane;
      }
      for (int i = i0; i < i1; i++)
        for (int j = j0; j < j1; j++) {
          const real4 c = shade(sc, prims, g.xc(j), g.yc(i), flags);
          double* o = out + ((size_t)i * W + j) * 4;
          o[0] = (double)c.x; o[1] = (double)c.y; o[2] = (double)c.z; o[3] = (double)c.w;
        }
    }
  return 0;
}

}  // extern "C"
