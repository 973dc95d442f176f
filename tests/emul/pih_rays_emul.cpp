// TEST-ONLY: host build of the batched ray tests (peg_in_hole_gym_amd/csrc/pih_rays.h), real = PIH_REAL (double or float).  Traces n rays
// against ONE env's state record the way pih_ray_view_kernel / pih_ray_fly_kernel (pih_rays.hip) do: forward kinematics with the host
// wave layer's fk_all (peg-in-hole) or the pose words (random-fly), the product's scene set-up without a camera, then the product's
// per-ray code.  tests/test_rays.py compiles it into a temporary directory (this file is not part of the Makefile's libraries);
// pih_rays_sanitize_main.cpp includes it.
#include "pih_host_platform.h"
#include "pih_wave_host.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_rays.h"

using namespace pih;

extern "C" {

int pihray_real_bytes(void) { return (int)sizeof(real); }

// rec: double[PIH_STATE_WORDS]; ray_words: float[n][PIH_RAY_WORDS]; flags: PIH_RAY_FRAME_EE | PIH_RAY_IGNORE_ROBOT; cull: skip the primitives
// whose bounding sphere the ray misses (what the kernels do) or call every primitive function; out: double[n][PIH_RAY_HIT_WORDS].
// -> 0, -2 for bad arguments
int pihray_view(const double* rec, const float* ray_words, int n, int flags, int cull, double* out) {
  if (!rec || !ray_words || !out || n < 0 || (flags & ~(PIH_RAY_FRAME_EE | PIH_RAY_IGNORE_ROBOT))) return -2;
  static Shared sh;
  static Wave w;
  for (int i = 0; i < PIH_STATE_WORDS; i++) sh.S[i] = (real)rec[i];
  fk_all(w, sh);
  view::ViewScene sc;
  // the two phases of the workgroup's scene set-up, a barrier between them
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::view_setup_poses(sh, sc, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::view_setup_balls(sc, tid);
  for (int r = 0; r < n; r++) {
    const float* ray = ray_words + (size_t)r * PIH_RAY_WORDS;
    const rays::Record o = cull ? rays::view_record<true>(sc, ray, flags) : rays::view_record<false>(sc, ray, flags);
    for (int k = 0; k < PIH_RAY_HIT_WORDS; k++) out[(size_t)r * PIH_RAY_HIT_WORDS + k] = (double)o.w[k];
  }
  return 0;
}

// rec: double[PIH_FLY_STATE_WORDS] (env-major record); the rest as above
int pihray_fly(const double* rec, int object, const float* ray_words, int n, int flags, int cull, double* out) {
  if (!rec || !ray_words || !out || n < 0 || object < 0 || object >= PIH_FLY_NOBJ || (flags & ~(PIH_RAY_FRAME_EE | PIH_RAY_IGNORE_ROBOT))) return -2;
  const fly::FlyPose ps = fly::load_fly_pose(rec, 0, 1);
  fly::FlyScene sc;
  for (int tid = 0; tid < 16; tid++) rays::fly_setup_poses(sc, ps, object, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::fly_setup_balls(sc, tid);
  for (int r = 0; r < n; r++) {
    const float* ray = ray_words + (size_t)r * PIH_RAY_WORDS;
    const rays::Record o = cull ? rays::fly_record<true>(sc, object, ray, flags) : rays::fly_record<false>(sc, object, ray, flags);
    for (int k = 0; k < PIH_RAY_HIT_WORDS; k++) out[(size_t)r * PIH_RAY_HIT_WORDS + k] = (double)o.w[k];
  }
  return 0;
}

}  // extern "C"
