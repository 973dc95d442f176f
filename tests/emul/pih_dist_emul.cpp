// TEST-ONLY: host build of the batched closest-point queries (peg_in_hole_gym_amd/csrc/pih_dist.h), real = PIH_REAL (double or float).
// Answers n queries against ONE env's state record the way pih_dist_view_kernel / pih_dist_fly_kernel (pih_dist.hip) do: forward
// kinematics with the host wave layer's fk_all (peg-in-hole) or the pose words (random-fly), the ray tests' scene set-up without a camera,
// then the product's per-query code.  tests/test_dist.py compiles it into a temporary directory (this file is not part of the Makefile's
// libraries); pih_dist_sanitize_main.cpp includes it.
#include "pih_host_platform.h"
#include "pih_wave_host.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_dist.h"

using namespace pih;

extern "C" {

int pihdist_real_bytes(void) { return (int)sizeof(real); }

static int bad_args(const void* rec, const void* words, const void* out, int n, int flags, int groups) {
  return !rec || !words || !out || n < 0 || (flags & ~PIH_RAY_FRAME_EE) || (groups & ~PIH_GROUP_ALL);
}

// rec: double[PIH_STATE_WORDS]; words: float[n][PIH_POINT_WORDS]; flags: PIH_RAY_FRAME_EE; groups: PIH_GROUP_*; cull: skip the primitives
// whose bounding sphere is out of reach (what the kernels do) or call every distance function; out: double[n][PIH_CLOSEST_WORDS].
// -> 0, -2 for bad arguments
int pihdist_view(const double* rec, const float* words, int n, int flags, int groups, int cull, double* out) {
  if (bad_args(rec, words, out, n, flags, groups)) return -2;
  static Shared sh;
  static Wave w;
  for (int i = 0; i < PIH_STATE_WORDS; i++) sh.S[i] = (real)rec[i];
  fk_all(w, sh);
  view::ViewScene sc;
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::view_setup_poses(sh, sc, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::view_setup_balls(sc, tid);
  const unsigned long long prims = dist::view_prims(groups);
  for (int r = 0; r < n; r++) {
    const float* q = words + (size_t)r * PIH_POINT_WORDS;
    const dist::Record o = cull ? dist::view_record<true>(sc, q, flags, prims) : dist::view_record<false>(sc, q, flags, prims);
    for (int k = 0; k < PIH_CLOSEST_WORDS; k++) out[(size_t)r * PIH_CLOSEST_WORDS + k] = (double)o.w[k];
  }
  return 0;
}

// rec: double[PIH_FLY_STATE_WORDS] (env-major record); the rest as above
int pihdist_fly(const double* rec, int object, const float* words, int n, int flags, int groups, int cull, double* out) {
  if (bad_args(rec, words, out, n, flags, groups) || object < 0 || object >= PIH_FLY_NOBJ) return -2;
  const fly::FlyPose ps = fly::load_fly_pose(rec, 0, 1);
  fly::FlyScene sc;
  for (int tid = 0; tid < 16; tid++) rays::fly_setup_poses(sc, ps, object, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::fly_setup_balls(sc, tid);
  const unsigned prims = dist::fly_prims(object, groups);
  for (int r = 0; r < n; r++) {
    const float* q = words + (size_t)r * PIH_POINT_WORDS;
    const dist::Record o = cull ? dist::fly_record<true>(sc, q, flags, prims) : dist::fly_record<false>(sc, q, flags, prims);
    for (int k = 0; k < PIH_CLOSEST_WORDS; k++) out[(size_t)r * PIH_CLOSEST_WORDS + k] = (double)o.w[k];
  }
  return 0;
}

}  // extern "C"
