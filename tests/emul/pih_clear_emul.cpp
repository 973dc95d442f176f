// TEST-ONLY: host build of the robot clearance queries (peg_in_hole_gym_amd/csrc/pih_clear.h), real = PIH_REAL (double or float).
// Answers C joint configurations against ONE env's state record the way pih_clear_view_kernel / pih_clear_fly_kernel (pih_clear.hip) do:
// forward kinematics of the state with the host wave layer's fk_all (peg-in-hole) or the pose words (random-fly), the ray tests' scene
// set-up without a camera, then the product's per-configuration code, one configuration after the other, all its probes.
// tests/test_clear.py compiles it into a temporary directory (this file is not part of the Makefile's libraries);
// pih_clear_sanitize_main.cpp includes it.
#include "pih_host_platform.h"
#include "pih_wave_host.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_clear.h"

using namespace pih;

template <class Rb, class F> static void walk(const float* q, const float* own, int C, double* out, const F& record) {
  for (int c = 0; c < C; c++) {
    const float* w = q ? q + (size_t)c * Rb::ND : own;
    real qv[Rb::ND];
    const bool ok = clear::load_q<Rb>(w, qv);
    clear::Probes<Rb::NP> P;
    clear::place_probes<Rb>(qv, ok, P);
    for (int p = 0; p < Rb::NP; p++) {
      const clear::Record o = record(P, ok, p);
      for (int k = 0; k < clear::CW; k++) out[((size_t)c * Rb::NP + p) * clear::CW + k] = (double)o.w[k];
    }
  }
}

extern "C" {

int pihclear_real_bytes(void) { return (int)sizeof(real); }
int pihclear_probes(int task) { return task ? clear::Ur5Robot::NP : clear::PandaRobot::NP; }

static int bad_args(const void* rec, const void* out, int C, int groups, double reach) {
  return !rec || !out || C < 0 || (groups & ~(PIH_GROUP_OBJECT | PIH_GROUP_TABLE)) || !groups || !(reach > 0);
}

// rec: double[PIH_STATE_WORDS]; q: float[C][9], or NULL with C == 1: the record's own joint words; groups: PIH_GROUP_OBJECT | PIH_GROUP_TABLE;
// cull: skip the obstacles whose bounding sphere is out of reach (what the kernels can do) or call every distance function;
// out: double[C][11][PIH_CLEAR_WORDS].  -> 0, -2 for bad arguments
int pihclear_view(const double* rec, const float* q, int C, int groups, double reach, int cull, double* out) {
  if (bad_args(rec, out, C, groups, reach) || (!q && C != 1)) return -2;
  static Shared sh;
  static Wave w;
  for (int i = 0; i < PIH_STATE_WORDS; i++) sh.S[i] = (real)rec[i];
  fk_all(w, sh);
  static view::ViewScene sc;
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::view_setup_poses(sh, sc, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::view_setup_balls(sc, tid);
  float own[clear::PandaRobot::ND];
  for (int i = 0; i < clear::PandaRobot::ND; i++) own[i] = (float)rec[PIH_S_QARM + i];
  walk<clear::PandaRobot>(q, own, C, out, [&](const clear::Probes<clear::PandaRobot::NP>& P, bool ok, int p) {
    return cull ? clear::view_record<true>(sc, P, ok, p, (real)reach, groups) : clear::view_record<false>(sc, P, ok, p, (real)reach, groups);
  });
  return 0;
}

// rec: double[PIH_FLY_STATE_WORDS] (env-major record); q: float[C][6] or NULL; out: double[C][6][PIH_CLEAR_WORDS]; the rest as above
int pihclear_fly(const double* rec, int object, const float* q, int C, int groups, double reach, int cull, double* out) {
  if (bad_args(rec, out, C, groups, reach) || (!q && C != 1) || object < 0 || object >= PIH_FLY_NOBJ) return -2;
  const fly::FlyPose ps = fly::load_fly_pose(rec, 0, 1);
  static fly::FlyScene sc;
  for (int tid = 0; tid < 16; tid++) rays::fly_setup_poses(sc, ps, object, tid);
  for (int tid = 0; tid < RENDER_THREADS; tid++) rays::fly_setup_balls(sc, tid);
  const int nsph = fly::R_NSPH[object];
  float own[clear::Ur5Robot::ND];
  for (int i = 0; i < clear::Ur5Robot::ND; i++) own[i] = (float)rec[PIH_F_Q + i];
  walk<clear::Ur5Robot>(q, own, C, out, [&](const clear::Probes<clear::Ur5Robot::NP>& P, bool ok, int p) {
    return cull ? clear::fly_record<true>(sc, nsph, P, ok, p, (real)reach, groups) : clear::fly_record<false>(sc, nsph, P, ok, p, (real)reach, groups);
  });
  return 0;
}

}  // extern "C"
