// TEST-ONLY: host build of the batched robot-model queries (peg_in_hole_gym_amd/csrc/pih_robot.h), real = PIH_REAL (double or float).
// One problem after the other through the product's per-lane code, the way the lanes of pih_robot.hip run it; arguments and results
// cross the boundary as double.  tests/emul/robot_emul.py compiles it (this file is not part of the Makefile's libraries);
// pih_robot_sanitize_main.cpp includes it into a stand-alone program.
#include "pih_host_platform.h"
#include "../../peg_in_hole_gym_amd/csrc/pih_robot.h"

using namespace pih;
using namespace pih::robot;

namespace {
template <int N> void load(const double* p, int i, real* v) { for (int k = 0; k < N; k++) v[k] = (real)p[(size_t)i * N + k]; }
template <int N> void store(double* p, int i, const real* v) { for (int k = 0; k < N; k++) p[(size_t)i * N + k] = (double)v[k]; }

template <class Rb> void fk_t(int n, const double* q, const double* qd, double* out) {
  for (int i = 0; i < n; i++) {
    real qv[Rb::ND], qdv[Rb::ND], rows[Rb::NF * LSW];
    load<Rb::ND>(q, i, qv);
    for (int k = 0; k < Rb::ND; k++) qdv[k] = qd ? (real)qd[(size_t)i * Rb::ND + k] : (real)0;
    fk_states<Rb>(qv, qdv, mk(0, 0, 0), rows);
    store<Rb::NF * LSW>(out, i, rows);
  }
}
template <class Rb> void jac_t(int n, const double* q, int frame, const double* lp, double* out) {
  for (int i = 0; i < n; i++) {
    real qv[Rb::ND], rows[6 * Rb::ND];
    load<Rb::ND>(q, i, qv);
    const V3 l = lp ? mk((real)lp[3 * i], (real)lp[3 * i + 1], (real)lp[3 * i + 2]) : mk(0, 0, 0);
    jacobian<Rb>(qv, frame, l, rows);
    store<6 * Rb::ND>(out, i, rows);
  }
}
template <class Rb> void mass_t(int n, const double* q, double* out) {
  for (int i = 0; i < n; i++) {
    real qv[Rb::ND], rows[Rb::ND * Rb::ND];
    load<Rb::ND>(q, i, qv);
    mass_matrix<Rb>(qv, rows);
    store<Rb::ND * Rb::ND>(out, i, rows);
  }
}
template <class Rb> void invdyn_t(int n, const double* q, const double* qd, const double* qdd, double* tau) {
  for (int i = 0; i < n; i++) {
    real qv[Rb::ND], qdv[Rb::ND], qddv[Rb::ND], rows[Rb::ND];
    load<Rb::ND>(q, i, qv); load<Rb::ND>(qd, i, qdv); load<Rb::ND>(qdd, i, qddv);
    inverse_dynamics<Rb>(qv, qdv, qddv, rows);
    store<Rb::ND>(tau, i, rows);
  }
}
}  // namespace

extern "C" {

int pihr_real_bytes(void) { return (int)sizeof(real); }
int pihr_dims(int robot, int* out) {
  if (robot == PIH_ROBOT_PANDA) { out[0] = Panda::ND; out[1] = Panda::NF; return 0; }
  if (robot == PIH_ROBOT_UR5) { out[0] = Ur5::ND; out[1] = Ur5::NF; return 0; }
  return -2;
}
int pihr_link_states_frames(int task) { return task == PIH_TASK_PEG_IN_HOLE ? PEG_FRAMES : (task == PIH_TASK_RANDOM_FLY ? FLY_FRAMES : -2); }

// q, qd (or NULL): double[n][ndof]; out: double[n][nframes][13]
int pihr_fk(int robot, int n, const double* q, const double* qd, double* out) {
  if (robot == PIH_ROBOT_PANDA) fk_t<Panda>(n, q, qd, out); else if (robot == PIH_ROBOT_UR5) fk_t<Ur5>(n, q, qd, out); else return -2;
  return 0;
}
// local (or NULL): double[n][3]; out: double[n][6][ndof]
int pihr_jacobian(int robot, int n, const double* q, int frame, const double* local, double* out) {
  int d[2];
  if (pihr_dims(robot, d) != 0 || frame < 0 || frame >= d[1]) return -2;
  if (robot == PIH_ROBOT_PANDA) jac_t<Panda>(n, q, frame, local, out); else jac_t<Ur5>(n, q, frame, local, out);
  return 0;
}
int pihr_mass_matrix(int robot, int n, const double* q, double* out) {
  if (robot == PIH_ROBOT_PANDA) mass_t<Panda>(n, q, out); else if (robot == PIH_ROBOT_UR5) mass_t<Ur5>(n, q, out); else return -2;
  return 0;
}
int pihr_inverse_dynamics(int robot, int n, const double* q, const double* qd, const double* qdd, double* tau) {
  if (robot == PIH_ROBOT_PANDA) invdyn_t<Panda>(n, q, qd, qdd, tau); else if (robot == PIH_ROBOT_UR5) invdyn_t<Ur5>(n, q, qd, qdd, tau); else return -2;
  return 0;
}
// states: double[n][words] env-major (words = PIH_STATE_WORDS or more for peg-in-hole, PIH_FLY_STATE_WORDS for random-fly); out: double[n][frames][13]
int pihr_link_states(int task, int n, int words, const double* states, double* out) {
  for (int e = 0; e < n; e++) {
    const double* rec = states + (size_t)e * words;
    auto S = [&](int w) { return (real)rec[w]; };
    if (task == PIH_TASK_PEG_IN_HOLE) {
      real rows[PEG_FRAMES * LSW]; peg_link_states(S, rows); store<PEG_FRAMES * LSW>(out, e, rows);
    } else if (task == PIH_TASK_RANDOM_FLY) {
      real rows[FLY_FRAMES * LSW]; fly_link_states(S, rows); store<FLY_FRAMES * LSW>(out, e, rows);
    } else return -2;
  }
  return 0;
}

}  // extern "C"
