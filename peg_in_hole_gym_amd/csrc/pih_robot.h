// pih_robot.h -- batched robot-model queries (include/pih_robot.h): link states, Jacobians, mass matrix and inverse dynamics of the
// Panda (9 DOF: 7 revolute + the two finger prismatic joints on the hand's branch) and of the UR5 (6 DOF), and the link states of
// the envs' current state.
//
// What replaces what: getLinkState(s)(computeLinkVelocity=1), calculateJacobian, calculateMassMatrix, calculateInverseDynamics of
// pybullet, which a controller or reward written against the reference's MetaEnv calls per env on the host.
//
// Mapping: ONE PROBLEM PER LANE, plain scalar code (27 .. 130 output words per problem are far too little work for a wavefront).  The
// algorithms are written once over a robot descriptor `Rb` (tables of the step: L_RFIX / L_TFIX / L_AXIS / masses / COM / inertias of
// pih_model.h for links [0, ANL); UR5_* and fly::U_* for the UR5); every loop over links is fully unrolled, so the per-link arrays
// are registers and no table is indexed by anything but a compile-time constant -- never by anything derived from q.
//
// Conventions are the step's (pih_common.h): world-aligned axes, each link's own origin as reference point, classical accelerations,
// gravity PIH_GRAVITY_Z, Bullet's per-link damping m v (k + k |v|), I w (k + k |w|) and the joint damping of the model.
//   kinematics      one outward pass: R, origin, joint axis of every link
//   fk_states       + velocity of every frame origin and angular velocity, from the same pass
//   jacobian        columns a_j x (p - o_j) | a_j (revolute), a_j | 0 (prismatic) of the ancestors of the frame, from the same pass
//   rnea            world-frame recursive Newton-Euler (the oracle's `rnea` line by line): tau = M qdd + bias(q, qd)
//   mass_matrix     ndof RNEA passes with unit accelerations, no velocity, no gravity; entry (i, j), i <= j, comes from pass j and is
//                   written to both triangles
// Outputs go through `real* out` with unit stride: the caller points it at the problem's rows in global memory or at the lane's
// staging rows in LDS (pih_robot.hip).
#pragma once
#include "pih_fly.h"      // pih_common.h and the UR5's dynamic tables fly::U_*

namespace pih {
namespace robot {

constexpr int LSW = PIH_LINK_STATE_WORDS;
static_assert(LSW == 13, "pos 3, quat 4, linear velocity 3, angular velocity 3");

namespace model_check {
constexpr int PAR[NL] = PIH_LINK_PARENT;
}

struct Panda : PandaChain {
  static constexpr int ND = PIH_ARM_NDOF, NF = ND + 1, EE_PARENT = PIH_EE_PARENT;
  static constexpr int parent(int L) { return L == ND - 1 ? ND - 3 : L - 1; }      // the second finger hangs on link 6 like the first
  static constexpr bool prismatic(int L) { return L >= 7; }
  PIH_HD static real mass(int L) { return L_MASS[L]; }
  PIH_HD static const real* com(int L) { return L_COM[L]; }
  PIH_HD static const real* inertia(int L) { return L_INERTIA[L]; }
  PIH_HD static real damping(int L) { return L_DAMPING[L]; }
};
struct Ur5 : Ur5Chain {
  static constexpr int ND = PIH_UR5_NJ, NF = ND + 1, EE_PARENT = ND - 1;
  static constexpr int parent(int L) { return L - 1; }
  static constexpr bool prismatic(int) { return false; }
  PIH_HD static real mass(int L) { return fly::U_MASS[L]; }
  PIH_HD static const real* com(int L) { return fly::U_COM[L]; }
  PIH_HD static const real* inertia(int L) { return fly::U_INERTIA[L]; }
  PIH_HD static real damping(int L) { return fly::U_DAMPING[L]; }
};
namespace model_check {
constexpr bool panda_ok() {
  for (int L = 0; L < Panda::ND; L++)
    if (PAR[L] != Panda::parent(L) || model_ce::JT[L] != (Panda::prismatic(L) ? PIH_JT_PRISMATIC : PIH_JT_REVOLUTE)) return false;
  return true;
}
static_assert(Panda::ND == ANL && panda_ok(), "Panda::parent / prismatic restate PIH_LINK_PARENT / PIH_LINK_JTYPE of the arm links");
}

// bit L set: joint L moves link X (L is X or one of its ancestors)
template <class Rb> constexpr unsigned ancestors(int X) {
  unsigned m = 0;
  for (int L = X; L >= 0; L = Rb::parent(L)) m |= 1u << L;
  return m;
}

template <class Rb> struct Kin { M3 R[Rb::ND]; V3 o[Rb::ND], a[Rb::ND]; };

template <class Rb> PIH_HD void kinematics(const real* q, Kin<Rb>& K) {
#pragma unroll
  for (int L = 0; L < Rb::ND; L++) {
    const int p = Rb::parent(L);
    const M3 Rp = p < 0 ? ldm(Rb::base_r()) : K.R[p < 0 ? 0 : p];
    const V3 op = p < 0 ? ld3(Rb::base_t()) : K.o[p < 0 ? 0 : p];
    const M3 Rj = mul(Rp, ldm(Rb::rfix(L)));
    const V3 oj = op + mul(Rp, ld3(Rb::tfix(L)));
    const V3 ax = ld3(Rb::axis(L));
    K.a[L] = mul(Rj, ax);
    if (Rb::prismatic(L)) { K.R[L] = Rj; K.o[L] = oj + q[L] * K.a[L]; }
    else { K.R[L] = mul(Rj, axis_angle(ax, q[L])); K.o[L] = oj; }      // the full-range axis_angle: q is caller data
  }
}

PIH_HD void put_frame(real* o, V3 p, const M3& R, V3 v, V3 w) {
  const Q4 q = m_to_q(R);
  o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
  o[7] = v.x; o[8] = v.y; o[9] = v.z; o[10] = w.x; o[11] = w.y; o[12] = w.z;
}

// out[NF][LSW]: every link frame and the end-effector frame; positions + off
template <class Rb> PIH_HD void fk_states(const real* q, const real* qd, V3 off, real* out) {
  constexpr int ND = Rb::ND;
  Kin<Rb> K; kinematics<Rb>(q, K);
  V3 w[ND], v[ND];
#pragma unroll
  for (int L = 0; L < ND; L++) {
    const int p = Rb::parent(L), pp = p < 0 ? 0 : p;
    V3 wp = mk(0, 0, 0), vp = mk(0, 0, 0);
    if (p >= 0) { wp = w[pp]; vp = v[pp] + cross(wp, K.o[L] - K.o[pp]); }
    const V3 aq = qd[L] * K.a[L];
    if (Rb::prismatic(L)) { w[L] = wp; v[L] = vp + aq; } else { w[L] = wp + aq; v[L] = vp; }
    put_frame(out + L * LSW, K.o[L] + off, K.R[L], v[L], w[L]);
  }
  constexpr int E = Rb::EE_PARENT;
  const V3 re = mul(K.R[E], ld3(Rb::ee_t()));
  put_frame(out + ND * LSW, K.o[E] + re + off, mul(K.R[E], ldm(Rb::ee_r())), v[E] + cross(w[E], re), w[E]);
}

// out[6][ND], rows 0..2 linear, 3..5 angular, for the point `local` of frame `frame` (0 .. NF - 1: the caller has checked the range)
template <class Rb> PIH_HD void jacobian(const real* q, int frame, V3 local, real* out) {
  constexpr int ND = Rb::ND;
  Kin<Rb> K; kinematics<Rb>(q, K);
  const int link = frame < ND ? frame : Rb::EE_PARENT;
  M3 Rf = K.R[0]; V3 of = K.o[0]; unsigned mask = ancestors<Rb>(0);
#pragma unroll
  for (int X = 1; X < ND; X++)
    if (X == link) { Rf = K.R[X]; of = K.o[X]; mask = ancestors<Rb>(X); }
  if (frame >= ND) { of = of + mul(Rf, ld3(Rb::ee_t())); Rf = mul(Rf, ldm(Rb::ee_r())); }
  const V3 p = of + mul(Rf, local);
#pragma unroll
  for (int j = 0; j < ND; j++) {
    const bool on = ((mask >> j) & 1u) != 0;
    const V3 a = K.a[j];
    V3 lin = Rb::prismatic(j) ? a : cross(a, p - K.o[j]), ang = Rb::prismatic(j) ? mk(0, 0, 0) : a;
    if (!on) { lin = mk(0, 0, 0); ang = mk(0, 0, 0); }
    out[0 * ND + j] = lin.x; out[1 * ND + j] = lin.y; out[2 * ND + j] = lin.z;
    out[3 * ND + j] = ang.x; out[4 * ND + j] = ang.y; out[5 * ND + j] = ang.z;
  }
}

// what the dynamics need of a pose: origins, joint axes, COM offsets and inertias about the COM in world axes
template <class Rb> struct Dyn { V3 o[Rb::ND], a[Rb::ND], rc[Rb::ND]; S3 Iw[Rb::ND]; };

template <class Rb> PIH_HD void dyn_setup(const real* q, Dyn<Rb>& D) {
  Kin<Rb> K; kinematics<Rb>(q, K);
#pragma unroll
  for (int L = 0; L < Rb::ND; L++) {
    D.o[L] = K.o[L]; D.a[L] = K.a[L];
    D.rc[L] = mul(K.R[L], ld3(Rb::com(L)));
    D.Iw[L] = rot_sym(K.R[L], lds3(Rb::inertia(L)));
  }
}

// World-frame recursive Newton-Euler.  VEL = false: no velocity terms, no damping (the mass-matrix passes, with gz = 0).
template <class Rb, bool VEL> PIH_HD void rnea(const Dyn<Rb>& D, const real* qd, const real* qdd, real gz, real* tau) {
  constexpr int ND = Rb::ND;
  V3 w[ND], al[ND], vo[ND], ao[ND], F[ND], N[ND];
#pragma unroll
  for (int L = 0; L < ND; L++) {
    const int p = Rb::parent(L), pp = p < 0 ? 0 : p;
    V3 wp = mk(0, 0, 0), alp = mk(0, 0, 0), vat = mk(0, 0, 0), aat = mk(0, 0, 0);
    if (p >= 0) {
      const V3 r = D.o[L] - D.o[pp];
      wp = w[pp]; alp = al[pp];
      const V3 t = cross(wp, r);
      vat = vo[pp] + t;
      aat = cross(alp, r) + ao[pp] + cross(wp, t);
    }
    const real rate = VEL ? qd[L] : (real)0;
    const V3 aq = rate * D.a[L];
    if (Rb::prismatic(L)) {
      w[L] = wp; al[L] = alp;
      vo[L] = vat + aq;
      ao[L] = aat + (real)2 * cross(wp, aq) + qdd[L] * D.a[L];
    } else {
      w[L] = wp + aq;
      al[L] = alp + cross(wp, aq) + qdd[L] * D.a[L];
      vo[L] = vat; ao[L] = aat;
    }
    const V3 rc = D.rc[L];
    const V3 t = cross(w[L], rc);
    const V3 vc = vo[L] + t;
    const V3 ac = cross(al[L], rc) + ao[L] + cross(w[L], t);
    const real m = Rb::mass(L);
    V3 f = mk(m * ac.x, m * ac.y, m * (ac.z - gz));
    const V3 Iw_ = mul(D.Iw[L], w[L]);
    V3 n = cross(w[L], Iw_) + mul(D.Iw[L], al[L]);
    if (VEL) {                                               // Bullet link damping, as the step's bias force (pih_step.h, pih_fly.h)
      const real sv = PIH_LIN_DAMP + PIH_LIN_DAMP * norm(vc), sw = PIH_ANG_DAMP + PIH_ANG_DAMP * norm(w[L]);
      f = f + (m * sv) * vc; n = n + sw * Iw_;
    }
    F[L] = f; N[L] = n + cross(rc, f);
  }
#pragma unroll
  for (int L = ND - 1; L >= 0; L--) {
    const int p = Rb::parent(L), pp = p < 0 ? 0 : p;
    tau[L] = dot(D.a[L], Rb::prismatic(L) ? F[L] : N[L]) + (VEL ? Rb::damping(L) * qd[L] : (real)0);
    if (p >= 0) { const V3 r = D.o[L] - D.o[pp]; F[pp] = F[pp] + F[L]; N[pp] = N[pp] + N[L] + cross(r, F[L]); }
  }
}

template <class Rb> PIH_HD void inverse_dynamics(const real* q, const real* qd, const real* qdd, real* tau) {
  Dyn<Rb> D; dyn_setup<Rb>(q, D);
  real t[Rb::ND];
  rnea<Rb, true>(D, qd, qdd, (real)PIH_GRAVITY_Z, t);
#pragma unroll
  for (int i = 0; i < Rb::ND; i++) tau[i] = t[i];
}

// out[ND][ND]
template <class Rb> PIH_HD void mass_matrix(const real* q, real* out) {
  constexpr int ND = Rb::ND;
  Dyn<Rb> D; dyn_setup<Rb>(q, D);
#pragma unroll
  for (int j = 0; j < ND; j++) {
    real e[ND], col[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) e[i] = i == j ? (real)1 : (real)0;
    rnea<Rb, false>(D, e, e, (real)0, col);
#pragma unroll
    for (int i = 0; i <= j; i++) { out[i * ND + j] = col[i]; out[j * ND + i] = col[i]; }
  }
}

// ---- link states of an env's current state, world coordinates.  `S(w)` reads word w of the env's state record.
constexpr int PEG_FRAMES = Panda::NF + ONL, FLY_FRAMES = Ur5::NF + 1;

template <class Get> PIH_HD void peg_link_states(Get S, real* out) {
  real q[Panda::ND], qd[Panda::ND];
#pragma unroll
  for (int i = 0; i < Panda::ND; i++) { q[i] = S(PIH_S_QARM + i); qd[i] = S(PIH_S_QDARM + i); }
  const V3 off = mk(S(PIH_S_OFFSET), S(PIH_S_OFFSET + 1), S(PIH_S_OFFSET + 2));
  fk_states<Panda>(q, qd, off, out);
  // the pipe: floating root (link ANL: the state's base pose and twist), then the serial chain of its 23 revolute joints
  Q4 qq; qq.x = S(PIH_S_QUAT); qq.y = S(PIH_S_QUAT + 1); qq.z = S(PIH_S_QUAT + 2); qq.w = S(PIH_S_QUAT + 3);
  M3 R = q_to_m(qq);
  V3 o = mk(S(PIH_S_POS), S(PIH_S_POS + 1), S(PIH_S_POS + 2));
  V3 v = mk(S(PIH_S_VLIN), S(PIH_S_VLIN + 1), S(PIH_S_VLIN + 2)), w = mk(S(PIH_S_VANG), S(PIH_S_VANG + 1), S(PIH_S_VANG + 2));
  put_frame(out + Panda::NF * LSW, o + off, R, v, w);
  for (int k = 1; k < ONL; k++) {
    const int L = ANL + k;                                   // (a loop counter: the tables are indexed by nothing of the state)
    const V3 on = o + mul(R, ld3(L_TFIX[L]));
    const M3 Rj = mul(R, ldm(L_RFIX[L]));
    const V3 ax = ld3(L_AXIS[L]);
    v = v + cross(w, on - o);
    w = w + S(PIH_S_QDJ + k - 1) * mul(Rj, ax);
    R = mul(Rj, axis_angle(ax, S(PIH_S_QJ + k - 1)));
    o = on;
    put_frame(out + (Panda::NF + k) * LSW, o + off, R, v, w);
  }
}

template <class Get> PIH_HD void fly_link_states(Get S, real* out) {
  real q[Ur5::ND], qd[Ur5::ND];
#pragma unroll
  for (int i = 0; i < Ur5::ND; i++) { q[i] = S(PIH_F_Q + i); qd[i] = S(PIH_F_QD + i); }
  const V3 off = mk(S(PIH_F_OFFSET), S(PIH_F_OFFSET + 1), S(PIH_F_OFFSET + 2));
  fk_states<Ur5>(q, qd, off, out);
  real* o = out + Ur5::NF * LSW;                             // the object: the state's pose and twist as they are
#pragma unroll
  for (int k = 0; k < 3; k++) { o[k] = S(PIH_F_OPOS + k) + (k == 0 ? off.x : (k == 1 ? off.y : off.z)); o[7 + k] = S(PIH_F_OVLIN + k); o[10 + k] = S(PIH_F_OVANG + k); }
#pragma unroll
  for (int k = 0; k < 4; k++) o[3 + k] = S(PIH_F_OQUAT + k);
}

}  // namespace robot
}  // namespace pih
