// pih_clear.h -- robot clearance for many joint configurations (pih_robot_clearance, include/pih_robot.h): the body-to-body form of
// p.getClosestPoints -- resetJointState(q) + getClosestPoints(robot, body, distance, linkIndexA) per link -- for the task's robot at
// caller-given joint values q against the pipe / the flying object and the table at the env's CURRENT state.
//   probes     the round primitives the task's free camera draws for the arm and pih_closest_points measures as PIH_GROUP_ARM, placed
//              by the forward kinematics of pih_robot.h at q: Panda -- capsule L = origin of link L - 1 (the base for L = 0) to origin of
//              link L, radius view::ARM_R[L], L = 0 .. 6, then the four hand spheres ASPH_C / ASPH_R[HAND_SPH0 + i] on link 6 (seg 6);
//              UR5 -- the six capsules PIH_UR5_CAP_A / B / R.  A sphere is a capsule of zero length (so are the Panda's links 1 and 5)
//   obstacles  PIH_GROUP_TABLE: the half space z <= PIH_TABLE_Z; PIH_GROUP_OBJECT: peg-in-hole the 24 pipe capsules (sc.vtx,
//              PIH_PIPE_RADIUS), random-fly the object's spheres (sc.sph / sc.sphr), from the scenes rays::view_setup_* / fly_setup_* leave
//   distance   between the two SURFACES, negative for an overlap.  capsule - capsule: |x - y| - ra - rb with (x, y) a closest pair of the
//              two axis segments (closest_axes); capsule - sphere: y is the centre; capsule - table: z - r - PIH_TABLE_Z of the lower end
//   normal     the unit vector from the obstacle's closest point to the probe's (contactNormalOnB): (x - y) / |x - y|, +z for the table.
//              point on probe = x - ra n, point on obstacle = y + rb n, so point on probe = point on obstacle + distance x normal for
//              overlapping and separated pairs alike.  Where the pair is not unique (parallel axes, a horizontal capsule over the table)
//              one closest pair is reported; where the axes touch (|x - y|^2 <= PIH_DIST_TINY2) n is a perpendicular of both axes
//   rounding   x - y has, in exact arithmetic, no part along an axis whose parameter is interior, and beyond an end only a part that
//              points away from the segment.  What rounding leaves there turns n when |x - y| is small and takes the reported points
//              off their surfaces (pih_dist.h, sd_capsule): it is taken out before the length is measured
//   walk       table, then the object's primitives in index order; an obstacle replaces the running nearest only if it is strictly
//              nearer; the running nearest starts at the call's reach
//   record     PIH_CLEAR_WORDS = 12: distance | obstacle seg | point on probe | point on obstacle | normal | probe seg
//   miss       reach | PIH_SEG_NONE | the probe's first axis end point, twice | 0 | probe seg
//   bad q      a word that is not finite_small: every probe of the configuration gets reach | PIH_SEG_NONE | 0 ... 0 | probe seg, and
//              no forward kinematics runs on the words.  Nothing is indexed by anything derived from q: the probe index is the loop
//              counter, the link arrays are indexed by compile-time constants only
// CULL: the obstacle lies inside its bounding sphere (c, rb) (the bound rows of the scene), the probe inside its own (cp, rp), so
// |cp - c| - rp - rb is a lower bound of the distance: dist::within with best + rp skips the obstacle.  PIH_RAY_BALL_PAD on rb keeps the
// records the same with and without (tests/test_clear.py compares the obstacle the host builds name).
// Everything here is PIH_HD on `real`: the host build of tests/emul compiles the same per-configuration code in fp64 and fp32.
#pragma once
#include "pih_dist.h"
#include "pih_robot.h"

namespace pih {
namespace clear {

using fly::FlyScene;
using view::ViewScene;

constexpr int CW = PIH_CLEAR_WORDS;
static_assert(CW == 12, "distance, seg, two points, normal, probe seg: three float4");

// ---- the probes of a robot at q: axis end points a[p], b[p] (a sphere: a = b); radius and seg are tables of the probe index
template <int NP_> struct Probes { V3 a[NP_], b[NP_]; };

struct PandaArm : robot::Panda { static constexpr int ND = view::VARM; };      // the seven revolute links: the fingers move no probe
static_assert(robot::Panda::parent(view::VARM - 1) == view::VARM - 2, "links 0 .. 6 are a serial chain");
PIH_CONST real PANDA_PROBE_R[PIH_CLEAR_PROBES_PANDA] = {
    (real)view::arm_radius(0), (real)view::arm_radius(1), (real)view::arm_radius(2), (real)view::arm_radius(3), (real)view::arm_radius(4),
    (real)view::arm_radius(5), (real)view::arm_radius(6), (real)view::M_SPH_R[view::HAND_SPH0], (real)view::M_SPH_R[view::HAND_SPH0 + 1],
    (real)view::M_SPH_R[view::HAND_SPH0 + 2], (real)view::M_SPH_R[view::HAND_SPH0 + 3]};

struct PandaRobot {
  static constexpr int NP = PIH_CLEAR_PROBES_PANDA, ND = robot::Panda::ND;
  static_assert(NP == view::VARM + view::VHAND, "arm capsules, hand spheres");
  PIH_HD static real radius(int p) { return PANDA_PROBE_R[p]; }
  PIH_HD static unsigned seg(int p) { return p < view::VARM ? (unsigned)p : 6u; }
  PIH_HD static void place(const real* q, Probes<NP>& P) {
    robot::Kin<PandaArm> K; robot::kinematics<PandaArm>(q, K);
#pragma unroll
    for (int L = 0; L < view::VARM; L++) { P.a[L] = L == 0 ? mk(0, 0, 0) : K.o[L == 0 ? 0 : L - 1]; P.b[L] = K.o[L]; }
#pragma unroll
    for (int i = 0; i < view::VHAND; i++) P.a[view::VARM + i] = P.b[view::VARM + i] = K.o[6] + mul(K.R[6], ld3(ASPH_C[view::HAND_SPH0 + i]));
  }
};
struct Ur5Robot {
  static constexpr int NP = PIH_CLEAR_PROBES_UR5, ND = robot::Ur5::ND;
  static_assert(NP == fly::RCAP, "the six link capsules");
  PIH_HD static real radius(int p) { return fly::R_CAP_R[p]; }
  PIH_HD static unsigned seg(int p) { return (unsigned)p; }
  PIH_HD static void place(const real* q, Probes<NP>& P) {
    robot::Kin<robot::Ur5> K; robot::kinematics<robot::Ur5>(q, K);
#pragma unroll
    for (int L = 0; L < NP; L++) { P.a[L] = K.o[L] + mul(K.R[L], ld3(fly::R_CAP_A[L])); P.b[L] = K.o[L] + mul(K.R[L], ld3(fly::R_CAP_B[L])); }
  }
};
// probe p of P (p is a loop counter or comes from the work-item index: a chain of selects, no indexed register array)
template <int NP_> PIH_HD void pick(const Probes<NP_>& P, int p, V3& a, V3& b) {
  a = P.a[0]; b = P.b[0];
#pragma unroll
  for (int k = 1; k < NP_; k++) {
    const V3 ak = P.a[k], bk = P.b[k];                // (values, then selects: a select between addresses would keep P in memory)
    const bool on = p == k;
    a = mk(on ? ak.x : a.x, on ? ak.y : a.y, on ? ak.z : a.z);
    b = mk(on ? bk.x : b.x, on ? bk.y : b.y, on ? bk.z : b.z);
  }
}

// ---- a closest pair (x on a .. b, y on c .. d) of two segments, either of which may have zero length, and v = x - y with rounding's axial
// parts taken out (header comment).  s = the component of r = a - c along d1 perpendicular to d2 decides the first parameter: the quotient
// (B F - C E) / (A E - B^2) of the textbook form loses all its digits for nearly parallel axes, this one only those of the angle
struct Axes { V3 x, y, v, d1, d2; };
PIH_HD real clamp01(real t) { return t < 0 ? (real)0 : (t > 1 ? (real)1 : t); }
PIH_HD Axes closest_axes(V3 a, V3 b, V3 c, V3 d) {
  Axes o;
  o.d1 = b - a; o.d2 = d - c;
  const V3 r = a - c;
  const real A = dot(o.d1, o.d1), E = dot(o.d2, o.d2), iA = (real)1 / max_(A, (real)1e-20), iE = (real)1 / max_(E, (real)1e-20);
  const real B = dot(o.d1, o.d2), C = dot(o.d1, r), F = dot(o.d2, r);
  const V3 d1p = o.d1 - (B * iE) * o.d2;                      // d1 without its part along d2
  const real Ap = dot(d1p, d1p);
  real s = Ap > (real)1e-12 * A ? clamp01(-dot(d1p, r) / Ap) : (real)0;      // (parallel, or a sphere: any s is as good, the clamps below decide)
  real t = (B * s + F) * iE;
  if (t < 0) { t = 0; s = clamp01(-C * iA); }
  else if (t > 1) { t = 1; s = clamp01((B - C) * iA); }
  o.x = a + s * o.d1; o.y = c + t * o.d2;
  V3 v = o.x - o.y;
  const real c1 = dot(v, o.d1), c2 = dot(v, o.d2);
  const bool off1 = (s > 0 && s < 1) || (s <= 0 && c1 < 0) || (s >= 1 && c1 > 0);
  const bool off2 = (t > 0 && t < 1) || (t <= 0 && c2 > 0) || (t >= 1 && c2 < 0);
  const V3 cr = cross(o.d1, o.d2);
  const real cr2 = dot(cr, cr);
  if (off1 && off2 && cr2 > (real)1e-8 * A * E) {
    v = (dot(v, cr) / cr2) * cr;                      // both parts at once: what is left lies along d1 x d2 (one after the other, the second brings the first back)
  } else {                                            // (nearly parallel axes are one direction)
    if (off1) v = v - (c1 * iA) * o.d1;
    if (off2) v = v - (dot(v, o.d2) * iE) * o.d2;
  }
  o.v = v;
  return o;
}
// a unit vector perpendicular to both axes (either may be 0)
PIH_HD V3 perpendicular_of_both(V3 d1, V3 d2) {
  const V3 c = cross(d1, d2);
  const real c2 = dot(c, c), A = dot(d1, d1), E = dot(d2, d2);
  if (c2 > (real)1e-10 * A * E && c2 > PIH_DIST_TINY2 * PIH_DIST_TINY2) return rsqrt_(c2) * c;
  return dist::any_perpendicular(A >= E ? d1 : d2);
}

// ---- the running nearest of a probe's walk: distance, normal, the probe's axis point x of the pair, what it belongs to
struct Near { real d; V3 n, x; int hit; };
PIH_HD void take_round(Near& bst, V3 a, V3 b, real ra, V3 c, V3 d, real rb, int hit) {
  const Axes ax = closest_axes(a, b, c, d);
  const real l2 = dot(ax.v, ax.v);
  real dd; V3 n;
  if (l2 > PIH_DIST_TINY2) { const real l = (real)sqrt(l2); n = ((real)1 / l) * ax.v; dd = l - ra - rb; }
  else { n = perpendicular_of_both(ax.d1, ax.d2); dd = -ra - rb; }
  if (dd < bst.d) { bst.d = dd; bst.n = n; bst.x = ax.x; bst.hit = hit; }
}
PIH_HD void take_table(Near& bst, V3 a, V3 b, real ra, int hit) {
  const V3 e = a.z <= b.z ? a : b;
  const real dd = e.z - ra - (real)PIH_TABLE_Z;
  if (dd < bst.d) { bst.d = dd; bst.n = mk(0, 0, 1); bst.x = e; bst.hit = hit; }
}
// the probe's bounding sphere
struct Ball { V3 c; real r; };
PIH_HD Ball probe_ball(V3 a, V3 b, real ra) { Ball o; o.c = (real)0.5 * (a + b); o.r = (real)0.5 * norm(b - a) + ra; return o; }

// peg-in-hole: hit = view::P_PIPE + capsule, view::HIT_TABLE or view::HIT_NONE
template <bool CULL> PIH_HD Near nearest_view(const ViewScene& sc, V3 a, V3 b, real ra, real reach, int groups) {
  using namespace view;
  Near bst; bst.d = reach; bst.n = mk(0, 0, 0); bst.x = a; bst.hit = HIT_NONE;
  if (groups & PIH_GROUP_TABLE) take_table(bst, a, b, ra, HIT_TABLE);
  if (groups & PIH_GROUP_OBJECT) {
    const Ball pb = probe_ball(a, b, ra);
    for (int sg = 0; sg < NSEG; sg++) {
      if (!dist::within<CULL>(pb.c, sc.bnd[P_PIPE + sg], bst.d + pb.r)) continue;
      take_round(bst, a, b, ra, ld3(sc.vtx[sg]), ld3(sc.vtx[sg + 1]), PIH_PIPE_RADIUS, P_PIPE + sg);
    }
  }
  return bst;
}
// random-fly: hit = fly::KIND_OBJECT, KIND_TABLE or KIND_NONE
template <bool CULL> PIH_HD Near nearest_fly(const FlyScene& sc, int nsph, V3 a, V3 b, real ra, real reach, int groups) {
  using namespace fly;
  Near bst; bst.d = reach; bst.n = mk(0, 0, 0); bst.x = a; bst.hit = KIND_NONE;
  if (groups & PIH_GROUP_TABLE) take_table(bst, a, b, ra, KIND_TABLE);
  if (groups & PIH_GROUP_OBJECT) {
    const Ball pb = probe_ball(a, b, ra);
    for (int i = 0; i < nsph; i++) {
      if (!dist::within<CULL>(pb.c, sc.bnd[RCAP + i], bst.d + pb.r)) continue;
      const V3 c = ld3(sc.sph[i]);
      take_round(bst, a, b, ra, c, c, sc.sphr[i], KIND_OBJECT);
    }
  }
  return bst;
}

// ---- the record of one probe
struct Record { real w[CW]; };
PIH_HD Record blank_record(real reach, V3 p, unsigned probe_seg) {
  Record r;
  r.w[0] = reach; r.w[1] = (real)PIH_SEG_NONE; r.w[2] = r.w[5] = p.x; r.w[3] = r.w[6] = p.y; r.w[4] = r.w[7] = p.z;
  r.w[8] = r.w[9] = r.w[10] = 0; r.w[11] = (real)probe_seg;
  return r;
}
PIH_HD Record hit_record(const Near& bst, real ra, unsigned seg, bool table, unsigned probe_seg) {
  Record r;
  const V3 pp = bst.x - ra * bst.n;
  V3 po = pp - bst.d * bst.n;
  if (table) po.z = (real)PIH_TABLE_Z;                // (exactly on the plane)
  r.w[0] = bst.d; r.w[1] = (real)seg; r.w[2] = pp.x; r.w[3] = pp.y; r.w[4] = pp.z; r.w[5] = po.x; r.w[6] = po.y; r.w[7] = po.z;
  r.w[8] = bst.n.x; r.w[9] = bst.n.y; r.w[10] = bst.n.z; r.w[11] = (real)probe_seg;
  return r;
}

// the joint words of a configuration -> are they all finite_small?  q takes them either way
template <class Rb> PIH_HD bool load_q(const float* w, real* q) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < Rb::ND; i++) { ok = ok && finite_small(w[i]); q[i] = (real)w[i]; }
  return ok;
}
// the probes of a configuration; a bad one (ok = false) leaves them at 0 and runs no kinematics on its words
template <class Rb> PIH_HD void place_probes(const real* q, bool ok, Probes<Rb::NP>& P) {
  real qs[Rb::ND];
#pragma unroll
  for (int i = 0; i < Rb::ND; i++) qs[i] = ok ? q[i] : (real)0;
  Rb::place(qs, P);
}
// record of probe p (0 .. NP - 1) of the configuration whose probes are P
template <bool CULL> PIH_HD Record view_record(const ViewScene& sc, const Probes<PandaRobot::NP>& P, bool ok, int p, real reach, int groups) {
  const unsigned ps = PandaRobot::seg(p);
  if (!ok) return blank_record(reach, mk(0, 0, 0), ps);
  V3 a, b; pick(P, p, a, b);
  const real ra = PandaRobot::radius(p);
  const Near bst = nearest_view<CULL>(sc, a, b, ra, reach, groups);
  if (bst.hit == view::HIT_NONE) return blank_record(reach, a, ps);
  return hit_record(bst, ra, view::seg_of_hit(bst.hit), bst.hit == view::HIT_TABLE, ps);
}
template <bool CULL> PIH_HD Record fly_record(const FlyScene& sc, int nsph, const Probes<Ur5Robot::NP>& P, bool ok, int p, real reach, int groups) {
  const unsigned ps = Ur5Robot::seg(p);
  if (!ok) return blank_record(reach, mk(0, 0, 0), ps);
  V3 a, b; pick(P, p, a, b);
  const real ra = Ur5Robot::radius(p);
  const Near bst = nearest_fly<CULL>(sc, nsph, a, b, ra, reach, groups);
  if (bst.hit == fly::KIND_NONE) return blank_record(reach, a, ps);
  return hit_record(bst, ra, fly::seg_of_kind(bst.hit), bst.hit == fly::KIND_TABLE, ps);
}

}  // namespace clear
}  // namespace pih
