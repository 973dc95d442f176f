// pih_dist.h -- batched closest-point queries against the cameras' scenes (pih_closest_points, include/pih_robot.h): what
// p.getClosestPoints answers for a POINT against the scene -- how far it is from the nearest selected primitive, which one that is, the
// closest point on its surface and the outward normal there.  The scenes are the ray tests': view::ViewScene (peg-in-hole: 38 primitives
// and the table plane) and fly::FlyScene (random-fly: six capsules, the object's spheres, the table plane), set up without a camera by
// rays::view_setup_poses / balls and rays::fly_setup_poses / balls of pih_rays.h: the end-effector frame in the camera's slots, one
// bounding sphere per primitive in the bound rows.  What is new here is the exact signed distance of every kind of primitive, with the
// normal, and one walk per task -- closest_view, closest_fly.
//   distance  negative inside a primitive.  sphere, capsule: |p - nearest axis point| - r.  oriented box: Euclidean outside, -(distance to
//             the nearest face) inside.  tube: the 2-D box distance of the rectangle [-halflen, halflen] x [rin, rout] in (axial, radial)
//             coordinates about the hole's axis (x); the bore is outside, the hole's centre is +rin away.  table: z - PIH_TABLE_Z, a half
//             space, negative below the plane
//   normal    the unit gradient of the distance: outward, inside and outside alike, so the closest point is p - d n and
//             p = closest point + d n.  Where the gradient does not exist (a sphere's centre, a capsule's axis, the tube's axis) any of the
//             closest points is reported with its normal: perpendicular to the axis, radial +z
//   walk      the ray tests' order: table, pipe capsules, tube, finger boxes, hand spheres, arm links in ARM_ORDER.  A primitive takes the
//             query only with d < best, and best starts at the query's reach: an exact tie keeps the first, nothing within reach is the miss
//   record    signed distance | seg as a float | closest point | outward unit normal, env-local
//   miss      reach | PIH_SEG_NONE | the query point, env-local | 0
//   bad query a word that is not finite_small, or reach <= 0: the miss record with words 0 and 2 .. 4 as given.  Nothing is indexed by
//             query data: `hit` only ever takes the constants of the loops below
// CULL: |p - c| - rb, with (c, rb) the primitive's bounding sphere, is a lower bound of its signed distance, so a primitive with
// |p - c| >= best + rb cannot take the query and is skipped, before any square root: squared lengths are compared once best + rb > 0 is
// known.  The spheres carry PIH_RAY_BALL_PAD = 1e-3 m on their radii, 1e4 x the rounding of the comparison, so the records are the same
// with and without (tests/test_dist.py compares the bits of the host builds).
// Every lane walks the whole primitive list in the same order (`prims` is wave-uniform): the scene reads are same-address LDS broadcasts.
// Everything here is PIH_HD on `real`: the host build of tests/emul compiles the same per-query code in fp64 and fp32.
#pragma once
#include "pih_rays.h"

namespace pih {
namespace dist {

using fly::FlyScene;
using view::ViewScene;

// ---- what `groups` (PIH_GROUP_*) selects: bit i = primitive i of the scene's header, and one bit more for the table
constexpr int VIEW_TABLE_BIT = view::HIT_TABLE, FLY_TABLE_BIT = fly::FLY_NPRIM;
static_assert(VIEW_TABLE_BIT < 64 && FLY_TABLE_BIT < 32, "the table's bit fits the scene's mask");
PIH_HD unsigned long long view_prims(int groups) {
  using namespace view;
  unsigned long long m = 0;
  if (groups & PIH_GROUP_ARM) m |= ((1ull << VARM) - 1ull) | (((1ull << VHAND) - 1ull) << P_HAND);
  if (groups & PIH_GROUP_FINGERS) m |= ((1ull << VBOX) - 1ull) << P_BOX;
  if (groups & PIH_GROUP_OBJECT) m |= ((1ull << NSEG) - 1ull) << P_PIPE;
  if (groups & PIH_GROUP_HOLE) m |= 1ull << P_TUBE;
  if (groups & PIH_GROUP_TABLE) m |= 1ull << VIEW_TABLE_BIT;
  return m;
}
PIH_HD unsigned fly_prims(int object, int groups) {
  using namespace fly;
  unsigned m = 0;
  if (groups & PIH_GROUP_ARM) m |= (1u << RCAP) - 1u;
  if (groups & PIH_GROUP_OBJECT) m |= all_prims(object) & ~((1u << RCAP) - 1u);
  if (groups & PIH_GROUP_TABLE) m |= 1u << FLY_TABLE_BIT;
  return m;
}

// ---- the running best of a walk: distance, normal, what it belongs to
struct Near { real d; V3 n; int hit; };
PIH_HD void take(Near& b, real d, V3 n, int hit) {
  if (d < b.d) { b.d = d; b.n = n; b.hit = hit; }
}
// can the primitive inside the sphere `ball` (centre, radius) be nearer than `best`?  CULL = false: always true
template <bool CULL> PIH_HD bool within(V3 p, const real* ball, real best) {
  if (!CULL) return true;
  const V3 v = p - ld3(ball);
  const real lim = best + ball[3];
  return lim > 0 && dot(v, v) < lim * lim;
}

// ---- signed distances; n = the outward unit normal
#define PIH_DIST_TINY2 ((real)1e-24)       // [m^2] below this squared length a direction is not taken from a difference
// a unit vector perpendicular to a (a = 0: +z)
PIH_HD V3 any_perpendicular(V3 a) {
  const real ax = absr(a.x), ay = absr(a.y), az = absr(a.z);
  const V3 c = (ax <= ay && ax <= az) ? mk(0, -a.z, a.y) : (ay <= az ? mk(a.z, 0, -a.x) : mk(-a.y, a.x, 0));
  const real l2 = dot(c, c);
  return l2 > PIH_DIST_TINY2 ? rsqrt_(l2) * c : mk(0, 0, 1);
}
// v = p - the nearest point of the axis (a sphere: its centre; axis = 0)
PIH_HD real sd_round(V3 v, V3 axis, real r, V3& n) {
  const real l2 = dot(v, v);
  if (l2 > PIH_DIST_TINY2) {
    const real l = (real)sqrt(l2);
    n = ((real)1 / l) * v;
    return l - r;
  }
  n = any_perpendicular(axis);
  return -r;
}
PIH_HD real sd_sphere(V3 p, V3 c, real r, V3& n) { return sd_round(p - c, mk(0, 0, 0), r, n); }
PIH_HD real sd_capsule(V3 p, V3 a, V3 b, real r, V3& n) {
  const V3 ba = b - a;
  real q = dot(p - a, ba) / max_(dot(ba, ba), (real)1e-20);
  q = q < 0 ? (real)0 : (q > 1 ? (real)1 : q);
  // v = p - the nearest axis point is perpendicular to the axis beside the cylinder and points away from it beyond an end.  Rounding leaves
  // v an axial part of some 1e-7 m, and for a point within 1e-4 m of the axis that turns the normal far enough to put the closest point
  // r (1 - cos) inside the surface: what exact arithmetic has as zero is taken out
  V3 v = p - (a + q * ba);
  const real s = dot(v, ba);
  if ((q > 0 && q < 1) || (q <= 0 && s > 0) || (q >= 1 && s < 0)) v = v - (s / max_(dot(ba, ba), (real)1e-20)) * ba;
  return sd_round(v, ba, r, n);
}
// the box |x_k| <= h_k, k < N, at the point x: outside the Euclidean distance, inside -(distance to the nearest face); n in box coordinates
template <int N> PIH_HD real sd_box_local(const real* x, const real* h, real* n) {
  real q[N], out2 = 0;
#pragma unroll
  for (int k = 0; k < N; k++) {
    q[k] = absr(x[k]) - h[k];
    const real o = max_(q[k], (real)0);
    out2 += o * o;
  }
  if (out2 > PIH_DIST_TINY2) {
    const real d = (real)sqrt(out2), inv = (real)1 / d;
#pragma unroll
    for (int k = 0; k < N; k++) n[k] = (x[k] < 0 ? -inv : inv) * max_(q[k], (real)0);
    return d;
  }
  int face = 0;
  real d = q[0];
#pragma unroll
  for (int k = 1; k < N; k++)
    if (q[k] > d) { d = q[k]; face = k; }
#pragma unroll
  for (int k = 0; k < N; k++) n[k] = k == face ? (x[k] < 0 ? (real)-1 : (real)1) : (real)0;
  return d;
}
PIH_HD real sd_box(V3 p, const M3& R, V3 c, V3 h, V3& n) {
  const V3 pl = tmul(R, p - c);
  const real x[3] = {pl.x, pl.y, pl.z}, hv[3] = {h.x, h.y, h.z};
  real nl[3];
  const real d = sd_box_local<3>(x, hv, nl);
  n = mul(R, mk(nl[0], nl[1], nl[2]));
  return d;
}
// the hole's tube about the x axis through HOLE_POS
PIH_HD real sd_tube(V3 p, V3& n) {
  const V3 oc = p - ld3(HOLE_POS);
  const real rho2 = oc.y * oc.y + oc.z * oc.z;
  real rho = 0;
  V3 e = mk(0, 0, 1);                                 // radial unit vector; on the axis any will do
  if (rho2 > PIH_DIST_TINY2) { rho = (real)sqrt(rho2); const real inv = (real)1 / rho; e = mk(0, oc.y * inv, oc.z * inv); }
  const real rmid = (real)(0.5 * (PIH_HOLE_RIN + PIH_HOLE_ROUT)), hwall = (real)(0.5 * (PIH_HOLE_ROUT - PIH_HOLE_RIN));
  const real x[2] = {oc.x, rho - rmid}, h[2] = {(real)PIH_HOLE_HALFLEN, hwall};
  real n2[2];
  const real d = sd_box_local<2>(x, h, n2);
  n = mk(n2[0], n2[1] * e.y, n2[1] * e.z);
  return d;
}

// peg-in-hole: the nearest of the primitives of `prims` (view_prims) to the point p, nearer than `reach` -> hit = primitive index,
// HIT_TABLE or HIT_NONE
template <bool CULL> PIH_HD Near closest_view(const ViewScene& sc, V3 p, real reach, unsigned long long prims) {
  using namespace view;
  Near b; b.d = reach; b.n = mk(0, 0, 0); b.hit = HIT_NONE;
  V3 n;
  if (prims & (1ull << VIEW_TABLE_BIT)) take(b, p.z - (real)PIH_TABLE_Z, mk(0, 0, 1), HIT_TABLE);
  unsigned segs = (unsigned)(prims >> P_PIPE) & ((1u << NSEG) - 1u);
  while (segs) {
    const int sg = __builtin_ctz(segs); segs &= segs - 1u;
    if (!within<CULL>(p, sc.bnd[P_PIPE + sg], b.d)) continue;
    const real d = sd_capsule(p, ld3(sc.vtx[sg]), ld3(sc.vtx[sg + 1]), PIH_PIPE_RADIUS, n);
    take(b, d, n, P_PIPE + sg);
  }
  if ((prims & (1ull << P_TUBE)) && within<CULL>(p, sc.bnd[P_TUBE], b.d)) {
    const real d = sd_tube(p, n);
    take(b, d, n, P_TUBE);
  }
  for (int f = 0; f < VBOX; f++)
    if ((prims & (1ull << (P_BOX + f))) && within<CULL>(p, sc.bnd[P_BOX + f], b.d)) {
      const real d = sd_box(p, ldm(sc.fR[f]), ld3(sc.fc[f]), ld3(FBOX_H), n);
      take(b, d, n, P_BOX + f);
    }
  unsigned hand = (unsigned)(prims >> P_HAND) & ((1u << VHAND) - 1u);
  while (hand) {
    const int i = __builtin_ctz(hand); hand &= hand - 1u;
    if (!within<CULL>(p, sc.bnd[P_HAND + i], b.d)) continue;
    const real d = sd_sphere(p, ld3(sc.hs[i]), ASPH_R[HAND_SPH0 + i], n);
    take(b, d, n, P_HAND + i);
  }
  unsigned ord = 0;
  for (int k = 0; k < VARM; k++) ord |= (((unsigned)prims >> ((ARM_ORDER_NIBBLES >> (4 * k)) & 7u)) & 1u) << k;
  while (ord) {
    const int L = (int)((ARM_ORDER_NIBBLES >> (4 * __builtin_ctz(ord))) & 7u); ord &= ord - 1u;
    if (!within<CULL>(p, sc.bnd[L], b.d)) continue;
    const real d = sd_capsule(p, ld3(sc.org[L]), ld3(sc.org[L + 1]), ARM_R[L], n);
    take(b, d, n, L);
  }
  return b;
}

// random-fly: the same over the table, the capsules and the object's spheres of `prims` (fly_prims); hit = link 0 .. RCAP - 1,
// KIND_OBJECT, KIND_TABLE or KIND_NONE
template <bool CULL> PIH_HD Near closest_fly(const FlyScene& sc, V3 p, real reach, unsigned prims) {
  using namespace fly;
  Near b; b.d = reach; b.n = mk(0, 0, 0); b.hit = KIND_NONE;
  V3 n;
  if (prims & (1u << FLY_TABLE_BIT)) take(b, p.z - (real)PIH_TABLE_Z, mk(0, 0, 1), KIND_TABLE);
  unsigned caps = prims & ((1u << RCAP) - 1u);
  while (caps) {
    const int L = __builtin_ctz(caps); caps &= caps - 1u;
    if (!within<CULL>(p, sc.bnd[L], b.d)) continue;
    const real d = sd_capsule(p, ld3(sc.cap[L][0]), ld3(sc.cap[L][1]), sc.capr[L], n);
    take(b, d, n, L);
  }
  unsigned sphs = (prims >> RCAP) & ((1u << RSPH) - 1u);
  while (sphs) {
    const int i = __builtin_ctz(sphs); sphs &= sphs - 1u;
    if (!within<CULL>(p, sc.bnd[RCAP + i], b.d)) continue;
    const real d = sd_sphere(p, ld3(sc.sph[i]), sc.sphr[i], n);
    take(b, d, n, KIND_OBJECT);
  }
  return b;
}

// ---- the record of one query
struct Record { real w[PIH_CLOSEST_WORDS]; };
PIH_HD Record miss_record(real reach, V3 p) {
  Record r;
  r.w[0] = reach; r.w[1] = (real)PIH_SEG_NONE; r.w[2] = p.x; r.w[3] = p.y; r.w[4] = p.z; r.w[5] = r.w[6] = r.w[7] = 0;
  return r;
}
PIH_HD Record hit_record(V3 p, const Near& b, unsigned seg, bool table) {
  Record r;
  V3 c = p - b.d * b.n;
  if (table) c.z = (real)PIH_TABLE_Z;                 // (exactly on the plane)
  r.w[0] = b.d; r.w[1] = (real)seg; r.w[2] = c.x; r.w[3] = c.y; r.w[4] = c.z; r.w[5] = b.n.x; r.w[6] = b.n.y; r.w[7] = b.n.z;
  return r;
}
// the point of the query words w[PIH_POINT_WORDS] (x, y, z, reach) in the env-local frame -> false for a bad query (header comment); p is
// then the words as given
template <class S> PIH_HD bool query_point(const S& sc, const float* w, int flags, V3& p, real& reach) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < PIH_POINT_WORDS; i++) ok = ok && finite_small(w[i]);
  p = mk((real)w[0], (real)w[1], (real)w[2]); reach = (real)w[3];
  if (!ok || !(w[3] > 0.f)) return false;
  if (flags & PIH_RAY_FRAME_EE) p = rays::frame_point(sc, p);
  return true;
}
template <bool CULL> PIH_HD Record view_record(const ViewScene& sc, const float* w, int flags, unsigned long long prims) {
  V3 p; real reach;
  if (!query_point(sc, w, flags, p, reach)) return miss_record(reach, p);
  const Near b = closest_view<CULL>(sc, p, reach, prims);
  if (b.hit == view::HIT_NONE) return miss_record(reach, p);
  return hit_record(p, b, view::seg_of_hit(b.hit), b.hit == view::HIT_TABLE);
}
template <bool CULL> PIH_HD Record fly_record(const FlyScene& sc, const float* w, int flags, unsigned prims) {
  V3 p; real reach;
  if (!query_point(sc, w, flags, p, reach)) return miss_record(reach, p);
  const Near b = closest_fly<CULL>(sc, p, reach, prims);
  if (b.hit == fly::KIND_NONE) return miss_record(reach, p);
  return hit_record(p, b, fly::seg_of_kind(b.hit), b.hit == fly::KIND_TABLE);
}

}  // namespace dist
}  // namespace pih
