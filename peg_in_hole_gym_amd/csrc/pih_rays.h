// pih_rays.h -- batched ray tests against the cameras' scenes (pih_ray_test, include/pih_robot.h): what p.rayTestBatch answers, for
// caller-given segments from -> to instead of a camera's pixel grid.  The scenes, the ray-versus-primitive functions and the normals are
// the cameras': view::ViewScene of pih_view.h (peg-in-hole: 38 primitives and the table plane) and fly::FlyScene of pih_fly_render.h
// (random-fly: six capsules, the object's spheres, the table plane).  What is new here is one function per task that traces an ARBITRARY
// ray (origin, unit direction, length, mask of the primitives to test) -- trace_view, trace_fly -- and the 8-word record of a ray.
//   hit      the nearest entry hit with ray parameter 0 < t <= length; the primitive functions report front faces only, so an origin
//            inside a sphere, a capsule or a box does not hit it; the tube's bore wall is hit from inside the bore; the table plane is
//            two-sided.  (ray_capsule is the union of a cylinder and two spheres: a ray from inside the cylinder part that runs along the
//            axis meets an end sphere from outside and reports it, here as in the cameras.)  peg-in-hole tests the arm last, in ARM_ORDER with VIEW_ARM_TIE, as view::shade_hit does: a ray through a pixel
//            centre names the link the image's seg byte names
//   record   fraction t / length in (0, 1] | seg as a float | hit position | outward unit normal (table: +z), env-local
//   miss     1 | PIH_SEG_NONE | `to` | 0
//   bad ray  a word that is not finite_small (NaN, Inf, beyond 1e15: found in the word's bits, the library is built with -ffast-math), or
//            a segment shorter than 1e-15: the miss record with the position words as given.  Nothing is indexed by ray data: `hit`
//            only ever takes the constants of the loops below
// A ray scene has no camera, and the scene structs' camera slots take what a ray scene has instead (the kernels' LDS stays the camera
// kernels'): eye, s, u, f hold the end-effector frame of PIH_RAY_FRAME_EE -- origin and the three axes -- and row i of bnd, the screen
// bound of primitive i, holds its bounding sphere (centre, radius + BALL_PAD).
// Every primitive is met through its bounding sphere (approach): the ray's origin is advanced to where the ray enters the sphere, the
// primitive function runs from there and the advance is added to its t.  A camera's eye is one point and its rays are short of nothing;
// a caller's ray starts anywhere, and the primitive functions lose digits with the SQUARE of the origin's distance over the primitive's
// size: a pipe capsule (r = 1 cm) 1.2 m away came back with t off by 3e-4 m in the fp32 host build; from the sphere's edge every hit of
// the test rays is within 1e-6 m (tests/ray_cases.py).
// The hits are the same set -- the primitive lies inside the sphere, the new origin outside the primitive -- and a ray that misses the
// sphere skips the primitive function (CULL; that part is an optimisation, measured in DESIGN.md 6.7).
// Rays are incoherent, so there is no tile culling: every lane walks the whole primitive list in the same order (`prims` is wave-uniform),
// and every scene read is a same-address LDS broadcast.
// This header keeps its own walks (trace_view, trace_fly), normals and bounding spheres beside the cameras' (view::nearest_hit /
// fly::nearest_hit, hit_normal / kind_normal, prim_ball): on those the random-fly kernel measured slower and 14 peg-in-hole rays left the
// recorded bits (DESIGN.md 6.5 has the figures).  A primitive added to a scene has to be added here too.
// Everything here is PIH_HD on `real`: the host build of tests/emul compiles the same per-ray code in fp64 and fp32.
#pragma once
#include "pih_view.h"

namespace pih {
namespace rays {

using fly::FlyPose;
using fly::FlyScene;
using view::ViewScene;

// the primitives PIH_RAY_IGNORE_ROBOT leaves on: peg-in-hole loses arm capsules, hand spheres and finger boxes, random-fly the six capsules
PIH_HD unsigned long long view_prims(int flags) {
  return (flags & PIH_RAY_IGNORE_ROBOT) ? view::all_prims() & ~((1ull << view::P_PIPE) - 1ull) : view::all_prims();
}
PIH_HD unsigned fly_prims(int object, int flags) {
  return (flags & PIH_RAY_IGNORE_ROBOT) ? fly::all_prims(object) & ~((1u << fly::RCAP) - 1u) : fly::all_prims(object);
}

// ---- the end-effector frame in the camera slots of a scene (ViewScene, FlyScene)
template <class S> PIH_HD void put_frame(S& sc, V3 p, const M3& R) {
  real m[9]; stm(m, R);
  st3(sc.eye, p); st3(sc.s, mk(m[0], m[3], m[6])); st3(sc.u, mk(m[1], m[4], m[7])); st3(sc.f, mk(m[2], m[5], m[8]));
}
template <class S> PIH_HD V3 frame_vector(const S& sc, V3 x) { return x.x * ld3(sc.s) + x.y * ld3(sc.u) + x.z * ld3(sc.f); }
template <class S> PIH_HD V3 frame_point(const S& sc, V3 x) { return ld3(sc.eye) + frame_vector(sc, x); }

// ---- bounding spheres in the bound rows of a scene
#define PIH_RAY_BALL_PAD ((real)1e-3)      // [m] on every radius: 1e4 x the rounding of the advance, so the advanced origin stays outside the primitive
template <class S> PIH_HD void put_ball(S& sc, int i, V3 c, real r) {
  sc.bnd[i][0] = c.x; sc.bnd[i][1] = c.y; sc.bnd[i][2] = c.z; sc.bnd[i][3] = r + PIH_RAY_BALL_PAD;
}
PIH_HD void put_capsule_ball(real (*bnd)[4], int i, V3 a, V3 b, real r) {
  const V3 c = (real)0.5 * (a + b);
  bnd[i][0] = c.x; bnd[i][1] = c.y; bnd[i][2] = c.z; bnd[i][3] = (real)0.5 * norm(b - a) + r + PIH_RAY_BALL_PAD;
}
// The ray o + t d, 0 < t <= len, against the sphere `ball` (centre, radius): -> can it reach the sphere at all?  If so o2 = o + s d is the
// origin advanced to the sphere (s = 0 for an origin inside it or past its nearest point).  CULL = false: always true
template <bool CULL> PIH_HD bool approach(V3 o, V3 d, real len, const real* ball, V3& o2, real& s) {
  const V3 c = ld3(ball); const real rb = ball[3];
  s = max_(dot(c - o, d) - rb, (real)0);
  o2 = o + s * d;
  if (!CULL) return true;
  const V3 oc = c - o2;
  const real p = dot(oc, d);                       // the sphere spans the ray parameters p - rb .. p + rb from o2
  return dot(oc, oc) - p * p <= rb * rb && p + rb > 0 && s <= len;
}

// two-sided plane z = PIH_TABLE_Z
PIH_HD real ray_table(V3 o, V3 d) {
  if (!(absr(d.z) > (real)1e-30)) return PIH_BIG;
  const real t = ((real)PIH_TABLE_Z - o.z) / d.z;
  return t > 0 ? t : PIH_BIG;
}

// peg-in-hole: nearest hit of the ray o + t d, 0 < t <= len, among the table and the primitives of `prims` (bit i: primitive i of
// pih_view.h) -> t, PIH_BIG for none; hit = primitive index, HIT_TABLE or HIT_NONE.  Order and tie rule of view::shade_hit
template <bool CULL> PIH_HD real trace_view(const ViewScene& sc, V3 o, V3 d, real len, unsigned long long prims, int& hit_out) {
  using namespace view;
  real best = PIH_BIG, s;
  int hit = HIT_NONE;
  V3 o2;
  {
    const real t = ray_table(o, d);
    if (t <= len) { best = t; hit = HIT_TABLE; }
  }
  unsigned segs = (unsigned)(prims >> P_PIPE) & ((1u << NSEG) - 1u);
  while (segs) {
    const int sg = __builtin_ctz(segs); segs &= segs - 1u;
    if (!approach<CULL>(o, d, len, sc.bnd[P_PIPE + sg], o2, s)) continue;
    const real t = s + ray_capsule(o2, d, ld3(sc.vtx[sg]), ld3(sc.vtx[sg + 1]), PIH_PIPE_RADIUS);
    if (t < best && t <= len) { best = t; hit = P_PIPE + sg; }
  }
  // Neighbouring pipe capsules share the end sphere at their common vertex.  From one origin both give the same hit there, bit for bit, and
  // the first keeps it (view::shade_hit); from two advanced origins the two hits differ in their last bits.  And where capsule k + 1's
  // cylinder begins it touches that sphere (in a straight stretch of pipe along the whole seam): the two hits are one to 1e-7 m over
  // 1e-4 m of pipe.  So the owner is read off the hit point, with the seam at the start plane of the later capsule, where exact
  // arithmetic has it: before the start plane of capsule k > 0 the hit lies on the shared sphere and belongs to capsule k - 1; on capsule
  // k's end sphere behind the start plane of capsule k + 1 it lies where that one's cylinder has begun, and belongs to it
  if (hit >= P_PIPE && hit < P_TUBE) {
    const int k = hit - P_PIPE;
    const V3 ph = o + best * d, a = ld3(sc.vtx[k]), b = ld3(sc.vtx[k + 1]);
    if (dot(ph - a, b - a) <= 0) hit -= k > 0 ? 1 : 0;
    else if (k + 1 < NSEG && dot(ph - b, b - a) >= 0 && dot(ph - b, ld3(sc.vtx[k + 2]) - b) > 0) hit++;
  }
  if ((prims & (1ull << P_TUBE)) && approach<CULL>(o, d, len, sc.bnd[P_TUBE], o2, s)) {
    const real t = s + ray_tube(o2, d);
    if (t < best && t <= len) { best = t; hit = P_TUBE; }
  }
  for (int f = 0; f < 2; f++)
    if ((prims & (1ull << (P_BOX + f))) && approach<CULL>(o, d, len, sc.bnd[P_BOX + f], o2, s)) {
      const real t = s + ray_box(o2, d, ldm(sc.fR[f]), ld3(sc.fc[f]), ld3(FBOX_H));
      if (t < best && t <= len) { best = t; hit = P_BOX + f; }
    }
  unsigned hand = (unsigned)(prims >> P_HAND) & ((1u << VHAND) - 1u);
  while (hand) {
    const int i = __builtin_ctz(hand); hand &= hand - 1u;
    if (!approach<CULL>(o, d, len, sc.bnd[P_HAND + i], o2, s)) continue;
    const real t = s + ray_sphere(o2 - ld3(sc.hs[i]), d, ASPH_R[HAND_SPH0 + i]);
    if (t < best && t <= len) { best = t; hit = P_HAND + i; }
  }
  unsigned ord = 0;
  for (int k = 0; k < VARM; k++) ord |= (((unsigned)prims >> ((ARM_ORDER_NIBBLES >> (4 * k)) & 7u)) & 1u) << k;
  while (ord) {
    const int L = (int)((ARM_ORDER_NIBBLES >> (4 * __builtin_ctz(ord))) & 7u); ord &= ord - 1u;
    if (!approach<CULL>(o, d, len, sc.bnd[L], o2, s)) continue;
    const real t = s + ray_capsule(o2, d, ld3(sc.org[L]), ld3(sc.org[L + 1]), ARM_R[L]);
    const real lim = hit < P_HAND ? best * ((real)1 - VIEW_ARM_TIE) : best;
    if (t < lim && t <= len) { best = t; hit = L; }
  }
  hit_out = hit;
  return best;
}
// outward unit normal at the point ph of what trace_view hit (not HIT_NONE), as view::shade_hit takes it
PIH_HD V3 normal_view(const ViewScene& sc, int hit, V3 ph) {
  using namespace view;
  if (hit < P_HAND) return capsule_normal(ph, ld3(sc.org[hit]), ld3(sc.org[hit + 1]));
  if (hit < P_BOX) return capsule_normal(ph, ld3(sc.hs[hit - P_HAND]), ld3(sc.hs[hit - P_HAND]));      // (radial: a sphere is a capsule of length 0)
  if (hit < P_PIPE) return box_normal(ph, ldm(sc.fR[hit - P_BOX]), ld3(sc.fc[hit - P_BOX]));
  if (hit < P_TUBE) return capsule_normal(ph, ld3(sc.vtx[hit - P_PIPE]), ld3(sc.vtx[hit - P_PIPE + 1]));
  return hit == P_TUBE ? tube_normal(ph) : mk(0, 0, 1);
}

// random-fly: the same over the table, the capsules and the object's spheres of `prims` (bit i: primitive i of pih_fly_render.h);
// kind = link 0 .. RCAP - 1, KIND_OBJECT (which = the sphere), KIND_TABLE or KIND_NONE.  Order of fly::shade_kind
template <bool CULL> PIH_HD real trace_fly(const FlyScene& sc, V3 o, V3 d, real len, unsigned prims, int& kind_out, int& which_out) {
  using namespace fly;
  real best = PIH_BIG, s;
  int kind = KIND_NONE, which = 0;
  V3 o2;
  {
    const real t = ray_table(o, d);
    if (t <= len) { best = t; kind = KIND_TABLE; }
  }
  unsigned caps = prims & ((1u << RCAP) - 1u);
  while (caps) {
    const int L = __builtin_ctz(caps); caps &= caps - 1u;
    if (!approach<CULL>(o, d, len, sc.bnd[L], o2, s)) continue;
    const real t = s + ray_capsule(o2, d, ld3(sc.cap[L][0]), ld3(sc.cap[L][1]), sc.capr[L]);
    if (t < best && t <= len) { best = t; kind = L; }
  }
  unsigned sphs = prims >> RCAP;
  while (sphs) {
    const int i = __builtin_ctz(sphs); sphs &= sphs - 1u;
    if (!approach<CULL>(o, d, len, sc.bnd[RCAP + i], o2, s)) continue;
    const real t = s + ray_sphere(o2 - ld3(sc.sph[i]), d, sc.sphr[i]);
    if (t < best && t <= len) { best = t; kind = KIND_OBJECT; which = i; }
  }
  kind_out = kind; which_out = which;
  return best;
}
PIH_HD V3 normal_fly(const FlyScene& sc, int kind, int which, V3 ph) {
  using namespace fly;
  if (kind < RCAP) return capsule_normal(ph, ld3(sc.cap[kind][0]), ld3(sc.cap[kind][1]));
  if (kind == KIND_OBJECT) return capsule_normal(ph, ld3(sc.sph[which]), ld3(sc.sph[which]));
  return mk(0, 0, 1);
}

// ---- the record of one ray
struct Record { real w[PIH_RAY_HIT_WORDS]; };
PIH_HD Record miss_record(V3 to) {
  Record r;
  r.w[0] = 1; r.w[1] = (real)PIH_SEG_NONE; r.w[2] = to.x; r.w[3] = to.y; r.w[4] = to.z; r.w[5] = r.w[6] = r.w[7] = 0;
  return r;
}
PIH_HD Record hit_record(real t, real len, unsigned seg, V3 ph, V3 n) {
  Record r;
  const real fr = t / len;
  r.w[0] = fr > 1 ? (real)1 : fr; r.w[1] = (real)seg; r.w[2] = ph.x; r.w[3] = ph.y; r.w[4] = ph.z; r.w[5] = n.x; r.w[6] = n.y; r.w[7] = n.z;
  return r;
}
// The segment of the ray words w[PIH_RAY_WORDS] (from, to) in the env-local frame: origin, unit direction, length.  -> false for a bad ray
// (header comment); `to` is then the words as given
template <class S> PIH_HD bool ray_segment(const S& sc, const float* w, int flags, V3& o, V3& d, real& len, V3& to) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < PIH_RAY_WORDS; i++) ok = ok && finite_small(w[i]);
  o = mk((real)w[0], (real)w[1], (real)w[2]); to = mk((real)w[3], (real)w[4], (real)w[5]);
  if (!ok) return false;
  V3 delta = to - o;
  const real len2 = dot(delta, delta);
  if (!(len2 > (real)1e-30)) return false;
  if (flags & PIH_RAY_FRAME_EE) { o = frame_point(sc, o); to = frame_point(sc, to); delta = frame_vector(sc, delta); }
  len = (real)sqrt(len2);
  d = ((real)1 / len) * delta;
  return true;
}
template <bool CULL> PIH_HD Record view_record(const ViewScene& sc, const float* w, int flags) {
  V3 o, d, to; real len;
  if (!ray_segment(sc, w, flags, o, d, len, to)) return miss_record(to);
  int hit;
  const real t = trace_view<CULL>(sc, o, d, len, view_prims(flags), hit);
  if (hit == view::HIT_NONE) return miss_record(to);
  const V3 ph = o + t * d;
  return hit_record(t, len, view::seg_of_hit(hit), ph, normal_view(sc, hit, ph));
}
template <bool CULL> PIH_HD Record fly_record(const FlyScene& sc, int object, const float* w, int flags) {
  V3 o, d, to; real len;
  if (!ray_segment(sc, w, flags, o, d, len, to)) return miss_record(to);
  int kind, which;
  const real t = trace_fly<CULL>(sc, o, d, len, fly_prims(object, flags), kind, which);
  if (kind == fly::KIND_NONE) return miss_record(to);
  const V3 ph = o + t * d;
  return hit_record(t, len, fly::seg_of_kind(kind), ph, normal_fly(sc, kind, which, ph));
}

// ---- scene set-up without a camera, in two phases with a barrier between them (and one behind).
// Phase 1: the camera headers' scene_setup_poses place the primitives on every thread but the one that builds the camera basis
// (peg-in-hole: 15; random-fly: RCAP), which never runs here -- the camera argument is not read; that thread leaves the end-effector
// frame in the camera's slots instead.  Phase 2: thread i < number of primitives leaves the bounding sphere of primitive i.
constexpr int VIEW_EE_THREAD = 15, FLY_EE_THREAD = fly::RCAP;
static_assert(FLY_EE_THREAD < 8 && 8 + fly::RSPH <= 15, "threads of fly::scene_setup_poses: capsules, camera, spheres from 8, colours on 15");
// peg-in-hole, after fk_all and a barrier (every thread of the workgroup calls both)
PIH_HD void view_setup_poses(const Shared& sh, ViewScene& sc, int tid) {
  if (tid == VIEW_EE_THREAD) {
    V3 pe; M3 Re; ee_pose(sh, pe, Re);
    put_frame(sc, pe, Re);
  } else {
    view::scene_setup_poses(sh, sc, fly::FlyCam{}, 0, tid);
  }
}
PIH_HD void view_setup_balls(ViewScene& sc, int tid) {
  using namespace view;
  if (tid < P_HAND) put_capsule_ball(sc.bnd, tid, ld3(sc.org[tid]), ld3(sc.org[tid + 1]), ARM_R[tid]);
  else if (tid < P_BOX) put_ball(sc, tid, ld3(sc.hs[tid - P_HAND]), ASPH_R[HAND_SPH0 + tid - P_HAND]);
  else if (tid < P_PIPE) put_ball(sc, tid, ld3(sc.fc[tid - P_BOX]), norm(ld3(FBOX_H)));
  else if (tid < P_TUBE) put_capsule_ball(sc.bnd, tid, ld3(sc.vtx[tid - P_PIPE]), ld3(sc.vtx[tid - P_PIPE + 1]), PIH_PIPE_RADIUS);
  else if (tid == P_TUBE) put_ball(sc, tid, ld3(HOLE_POS), (real)sqrt(PIH_HOLE_HALFLEN * PIH_HOLE_HALFLEN + PIH_HOLE_ROUT * PIH_HOLE_ROUT));
}
// random-fly (threads 0 .. 15 of the workgroup call the first, every thread the second)
PIH_HD void fly_setup_poses(FlyScene& sc, const FlyPose& ps, int object, int tid) {
  if (tid == FLY_EE_THREAD) {
    V3 pe; M3 Re; chain_ee<Ur5Chain>(ps.q, pe, Re);
    put_frame(sc, pe, Re);
  } else if (tid < 8 + fly::RSPH) {            // (thread 15 of fly::scene_setup_poses fills the colours: not needed)
    fly::scene_setup_poses(sc, ps, fly::FlyCam{}, object, 0, tid);
  }
}
PIH_HD void fly_setup_balls(FlyScene& sc, int tid) {
  using namespace fly;
  if (tid < RCAP) put_capsule_ball(sc.bnd, tid, ld3(sc.cap[tid][0]), ld3(sc.cap[tid][1]), sc.capr[tid]);
  else if (tid < FLY_NPRIM) put_ball(sc, tid, ld3(sc.sph[tid - RCAP]), sc.sphr[tid - RCAP]);
}

}  // namespace rays
}  // namespace pih
