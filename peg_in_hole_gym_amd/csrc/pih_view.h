// pih_view.h -- a free camera for the peg-in-hole task (pih_render_view, include/pih_render_view.h): what the wrist camera of pih_render.h draws -- the
// table plane, the 24 pipe capsules, the hole tube, the two finger-pad boxes, from the same primitives and constants -- plus the arm, seen
// from a caller-given viewpoint.  Camera, pixel grid and depth buffer are those of pih_render_cam (header comment of pih_fly_render.h).
//
// The arm is a BUILD-DEFINED stand-in: the Panda's visual meshes are not available to this build, so
//   link L = 0 .. 6   a capsule from its parent's origin (the arm base origin for link 0) to its own origin; radius = that of the model's
//                     collision sphere at the link's origin where it has one (PIH_ARM_SPH_*: links 3, 4, 5), VIEW_ARM_RADIUS otherwise.
//                     The origins of links 1 and 5 coincide with their parents': those capsules are spheres, and ray_capsule renders
//                     them as such (its cylinder part is skipped for A <= 1e-18, the two end spheres are one).  Neighbouring capsules
//                     share their end spheres, so two links can give the SAME hit; which of them owns the pixel must not hang on the last
//                     bit of two fp32 numbers: the links are tested in the order ARM_ORDER -- the two sphere links first, they are the
//                     joint housings -- and a later link takes the pixel only if its hit is nearer by more than ARM_TIE (relative).
//                     So link 1 owns the shoulder sphere it shares with links 0 and 2.  Link 5's sphere (r = 0.055) lies inside the end
//                     spheres of links 4 and 6 (r = 0.06) and is never seen from outside.
//   hand              the model's three hand spheres and the flange sphere (PIH_ARM_SPH entries 2 .. 5); it belongs to link 6
// Frames of the camera words: the env-local frame; PIH_RENDER_CAM_EE: the grasp-target frame (pybullet link 11, ee_pose) -- it turns with
// the hand; PIH_RENDER_CAM_EE_POS: eye and target offset by the grasp-target's position, axes env-local -- what the reference's wrist
// camera does.  Flat colours 0 .. 255: arm VIEW_COL_ARM, hand and fingers PIH_COL_FINGER, pipe and hole PIH_COL_PIPE, table, background.
// Segmentation byte (PIH_RENDER_OUT_RGBA8): link 0 .. 6 (hand: 6), fingers 7 and 8, PIH_VIEW_SEG_HOLE, PIH_VIEW_SEG_TABLE,
// PIH_VIEW_SEG_PIPE0 + capsule, PIH_SEG_NONE.
//
// Mapping (as pih_fly_render.h): one 256-thread workgroup per (env, strip of rows), forward kinematics (fk_all), scene and camera once per
// workgroup in LDS; each WAVE walks 16-row x 64-column tiles; lane i < VIEW_NPRIM tests the conservative screen bound of primitive i, in
// camera coordinates, against the tile (capsule: union of its end spheres' bounds; boxes: their eight corners against the tile's
// frustum; tube: bounding sphere; a primitive that cannot be bounded stays on for every tile); the 64-bit ballot is the tile's list.
// Everything here is PIH_HD on `real`: the host build of tests/emul compiles the same per-scene and per-pixel code in fp64 and fp32.
#pragma once
#include "pih_render.h"
#include "pih_fly_render.h"

namespace pih {
namespace view {

using fly::FlyCam;
using fly::FlyGrid;
using fly::TILE_COLS;
using fly::TILE_ROWS;

constexpr int VARM = 7, VHAND = 4, VBOX = 2;
// primitive i: arm capsule of link i | hand sphere | finger box | pipe capsule | hole tube
constexpr int P_HAND = VARM, P_BOX = P_HAND + VHAND, P_PIPE = P_BOX + VBOX, P_TUBE = P_PIPE + NSEG, VIEW_NPRIM = P_TUBE + 1;
static_assert(VIEW_NPRIM == 38 && VIEW_NPRIM <= 64, "the tile's primitive list is a 64-bit ballot");
constexpr int HIT_TABLE = VIEW_NPRIM, HIT_NONE = VIEW_NPRIM + 1;      // what a ray hit: a primitive, the table or nothing
constexpr int HAND_SPH0 = PIH_ARM_PIPE_SPH0;                          // first of the VHAND hand / flange spheres in PIH_ARM_SPH_*

#define VIEW_COL_ARM ((real)204)
#define VIEW_ARM_RADIUS 0.06

// radius of link L's capsule: the collision sphere at the link's origin, if the model has one
constexpr int M_SPH_LINK[PIH_ARM_NSPH] = PIH_ARM_SPH_LINK;
constexpr double M_SPH_C[PIH_ARM_NSPH][3] = PIH_ARM_SPH_C;
constexpr double M_SPH_R[PIH_ARM_NSPH] = PIH_ARM_SPH_R;
constexpr double arm_radius(int L) {
  for (int i = 0; i < PIH_ARM_NSPH; i++)
    if (M_SPH_LINK[i] == L && M_SPH_C[i][0] == 0 && M_SPH_C[i][1] == 0 && M_SPH_C[i][2] == 0) return M_SPH_R[i];
  return VIEW_ARM_RADIUS;
}
static_assert(arm_radius(2) == VIEW_ARM_RADIUS && arm_radius(5) == 0.055 && arm_radius(6) == VIEW_ARM_RADIUS, "links 3, 4, 5 take their collision spheres");
static_assert(M_SPH_LINK[HAND_SPH0] == 6 && M_SPH_LINK[HAND_SPH0 + VHAND - 1] == 6 && M_SPH_LINK[HAND_SPH0 + VHAND] != 6, "the hand's spheres ride on link 6");
constexpr double M_TFIX[PIH_NL][3] = PIH_LINK_TFIX;
constexpr bool at_parent(int L) { return M_TFIX[L][0] == 0 && M_TFIX[L][1] == 0 && M_TFIX[L][2] == 0; }
static_assert(at_parent(1) && at_parent(5) && !at_parent(0) && !at_parent(2) && !at_parent(3) && !at_parent(4) && !at_parent(6), "the sphere links");
constexpr unsigned ARM_ORDER_NIBBLES = 0x6432051u;          // ARM_ORDER, link k-th tested in nibble k: 1, 5, 0, 2, 3, 4, 6 -- links 1 and 5 (PIH_LINK_TFIX = 0: spheres) first
#define VIEW_ARM_TIE ((real)1e-5)
PIH_CONST real ARM_R[VARM] = {(real)arm_radius(0), (real)arm_radius(1), (real)arm_radius(2), (real)arm_radius(3), (real)arm_radius(4), (real)arm_radius(5), (real)arm_radius(6)};

struct ViewScene {
  real eye[3], s[3], u[3], f[3];            // camera position and basis (env-local frame)
  real tx, ty, znear, zfar;                 // tan(fov / 2) aspect, tan(fov / 2), clip planes
  real org[VARM + 1][3];                    // arm base origin, then the link origins: capsule L = org[L] .. org[L + 1]
  real hs[VHAND][3];                        // hand spheres
  real vtx[NSEG + 1][3];                    // pipe vertices
  real fR[2][9], fc[2][3];                  // finger boxes
  real bnd[VIEW_NPRIM][4];                  // screen bound (u0, u1, v0, v1) of every primitive; u0 > u1 = "always on"
  real bc[2][8][3];                         // finger-box corners in camera coordinates
};

PIH_HD V3 to_camera(const ViewScene& sc, V3 p) {      // (x right, y up, z = -depth: what sphere_bound takes)
  const V3 rel = p - ld3(sc.eye);
  return mk(dot(rel, ld3(sc.s)), dot(rel, ld3(sc.u)), -dot(rel, ld3(sc.f)));
}
// screen bound of a sphere / a capsule -> 1: bounded; 0: cannot bound (it reaches the eye plane), on for every tile; -1: wholly behind the
// eye plane, where no pixel's ray goes (every ray has d . f > 0): on no tile.  The wrist preset has the whole arm behind it.
PIH_HD int sphere_bound3(V3 rel, real r, real& u0, real& u1, real& v0, real& v1) {
  if (rel.z > r) return -1;                           // (z = -depth)
  return sphere_bound(rel, r, u0, u1, v0, v1) ? 1 : 0;
}
PIH_HD int capsule_bound(const ViewScene& sc, V3 a, V3 b, real r, real& u0, real& u1, real& v0, real& v1) {
  real a0, a1, b0, b1, c0, c1, d0, d1;
  const int ka = sphere_bound3(to_camera(sc, a), r, a0, a1, b0, b1), kb = sphere_bound3(to_camera(sc, b), r, c0, c1, d0, d1);
  if (ka < 0 && kb < 0) return -1;                    // (the capsule is the convex hull of its end spheres)
  if (ka <= 0 || kb <= 0) return 0;
  u0 = a0 < c0 ? a0 : c0; u1 = a1 > c1 ? a1 : c1; v0 = b0 < d0 ? b0 : d0; v1 = b1 > d1 ? b1 : d1;
  return 1;
}
// what scene_setup_bounds stores for the three answers
PIH_HD void put_bound(ViewScene& sc, int i, int k, real a0, real a1, real b0, real b1) {
  real u0 = 1, u1 = -1, v0 = 1, v1 = -1;              // "cannot bound": keep for every tile
  if (k > 0) { u0 = a0; u1 = a1; v0 = b0; v1 = b1; }
  if (k < 0) u0 = u1 = v0 = v1 = PIH_BIG;             // on no tile
  sc.bnd[i][0] = u0; sc.bnd[i][1] = u1; sc.bnd[i][2] = v0; sc.bnd[i][3] = v1;
}

// Scene set-up, part 1, after fk_all and a barrier (every thread of the workgroup calls it): threads 0 .. 7 place the arm's origins, 8 .. 11
// the hand's spheres, 12 and 13 the finger boxes, 15 builds the camera basis, 64 .. 64 + NSAMP - 1 place the pipe's vertices
PIH_HD void scene_setup_poses(const Shared& sh, ViewScene& sc, const FlyCam& cam, int flags, int tid) {
  if (tid <= VARM) st3(sc.org[tid], tid == 0 ? mk(0, 0, 0) : ld3(sh.LO[tid - 1]));
  if (tid >= 8 && tid < 8 + VHAND) {
    const int i = HAND_SPH0 + tid - 8, L = ASPH_LINK[i];
    st3(sc.hs[tid - 8], ld3(sh.LO[L]) + mul(ldm(sh.a.LR[L]), ld3(ASPH_C[i])));
  }
  if (tid >= 12 && tid < 14) {
    const int f = tid - 12, L = PIH_FINGER_LINK0 + f;
    const M3 R = ldm(sh.a.LR[L]);
    stm(sc.fR[f], R); st3(sc.fc[f], ld3(sh.LO[L]) + mul(R, ld3(FBOX_C[f])));
  }
  if (tid == 15) {
    V3 eye = mk((real)cam.w[fly::CAM_EYE], (real)cam.w[fly::CAM_EYE + 1], (real)cam.w[fly::CAM_EYE + 2]);
    V3 tgt = mk((real)cam.w[fly::CAM_TARGET], (real)cam.w[fly::CAM_TARGET + 1], (real)cam.w[fly::CAM_TARGET + 2]);
    V3 up = mk((real)cam.w[fly::CAM_UP], (real)cam.w[fly::CAM_UP + 1], (real)cam.w[fly::CAM_UP + 2]);
    if (flags & (PIH_RENDER_CAM_EE | PIH_RENDER_CAM_EE_POS)) {
      V3 pe; M3 Re; ee_pose(sh, pe, Re);
      if (flags & PIH_RENDER_CAM_EE) { eye = pe + mul(Re, eye); tgt = pe + mul(Re, tgt); up = mul(Re, up); }
      else { eye = pe + eye; tgt = pe + tgt; }
    }
    V3 f = tgt - eye; f = rsqrt_(dot(f, f)) * f;
    V3 s = cross(f, up); s = rsqrt_(dot(s, s)) * s;
    st3(sc.eye, eye); st3(sc.f, f); st3(sc.s, s); st3(sc.u, cross(s, f));
    real sn, cs; sincos_((real)cam.w[fly::CAM_FOV] * (PIH_PI / (real)360), &sn, &cs);
    sc.ty = sn / cs; sc.tx = sc.ty * (real)cam.w[fly::CAM_ASPECT];
    sc.znear = (real)cam.w[fly::CAM_NEAR]; sc.zfar = (real)cam.w[fly::CAM_FAR];
  }
  if (tid >= 64 && tid < 64 + NSAMP && SAMP_VERTEX[tid - 64]) place_pipe_vertex(sh, sc.vtx, tid - 64);
}
// part 2, after a barrier (threads 0 .. VIEW_NPRIM - 1): the screen bound of primitive `tid` in camera coordinates
PIH_HD void scene_setup_bounds(ViewScene& sc, int tid) {
  if (tid < VIEW_NPRIM) {
    real a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    int k = 0;
    if (tid < P_HAND) {
      k = capsule_bound(sc, ld3(sc.org[tid]), ld3(sc.org[tid + 1]), ARM_R[tid], a0, a1, b0, b1);
    } else if (tid < P_BOX) {
      k = sphere_bound3(to_camera(sc, ld3(sc.hs[tid - P_HAND])), ASPH_R[HAND_SPH0 + tid - P_HAND], a0, a1, b0, b1);
    } else if (tid < P_PIPE) {                        // finger boxes: corners, tested against each tile's frustum (prim_on_tile)
      const int f = tid - P_BOX;
      const M3 R = ldm(sc.fR[f]); const V3 c = ld3(sc.fc[f]), h = ld3(FBOX_H);
      for (int q = 0; q < 8; q++)
        st3(sc.bc[f][q], to_camera(sc, c + mul(R, mk((q & 1) ? h.x : -h.x, (q & 2) ? h.y : -h.y, (q & 4) ? h.z : -h.z))));
    } else if (tid < P_TUBE) {
      k = capsule_bound(sc, ld3(sc.vtx[tid - P_PIPE]), ld3(sc.vtx[tid - P_PIPE + 1]), PIH_PIPE_RADIUS, a0, a1, b0, b1);
    } else {                                          // hole tube: bounding sphere
      const real rad = (real)sqrt(PIH_HOLE_HALFLEN * PIH_HOLE_HALFLEN + PIH_HOLE_ROUT * PIH_HOLE_ROUT);
      k = sphere_bound3(to_camera(sc, ld3(HOLE_POS)), rad, a0, a1, b0, b1);
    }
    put_bound(sc, tid, k, a0, a1, b0, b1);
  }
}

// does primitive `i` (this lane's) touch the tile [tu0, tu1] x [tv0, tv1] of the camera plane?
PIH_HD bool prim_on_tile(const ViewScene& sc, int i, real tu0, real tu1, real tv0, real tv1) {
  if (i >= VIEW_NPRIM) return false;
  if (i >= P_BOX && i < P_PIPE) {
    // convex box vs the tile's frustum {tu0 d <= x <= tu1 d, tv0 d <= y <= tv1 d, d = depth}: invisible if all 8 corners lie outside one
    // of the four side planes (homogeneous form, valid for corners beside or behind the eye)
    bool o0 = true, o1 = true, o2 = true, o3 = true;
    for (int k = 0; k < 8; k++) {
      const real x = sc.bc[i - P_BOX][k][0], y = sc.bc[i - P_BOX][k][1], dpt = -sc.bc[i - P_BOX][k][2];
      o0 = o0 && (x - tu1 * dpt > 0); o1 = o1 && (x - tu0 * dpt < 0); o2 = o2 && (y - tv1 * dpt > 0); o3 = o3 && (y - tv0 * dpt < 0);
    }
    return !(o0 || o1 || o2 || o3);
  }
  const real u0 = sc.bnd[i][0], u1 = sc.bnd[i][1], v0 = sc.bnd[i][2], v1 = sc.bnd[i][3];
  if (u0 > u1) return true;
  return !(u1 < tu0 || u0 > tu1 || v1 < tv0 || v0 > tv1);
}
// the list with every primitive on (what a tile without culling sees)
PIH_HD unsigned long long all_prims() { return (1ull << VIEW_NPRIM) - 1ull; }

// segmentation value of what a ray hit
static_assert(PIH_VIEW_SEG_HOLE == 9 && PIH_VIEW_SEG_TABLE == 10 && PIH_VIEW_SEG_PIPE0 == 32, "seg values (include/pih_render_view.h)");
PIH_HD unsigned seg_of_hit(int hit) {
  if (hit < P_HAND) return (unsigned)hit;
  if (hit < P_BOX) return 6u;
  if (hit < P_PIPE) return 7u + (unsigned)(hit - P_BOX);
  if (hit < P_TUBE) return (unsigned)(PIH_VIEW_SEG_PIPE0 + hit - P_PIPE);
  return hit == P_TUBE ? (unsigned)PIH_VIEW_SEG_HOLE : (hit == HIT_TABLE ? (unsigned)PIH_VIEW_SEG_TABLE : (unsigned)PIH_SEG_NONE);
}

// ---- THE walk of this scene: the nearest hit of a pixel's ray (fly::CameraRay) among the table and the primitives of `prims` (bit i:
// primitive i; wave-uniform), in the order table, pipe capsules, hole tube, finger boxes, hand spheres, arm; a later primitive takes the
// ray only if it is nearer; a hit outside tnear .. tfar is dropped.  t = ray parameter (PIH_BIG: none), hit = primitive index, HIT_TABLE
// or HIT_NONE
struct ViewHit { real t; int hit; };
PIH_HD ViewHit nearest_hit(const ViewScene& sc, unsigned long long prims, const fly::CameraRay& ray) {
  const V3 eye = ray.o, d = ray.d;
  const real tnear = ray.tnear, tfar = ray.tfar;
  real best = PIH_BIG;
  int hit = HIT_NONE;
  if (absr(d.z) > (real)1e-30) {
    const real t = ((real)PIH_TABLE_Z - eye.z) / d.z;
    if (t >= tnear && t <= tfar) { best = t; hit = HIT_TABLE; }
  }
  unsigned segs = (unsigned)(prims >> P_PIPE) & ((1u << NSEG) - 1u);
  while (segs) {
    const int sg = __builtin_ctz(segs); segs &= segs - 1u;
    const real t = ray_capsule(eye, d, ld3(sc.vtx[sg]), ld3(sc.vtx[sg + 1]), PIH_PIPE_RADIUS);
    if (t < best && t >= tnear && t <= tfar) { best = t; hit = P_PIPE + sg; }
  }
  if (prims & (1ull << P_TUBE)) {
    const real t = ray_tube(eye, d);
    if (t < best && t >= tnear && t <= tfar) { best = t; hit = P_TUBE; }
  }
  for (int f = 0; f < 2; f++)
    if (prims & (1ull << (P_BOX + f))) {
      const real t = ray_box(eye, d, ldm(sc.fR[f]), ld3(sc.fc[f]), ld3(FBOX_H));
      if (t < best && t >= tnear && t <= tfar) { best = t; hit = P_BOX + f; }
    }
  unsigned hand = (unsigned)(prims >> P_HAND) & ((1u << VHAND) - 1u);
  while (hand) {
    const int i = __builtin_ctz(hand); hand &= hand - 1u;
    const real t = ray_sphere(eye - ld3(sc.hs[i]), d, ASPH_R[HAND_SPH0 + i]);
    if (t < best && t >= tnear && t <= tfar) { best = t; hit = P_HAND + i; }
  }
  // the arm comes last, its links in the order ARM_ORDER (bit k of `ord`: link ARM_ORDER[k] is on); while `hit` is a link, a later link
  // needs the margin.  (A scalar bit scan like the pipe's: a counted loop is unrolled into seven copies of ray_capsule, 181 VGPRs.)
  unsigned ord = 0;
  for (int k = 0; k < VARM; k++) ord |= (((unsigned)prims >> ((ARM_ORDER_NIBBLES >> (4 * k)) & 7u)) & 1u) << k;
  while (ord) {
    const int L = (int)((ARM_ORDER_NIBBLES >> (4 * __builtin_ctz(ord))) & 7u); ord &= ord - 1u;
    const real t = ray_capsule(eye, d, ld3(sc.org[L]), ld3(sc.org[L + 1]), ARM_R[L]);
    const real lim = hit < P_HAND ? best * ((real)1 - VIEW_ARM_TIE) : best;
    if (t < lim && t >= tnear && t <= tfar) { best = t; hit = L; }
  }
  ViewHit h; h.t = best; h.hit = hit;
  return h;
}
// the flat colour of what a ray hit
PIH_HD real hit_colour(int hit) {
  if (hit < P_HAND) return VIEW_COL_ARM;
  if (hit < P_PIPE) return PIH_COL_FINGER;
  if (hit <= P_TUBE) return PIH_COL_PIPE;
  return hit == HIT_TABLE ? PIH_COL_TABLE : PIH_COL_BG;
}
// outward unit normal at the point ph of `hit` (the helpers of pih_raycast.h and pih_render.h; radial on the hand's spheres; +z on the table)
PIH_HD V3 hit_normal(const ViewScene& sc, int hit, V3 ph) {
  V3 n = mk(0, 0, 1);
  if (hit < P_HAND) n = capsule_normal(ph, ld3(sc.org[hit]), ld3(sc.org[hit + 1]));
  else if (hit < P_BOX) n = capsule_normal(ph, ld3(sc.hs[hit - P_HAND]), ld3(sc.hs[hit - P_HAND]));      // (radial: a sphere is a capsule of length 0)
  else if (hit < P_PIPE) n = box_normal(ph, ldm(sc.fR[hit - P_BOX]), ld3(sc.fc[hit - P_BOX]));
  else if (hit < P_TUBE) n = capsule_normal(ph, ld3(sc.vtx[hit - P_PIPE]), ld3(sc.vtx[hit - P_PIPE + 1]));
  else if (hit == P_TUBE) n = tube_normal(ph);
  return n;
}
// the sphere that holds primitive i < VIEW_NPRIM, grown by `pad` (fly::Ball says why the margin is added there)
PIH_HD fly::Ball prim_ball(const ViewScene& sc, int i, real pad) {
  if (i < P_HAND) return fly::capsule_ball(ld3(sc.org[i]), ld3(sc.org[i + 1]), ARM_R[i], pad);
  if (i < P_BOX) return fly::sphere_ball(ld3(sc.hs[i - P_HAND]), ASPH_R[HAND_SPH0 + i - P_HAND], pad);
  if (i < P_PIPE) return fly::sphere_ball(ld3(sc.fc[i - P_BOX]), norm(ld3(FBOX_H)), pad);
  if (i < P_TUBE) return fly::capsule_ball(ld3(sc.vtx[i - P_PIPE]), ld3(sc.vtx[i - P_PIPE + 1]), PIH_PIPE_RADIUS, pad);
  return fly::sphere_ball(ld3(HOLE_POS), (real)sqrt(PIH_HOLE_HALFLEN * PIH_HOLE_HALFLEN + PIH_HOLE_ROUT * PIH_HOLE_ROUT), pad);
}

// one pixel: xc, yc = camera-plane coordinates of the pixel centre (already multiplied by tx / ty); prims = bit i set if primitive i
// may cover the pixel (wave-uniform); hit_out = what the ray hit (primitive index, HIT_TABLE, HIT_NONE)
PIH_HD real4 shade_hit(const ViewScene& sc, unsigned long long prims, real xc, real yc, int flags, int& hit_out) {
  const fly::CameraRay ray = fly::camera_ray(sc, xc, yc);
  const ViewHit h = nearest_hit(sc, prims, ray);
  real col = hit_colour(h.hit);
  if ((flags & PIH_RENDER_SHADED) && h.hit != HIT_NONE) {
    // Lambert term against the fixed light
    const V3 n = hit_normal(sc, h.hit, ray.o + h.t * ray.d);
    const real ndl = n.x * PIH_LIGHT_X + n.y * PIH_LIGHT_Y + n.z * PIH_LIGHT_Z;
    col = col * (PIH_LIGHT_AMBIENT + PIH_LIGHT_DIFFUSE * max_(ndl, (real)0));
  }
  real4 o; o.x = fly::depth_value(sc, ray, h.t, h.hit != HIT_NONE); o.y = col; o.z = col; o.w = col;
  hit_out = h.hit;
  return o;
}

// one pixel of each format (`bad`: the env's camera is degenerate, wave-uniform); byte rounding: fly::pack_byte
PIH_HD real4 pixel_float4(const ViewScene& sc, unsigned long long prims, real xc, real yc, int flags, bool bad) {
  int hit;
  return bad ? fly::background() : shade_hit(sc, prims, xc, yc, flags, hit);
}
PIH_HD unsigned pixel_rgba8(const ViewScene& sc, unsigned long long prims, real xc, real yc, int flags, bool bad) {
  int hit = HIT_NONE;
  const real4 c = bad ? fly::background() : shade_hit(sc, prims, xc, yc, flags, hit);
  return fly::pack_byte(c.y) | (fly::pack_byte(c.z) << 8) | (fly::pack_byte(c.w) << 16) | (seg_of_hit(hit) << 24);
}
PIH_HD real pixel_depth(const ViewScene& sc, unsigned long long prims, real xc, real yc, bool bad) {
  int hit;
  return bad ? (real)1 : shade_hit(sc, prims, xc, yc, 0, hit).x;
}

#ifndef PIH_PLATFORM_DEFINED      // ---------------------------------------------------------------- device only
// The scene set-up of a peg-in-hole free-camera kernel (every thread of the workgroup calls it; four barriers): the env's state record
// goes to LDS, fk_all runs once per workgroup, thread 15 reads the env's camera row and tests the camera (fly::camera_or_preset with the
// wrist preset) and leaves the code in cam_bad, `hook` adds a light (fly::NoLight: none), then the scene's two phases.
// -> the env gets the background
template <class Hook>
PIH_HD bool camera_setup(Shared& sh, ViewScene& sc, int& cam_bad, const Hook& hook, const float* __restrict__ state, FlyCam& cam,
                         const float* __restrict__ cam_dev, int env, int e, int& flags, int tid) {
  Wave w; w.l = tid; w.counter = 0;
  const float* rec = state + (size_t)env * PIH_STATE_WORDS;
  for (int i = tid; i < PIH_STATE_WORDS; i += RENDER_THREADS) sh.S[i] = rec[i];
  __syncthreads();
  fk_all(w, sh);
  __syncthreads();
  if (tid == 15) {
    fly::load_row(cam.w, cam_dev, e);
    cam_bad = fly::camera_or_preset(cam, FlyCam{PIH_VIEW_CAM_WRIST}, &flags);
  }
  if (tid == Hook::LIGHT_THREAD) hook.light_thread(all_prims());
  scene_setup_poses(sh, sc, cam, flags, tid);
  __syncthreads();
  scene_setup_bounds(sc, tid);
  hook.table(sc, tid);
  __syncthreads();
  return cam_bad != fly::CAM_OK || hook.bad();
}
#endif

}  // namespace view
}  // namespace pih
