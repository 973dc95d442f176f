// pih_fly_render.h -- a free camera for the 'random-fly' task (pih_render_cam, include/pih.h): the UR5's six collision capsules, the
// object's sphere cover and the table plane, ray-cast from a caller-given viewpoint.
//
// The task class is not in the reference snapshot, so there is no prescribed camera pose: the camera comes from the caller in the terms
// of p.computeViewMatrix (eye, target, up) and p.computeProjectionMatrixFOV (fov, aspect, near, far), the image in the layout of
// p.getCameraImage as PegInHole.render uses it (envs/peg_in_hole.py:276-304): (depth-buffer value, r, g, b) per pixel.
//   basis   f = normalize(target - eye), s = normalize(f x up), u = s x f                          (computeViewMatrix)
//   pixel   (i, j), row 0 on top: xc = (2 (j + 1/2) / W - 1) tan(fov / 2) aspect, yc = (1 - 2 (i + 1/2) / H) tan(fov / 2),
//           ray d = normalize(f + xc s + yc u); the eye-space depth of a hit at ray parameter t is z = t (d . f)
//   scene   (env-local frame) the plane z = PIH_TABLE_Z; link capsules o_L + R_L CAP_A[L] .. o_L + R_L CAP_B[L], radius CAP_R[L], with the
//           link frames of fly::step_env; the object's first NSPH spheres at opos + R(oquat) SPH_C
//   hit     the nearest one with near <= z <= far; a primitive's hit outside [near, far] is dropped and the ray goes on to the others
//   depth   far (z - near) / (z (far - near)), 1 where nothing was hit
//   rgb     0 .. 255: table 153, link L 255 PIH_UR5_RGB[L], object 255 PIH_FLY_OBJ_RGB[object], nothing 255; PIH_RENDER_SHADED multiplies
//           by ambient + diffuse max(0, n . l) of pih_raycast.h (n: +z on the table, radial on capsules and spheres)
// PIH_RENDER_CAM_EE: eye, target and up are given in the ee_link frame of the env's UR5 (chain_ee<Ur5Chain>) -- an eye-in-hand camera.
// Output formats: float4 (depth, r, g, b) as above; PIH_RENDER_OUT_RGBA8 = bytes (r, g, b, seg), seg = the hit's kind (link 0 .. 5,
// PIH_SEG_OBJECT, PIH_SEG_TABLE, PIH_SEG_NONE); PIH_RENDER_OUT_DEPTH = the depth value alone.  PIH_RENDER_CAM_DEVICE: one camera per env,
// read by the kernel, tested by the kernel (cam_degenerate): a degenerate one gives its env the background.  Kernel: pih_fly_image_kernel
// (pih_fly_image.hip), one instance per output format, for one host camera and for per-env cameras alike.
//
// Mapping (as pih_render.h): one 256-thread workgroup per (env, strip of rows), the scene once per workgroup in LDS; each WAVE walks
// 16-row x 64-column tiles; lane i < FLY_NPRIM tests the conservative screen bound of primitive i (camera coordinates; a capsule's bound
// is the union of its two end spheres' bounds; a sphere that reaches the eye plane keeps its primitive on for every tile) against the
// tile, the ballot is the tile's primitive list, one tile row is one coalesced 1 KB store.
// Everything here is PIH_HD on `real`: the host build of tests/emul compiles the same per-scene and per-pixel code in fp64 and fp32.
//
// This scene's primitive list -- its order, which array holds which primitive, its radii, its normals, its bounding spheres -- is spelled
// out once for the cameras, here: nearest_hit (the walk), kind_normal, prim_ball.  The shaded camera (shade_kind) and
// the lit camera (lit::lit_kind) are built on them; pih_view.h holds the same three for the peg-in-hole scene.  Two walks remain beside
// it: the shadow ray of pih_lit.h (an any-hit walk with a light-space cull) and the ray tests of pih_rays.h, which keep their own copy
// (DESIGN.md 6.5 says why).  The camera and ray kernels are held
// to their outputs' bits by tests/test_gpu_scene_bits.py and to their times by a measurement against the build before
// (profiles/scene_share_bench.txt); tools/isa_fingerprint.py holds the step kernels.
//
// This header is also the home of what ALL camera kernels share (the wrist camera of pih_render.h, this camera, pih_view.h, pih_lit.h), each
// piece once: CameraRay / camera_ray / depth_value (a pixel's ray and its depth-buffer value), Ball, FlyGrid (pixel grid), camera_or_preset, load_row, load_fly_pose, Pixels / NoLight (with lit::LitPixels / lit::LightHook)
// -- these also in the host build -- and, device only, render_strip (THE tile walk), render_image (the walk in an output format),
// camera_setup (this task's scene set-up; view::camera_setup is the peg-in-hole one) and dispatch_fmt (format -> kernel instance).
#pragma once
#include "pih_common.h"
#include "pih_raycast.h"
#ifndef PIH_PLATFORM_DEFINED
#include <type_traits>
#endif

namespace pih {
namespace fly {

constexpr int RCAP = PIH_UR5_NJ, RSPH = PIH_FLY_OBJ_MAXSPH;
constexpr int FLY_NPRIM = RCAP + RSPH;      // primitive i: capsule of link i (i < RCAP), object sphere i - RCAP
static_assert(FLY_NPRIM <= 32, "the tile's primitive list is a 32-bit mask");
// colour classes of a pixel = rows of FlyScene::rgb: link L, then
constexpr int KIND_OBJECT = RCAP, KIND_TABLE = RCAP + 1, KIND_NONE = RCAP + 2, NKIND = RCAP + 3;

PIH_CONST real R_UR5_RGB[RCAP][3] = PIH_UR5_RGB;
PIH_CONST real R_OBJ_RGB[PIH_FLY_NOBJ][3] = PIH_FLY_OBJ_RGB;
PIH_CONST real R_CAP_A[RCAP][3] = PIH_UR5_CAP_A;
PIH_CONST real R_CAP_B[RCAP][3] = PIH_UR5_CAP_B;
PIH_CONST real R_CAP_R[RCAP] = PIH_UR5_CAP_R;
PIH_CONST int R_NSPH[PIH_FLY_NOBJ] = PIH_FLY_OBJ_NSPH;
PIH_CONST real R_SPH_C[PIH_FLY_NOBJ][RSPH][3] = PIH_FLY_OBJ_SPH_C;
PIH_CONST real R_SPH_R[PIH_FLY_NOBJ][RSPH] = PIH_FLY_OBJ_SPH_R;

// the camera as the caller gives it (PIH_CAM_WORDS floats, passed to the kernel by value)
struct FlyCam { float w[PIH_CAM_WORDS]; };
enum : int { CAM_EYE = 0, CAM_TARGET = 3, CAM_UP = 6, CAM_FOV = 9, CAM_ASPECT = 10, CAM_NEAR = 11, CAM_FAR = 12 };
static_assert(CAM_FAR + 1 == PIH_CAM_WORDS, "camera words (include/pih.h)");
// the words of an env's state record the camera needs
struct FlyPose { real q[RCAP], opos[3], oquat[4]; };

struct FlyScene {
  real eye[3], s[3], u[3], f[3];            // camera position and basis (env-local frame)
  real tx, ty, znear, zfar;                 // tan(fov / 2) aspect, tan(fov / 2), clip planes
  real cap[RCAP][2][3], capr[RCAP];         // capsule end points and radii
  real sph[RSPH][3], sphr[RSPH];
  real bnd[FLY_NPRIM][4];                   // screen bound (u0, u1, v0, v1) of every primitive; u0 > u1 = "always on"
  real rgb[NKIND][3];
};

// Scene set-up, part 1 (threads 0 .. 15 of the workgroup do something): thread L < 6 walks the chain to link L and places its capsule,
// thread 6 walks it to ee_link and builds the camera basis, threads 8 .. 12 place the object's spheres, thread 15 fills the colours.
PIH_HD void scene_setup_poses(FlyScene& sc, const FlyPose& ps, const FlyCam& cam, int object, int flags, int tid) {
  if (tid <= RCAP) {
    // link frames as fly::step_env builds them: R_L = R_parent RFIX[L] rot(AXIS[L], q[L]), o_L = o_parent + R_parent TFIX[L]
    M3 R = ldm(IDENT3); V3 org = ld3(UR5_BASE_T);
    const int last = tid < RCAP ? tid : RCAP - 1;
#pragma unroll
    for (int L = 0; L < RCAP; L++) {                  // (unrolled: q[L] stays in registers)
      if (L > last) break;
      org = org + mul(R, ld3(UR5_TFIX[L]));
      R = mul(mul(R, ldm(UR5_RFIX[L])), axis_angle(ld3(UR5_AXIS[L]), ps.q[L]));
    }
    if (tid < RCAP) {
      st3(sc.cap[tid][0], org + mul(R, ld3(R_CAP_A[tid]))); st3(sc.cap[tid][1], org + mul(R, ld3(R_CAP_B[tid])));
      sc.capr[tid] = R_CAP_R[tid];
    } else {
      V3 eye = mk((real)cam.w[CAM_EYE], (real)cam.w[CAM_EYE + 1], (real)cam.w[CAM_EYE + 2]);
      V3 tgt = mk((real)cam.w[CAM_TARGET], (real)cam.w[CAM_TARGET + 1], (real)cam.w[CAM_TARGET + 2]);
      V3 up = mk((real)cam.w[CAM_UP], (real)cam.w[CAM_UP + 1], (real)cam.w[CAM_UP + 2]);
      if (flags & PIH_RENDER_CAM_EE) {
        const M3 Re = mul(R, ldm(UR5_EE_R)); const V3 pe = org + mul(R, ld3(UR5_EE_T));
        eye = pe + mul(Re, eye); tgt = pe + mul(Re, tgt); up = mul(Re, up);
      }
      V3 f = tgt - eye; f = rsqrt_(dot(f, f)) * f;
      V3 s = cross(f, up); s = rsqrt_(dot(s, s)) * s;
      st3(sc.eye, eye); st3(sc.f, f); st3(sc.s, s); st3(sc.u, cross(s, f));
      real sn, cs; sincos_((real)cam.w[CAM_FOV] * (PIH_PI / (real)360), &sn, &cs);
      sc.ty = sn / cs; sc.tx = sc.ty * (real)cam.w[CAM_ASPECT];
      sc.znear = (real)cam.w[CAM_NEAR]; sc.zfar = (real)cam.w[CAM_FAR];
    }
  } else if (tid >= 8 && tid < 8 + RSPH) {
    const int i = tid - 8;
    Q4 oq; oq.x = ps.oquat[0]; oq.y = ps.oquat[1]; oq.z = ps.oquat[2]; oq.w = ps.oquat[3];
    st3(sc.sph[i], ld3(ps.opos) + mul(q_to_m(oq), ld3(R_SPH_C[object][i])));
    sc.sphr[i] = R_SPH_R[object][i];
  } else if (tid == 15) {
    for (int c = 0; c < 3; c++) {
      for (int L = 0; L < RCAP; L++) sc.rgb[L][c] = (real)255 * R_UR5_RGB[L][c];
      sc.rgb[KIND_OBJECT][c] = (real)255 * R_OBJ_RGB[object][c];
      sc.rgb[KIND_TABLE][c] = PIH_COL_TABLE; sc.rgb[KIND_NONE][c] = PIH_COL_BG;
    }
  }
}
// part 2, after a barrier (threads 0 .. FLY_NPRIM - 1): the screen bound of primitive `tid` in camera coordinates
PIH_HD V3 to_camera(const FlyScene& sc, V3 p) {      // (x right, y up, z = -depth: what sphere_bound takes)
  const V3 rel = p - ld3(sc.eye);
  return mk(dot(rel, ld3(sc.s)), dot(rel, ld3(sc.u)), -dot(rel, ld3(sc.f)));
}
PIH_HD void scene_setup_bounds(FlyScene& sc, int object, int tid) {
  if (tid >= FLY_NPRIM) return;
  real u0 = 1, u1 = -1, v0 = 1, v1 = -1;              // "cannot bound": keep for every tile
  if (tid < RCAP) {
    real a0, a1, b0, b1, c0, c1, d0, d1;
    if (sphere_bound(to_camera(sc, ld3(sc.cap[tid][0])), sc.capr[tid], a0, a1, b0, b1) && sphere_bound(to_camera(sc, ld3(sc.cap[tid][1])), sc.capr[tid], c0, c1, d0, d1)) {
      u0 = a0 < c0 ? a0 : c0; u1 = a1 > c1 ? a1 : c1; v0 = b0 < d0 ? b0 : d0; v1 = b1 > d1 ? b1 : d1;
    }
  } else if (tid - RCAP < R_NSPH[object]) {
    real a0, a1, b0, b1;
    if (sphere_bound(to_camera(sc, ld3(sc.sph[tid - RCAP])), sc.sphr[tid - RCAP], a0, a1, b0, b1)) { u0 = a0; u1 = a1; v0 = b0; v1 = b1; }
  } else {
    u0 = u1 = v0 = v1 = PIH_BIG;                      // padding sphere of the object table: on no tile
  }
  sc.bnd[tid][0] = u0; sc.bnd[tid][1] = u1; sc.bnd[tid][2] = v0; sc.bnd[tid][3] = v1;
}

// does primitive `i` (this lane's) touch the tile [tu0, tu1] x [tv0, tv1] of the camera plane?
PIH_HD bool prim_on_tile(const FlyScene& sc, int i, real tu0, real tu1, real tv0, real tv1) {
  if (i >= FLY_NPRIM) return false;
  const real u0 = sc.bnd[i][0], u1 = sc.bnd[i][1], v0 = sc.bnd[i][2], v1 = sc.bnd[i][3];
  if (u0 > u1) return true;
  return !(u1 < tu0 || u0 > tu1 || v1 < tv0 || v0 > tv1);
}
// the mask with every primitive of the object on (what a tile without culling sees)
PIH_HD unsigned all_prims(int object) { return (1u << (RCAP + R_NSPH[object])) - 1u; }

// ---- what the per-pixel code of both scenes shares (this scene's and view::ViewScene's; shaded and lit cameras)
// the ray of a pixel, eye + t d, and the ray parameters of the near and far planes
struct CameraRay { V3 o, d; real inv, tnear, tfar; };      // inv = d . f
// the ray through the point (xc, yc) of the camera plane (already multiplied by tx / ty)
template <class S /* FlyScene, view::ViewScene */> PIH_HD CameraRay camera_ray(const S& sc, real xc, real yc) {
  CameraRay r;
  r.o = ld3(sc.eye);
  r.inv = rsqrt_((real)1 + xc * xc + yc * yc);
  r.d = r.inv * (ld3(sc.f) + xc * ld3(sc.s) + yc * ld3(sc.u));
  r.tnear = sc.znear / r.inv; r.tfar = sc.zfar / r.inv;      // ray parameters of the clip planes
  return r;
}
// the depth-buffer value of a hit at ray parameter t (hit = false: nothing was hit)
template <class S> PIH_HD real depth_value(const S& sc, const CameraRay& ray, real t, bool hit) {
  real depth = 1;
  if (hit) {
    const real z = t * ray.inv;
    depth = sc.zfar * (z - sc.znear) / (z * (sc.zfar - sc.znear));
  }
  return depth;
}
// the sphere that holds a primitive (centre, radius), grown by the caller's margin `pad` (LIT_CULL_SLACK for the light-space cull of
// pih_lit.h).  The margin is the last term of the one sum 0.5 |b - a| + r + pad: under -ffast-math a margin added to the finished radius
// is another sum, which matters wherever a radius enters a hit's bits
struct Ball { V3 c; real r; };
PIH_HD Ball capsule_ball(V3 a, V3 b, real r, real pad) { Ball s; s.c = (real)0.5 * (a + b); s.r = (real)0.5 * norm(b - a) + r + pad; return s; }
PIH_HD Ball sphere_ball(V3 c, real r, real pad) { Ball s; s.c = c; s.r = r + pad; return s; }

// ---- THE walk of this scene: the nearest hit of a pixel's ray among the table and the primitives of `prims` (bit i: primitive i;
// wave-uniform), in the order table, capsules, object spheres; a later primitive takes the ray only if it is nearer; a hit outside
// tnear .. tfar is dropped.  t = ray parameter (PIH_BIG: none), kind = link 0 .. RCAP - 1, KIND_OBJECT (sphere `which`), KIND_TABLE or KIND_NONE
struct FlyHit { real t; int kind, which; };
PIH_HD FlyHit nearest_hit(const FlyScene& sc, unsigned prims, const CameraRay& ray) {
  const V3 eye = ray.o, d = ray.d;
  const real tnear = ray.tnear, tfar = ray.tfar;
  real best = PIH_BIG;
  int kind = KIND_NONE, which = 0;
  if (absr(d.z) > (real)1e-30) {
    const real t = ((real)PIH_TABLE_Z - eye.z) / d.z;
    if (t >= tnear && t <= tfar) { best = t; kind = KIND_TABLE; }
  }
  unsigned caps = prims & ((1u << RCAP) - 1u);
  while (caps) {
    const int L = __builtin_ctz(caps); caps &= caps - 1u;
    const real t = ray_capsule(eye, d, ld3(sc.cap[L][0]), ld3(sc.cap[L][1]), sc.capr[L]);
    if (t < best && t >= tnear && t <= tfar) { best = t; kind = L; }
  }
  unsigned sphs = prims >> RCAP;
  while (sphs) {
    const int i = __builtin_ctz(sphs); sphs &= sphs - 1u;
    const real t = ray_sphere(eye - ld3(sc.sph[i]), d, sc.sphr[i]);
    if (t < best && t >= tnear && t <= tfar) { best = t; kind = KIND_OBJECT; which = i; }
  }
  FlyHit h; h.t = best; h.kind = kind; h.which = which;
  return h;
}
// outward unit normal at the point ph of a hit: radial on capsules and spheres, +z on the table
PIH_HD V3 kind_normal(const FlyScene& sc, const FlyHit& h, V3 ph) {
  V3 n = mk(0, 0, 1);
  if (h.kind < RCAP) n = capsule_normal(ph, ld3(sc.cap[h.kind][0]), ld3(sc.cap[h.kind][1]));
  else if (h.kind == KIND_OBJECT) n = capsule_normal(ph, ld3(sc.sph[h.which]), ld3(sc.sph[h.which]));      // (radial: a sphere is a capsule of length 0)
  return n;
}
// the sphere that holds primitive i < FLY_NPRIM
PIH_HD Ball prim_ball(const FlyScene& sc, int i, real pad) {
  if (i < RCAP) return capsule_ball(ld3(sc.cap[i][0]), ld3(sc.cap[i][1]), sc.capr[i], pad);
  return sphere_ball(ld3(sc.sph[i - RCAP]), sc.sphr[i - RCAP], pad);
}

// one pixel: xc, yc = camera-plane coordinates of the pixel centre (already multiplied by tx / ty); prims = bit i set if primitive i
// may cover the pixel (wave-uniform); kind_out = what the ray hit
PIH_HD real4 shade_kind(const FlyScene& sc, unsigned prims, real xc, real yc, int flags, int& kind_out) {
  const CameraRay ray = camera_ray(sc, xc, yc);
  const FlyHit h = nearest_hit(sc, prims, ray);
  real lit = 1;
  if ((flags & PIH_RENDER_SHADED) && h.kind != KIND_NONE) {
    // Lambert term against the fixed light
    const V3 n = kind_normal(sc, h, ray.o + h.t * ray.d);
    const real ndl = n.x * PIH_LIGHT_X + n.y * PIH_LIGHT_Y + n.z * PIH_LIGHT_Z;
    lit = PIH_LIGHT_AMBIENT + PIH_LIGHT_DIFFUSE * max_(ndl, (real)0);
  }
  real4 o; o.x = depth_value(sc, ray, h.t, h.kind != KIND_NONE); o.y = sc.rgb[h.kind][0] * lit; o.z = sc.rgb[h.kind][1] * lit; o.w = sc.rgb[h.kind][2] * lit;
  kind_out = h.kind;
  return o;
}
PIH_HD real4 shade(const FlyScene& sc, unsigned prims, real xc, real yc, int flags) {
  int kind;
  return shade_kind(sc, prims, xc, yc, flags, kind);
}

// The packed formats of pih_render_cam.  PIH_RENDER_OUT_RGBA8: one 32-bit word per pixel, bytes (r, g, b, seg) in memory order.
// A colour value v (fp32, 0 .. 255) becomes the byte min(255, (int)(v + 0.5)): rounded half up, so 178.5 -> 179; v is never negative.
PIH_HD unsigned pack_byte(real v) {
  const int b = (int)(v + (real)0.5);
  return b > 255 ? 255u : (unsigned)b;
}
// segmentation value of a pixel's kind: the link index, PIH_SEG_OBJECT, PIH_SEG_TABLE, PIH_SEG_NONE
static_assert(PIH_SEG_OBJECT == RCAP && PIH_SEG_OBJECT == KIND_OBJECT && PIH_SEG_TABLE == KIND_TABLE, "seg values of links, object and table are the pixel kinds");
PIH_HD unsigned seg_of_kind(int kind) { return kind < KIND_NONE ? (unsigned)kind : (unsigned)PIH_SEG_NONE; }
PIH_HD unsigned pack_rgba8(const real4& c, int kind) {
  return pack_byte(c.y) | (pack_byte(c.z) << 8) | (pack_byte(c.w) << 16) | (seg_of_kind(kind) << 24);
}
// what a pixel of an env with a degenerate camera holds: depth 1, rgb 255, PIH_SEG_NONE
PIH_HD real4 background() { real4 o; o.x = 1; o.y = o.z = o.w = PIH_COL_BG; return o; }
// one pixel of each format (`bad`: the env's camera is degenerate, wave-uniform)
PIH_HD real4 pixel_float4(const FlyScene& sc, unsigned prims, real xc, real yc, int flags, bool bad) {
  return bad ? background() : shade(sc, prims, xc, yc, flags);
}
PIH_HD unsigned pixel_rgba8(const FlyScene& sc, unsigned prims, real xc, real yc, int flags, bool bad) {
  int kind = KIND_NONE;
  const real4 c = bad ? background() : shade_kind(sc, prims, xc, yc, flags, kind);
  return pack_rgba8(c, kind);
}
PIH_HD real pixel_depth(const FlyScene& sc, unsigned prims, real xc, real yc, bool bad) {
  return bad ? (real)1 : shade(sc, prims, xc, yc, 0).x;
}

// Is the camera degenerate?  -> 0 or the code of the first field that is.  The host validates a camera it can read with this
// (pih_render_cam maps the code to its message); a camera in device memory (PIH_RENDER_CAM_DEVICE) is tested by the kernel, once per
// workgroup, and a degenerate one gives its env the background image.  The tests are frame-independent, so they hold for
// PIH_RENDER_CAM_EE as well.  !(a > b) also catches NaN where the compiler honours NaN; the library is built with -ffast-math, which does
// not, so a non-finite word is found by its bit pattern first -- with finite words no expression below can produce a NaN.
enum : int { CAM_OK = 0, CAM_BAD_VIEW = 1, CAM_BAD_UP = 2, CAM_BAD_FOV = 3, CAM_BAD_ASPECT = 4, CAM_BAD_NEAR = 5, CAM_BAD_FAR = 6 };
PIH_HHD bool cam_word_finite(float x) {
  unsigned u; __builtin_memcpy(&u, &x, sizeof u);
  return (u & 0x7f800000u) != 0x7f800000u;
}
PIH_HHD int cam_degenerate(const float* c) {
  bool fin[PIH_CAM_WORDS];
  for (int i = 0; i < PIH_CAM_WORDS; i++) fin[i] = cam_word_finite(c[i]);
  const double f[3] = {(double)c[3] - c[0], (double)c[4] - c[1], (double)c[5] - c[2]}, up[3] = {c[6], c[7], c[8]};
  const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]), ul = sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
  const double cx = f[1] * up[2] - f[2] * up[1], cy = f[2] * up[0] - f[0] * up[2], cz = f[0] * up[1] - f[1] * up[0];
  if (!(fin[0] && fin[1] && fin[2] && fin[3] && fin[4] && fin[5]) || !(fl > 1e-9 && fl < 1e15)) return CAM_BAD_VIEW;
  if (!(fin[6] && fin[7] && fin[8]) || !(ul > 0 && ul < 1e15 && sqrt(cx * cx + cy * cy + cz * cz) > 1e-6 * fl * ul)) return CAM_BAD_UP;
  if (!fin[CAM_FOV] || !(c[CAM_FOV] > 0.f && c[CAM_FOV] < 180.f)) return CAM_BAD_FOV;
  if (!fin[CAM_ASPECT] || !(c[CAM_ASPECT] > 0.f && c[CAM_ASPECT] < 1e15f)) return CAM_BAD_ASPECT;
  if (!fin[CAM_NEAR] || !(c[CAM_NEAR] > 0.f && c[CAM_NEAR] < 1e15f)) return CAM_BAD_NEAR;
  if (!fin[CAM_FAR] || !(c[CAM_FAR] > c[CAM_NEAR] && c[CAM_FAR] < 1e15f)) return CAM_BAD_FAR;
  return CAM_OK;
}

// The camera a kernel (or the host build) uses: `cam` if it passes cam_degenerate, else `preset` -- so that the scene stays finite; the env
// then gets the background.  -> the code of cam_degenerate.  flags != nullptr: `preset` is the peg-in-hole wrist preset, which is given in
// the PIH_RENDER_CAM_EE_POS frame whatever frame flag the call carries.
PIH_HHD int camera_or_preset(FlyCam& cam, const FlyCam& preset, int* flags = nullptr) {
  const int code = cam_degenerate(cam.w);
  if (code != CAM_OK) {
    cam = preset;
    if (flags) *flags = (*flags & ~PIH_RENDER_CAM_EE) | PIH_RENDER_CAM_EE_POS;
  }
  return code;
}
// row `e` of a [count, N] array of per-env cameras (floats) or lights (words as integers: pih_lit.h), if there is one: N wave-uniform loads
template <class T, int N> PIH_HD void load_row(T (&dst)[N], const T* rows, int e) {
  if (rows) {
#pragma unroll
    for (int i = 0; i < N; i++) dst[i] = rows[(size_t)e * N + i];
  }
}
// the words of env `env`'s state record the camera needs; word k of the env is state[k * n + env] (the library's structure-of-arrays state:
// 13 wave-uniform loads; an env-major record of the host build: env = 0, n = 1)
template <class T> PIH_HD FlyPose load_fly_pose(const T* state, int env, int n) {
  FlyPose ps;
  const T* rec = state + env;
#pragma unroll
  for (int i = 0; i < RCAP; i++) ps.q[i] = (real)rec[(size_t)(PIH_F_Q + i) * n];
#pragma unroll
  for (int i = 0; i < 3; i++) ps.opos[i] = (real)rec[(size_t)(PIH_F_OPOS + i) * n];
#pragma unroll
  for (int i = 0; i < 4; i++) ps.oquat[i] = (real)rec[(size_t)(PIH_F_OQUAT + i) * n];
  return ps;
}

// The pixel grid, shared by the kernel and the host build: pixel-centre and tile-edge coordinates on the camera plane
struct FlyGrid {
  real sx, sy, tx, ty;
  PIH_HD FlyGrid(real tx_, real ty_, int W, int H) : sx((real)2 / (real)W), sy((real)2 / (real)H), tx(tx_), ty(ty_) {}      // (the wrist camera: constants)
  template <class S /* FlyScene, view::ViewScene */> PIH_HD FlyGrid(const S& sc, int W, int H) : FlyGrid(sc.tx, sc.ty, W, H) {}
  PIH_HD real xc(int j) const { return (sx * ((real)j + (real)0.5) - (real)1) * tx; }
  PIH_HD real yc(int i) const { return ((real)1 - sy * ((real)i + (real)0.5)) * ty; }
  PIH_HD real xedge(int j) const { return (sx * (real)j - (real)1) * tx; }
  PIH_HD real yedge(int i) const { return ((real)1 - sy * (real)i) * ty; }
};
constexpr int TILE_ROWS = 16, TILE_COLS = 64;        // one row of a tile per wave instruction

// the three formats of one pixel of an unlit free camera, as render_image takes them: pixel_* of the scene's namespace (fly, view)
template <class S, class MASK> struct Pixels {
  const S& sc; int flags; bool bad;
  PIH_HD unsigned as_rgba8(MASK prims, real xc, real yc) const { return pixel_rgba8(sc, prims, xc, yc, flags, bad); }
  PIH_HD real as_depth(MASK prims, real xc, real yc) const { return pixel_depth(sc, prims, xc, yc, bad); }
  PIH_HD real4 as_float4(MASK prims, real xc, real yc) const { return pixel_float4(sc, prims, xc, yc, flags, bad); }
};
// what a set-up hooks in for a camera without a caller-given light (pih_lit.h has the one with)
struct NoLight {
  static constexpr int LIGHT_THREAD = -1;      // no thread of the workgroup
  PIH_HD void light_thread(unsigned long long) const {}
  template <class S> PIH_HD void table(const S&, int) const {}
  PIH_HD bool bad() const { return false; }
};

#ifndef PIH_PLATFORM_DEFINED      // ---------------------------------------------------------------- device only: the kernels' shared pieces
// THE tile walk of the camera kernels.  The workgroup renders rows r0 .. r1 - 1 of its env's image (whose row 0 is row `row0` of out, W values a row: the index stays in size_t): each WAVE
// walks 16-row x 64-column tiles; lane i tests primitive i against the tile (prim_on_tile of the scene's namespace), the ballot is the
// tile's primitive list (MASK: unsigned for the scenes of <= 32 primitives, unsigned long long for view::ViewScene); then one pixel per
// lane, pixel(prims, xc, yc) -> the stored value: one tile row is one coalesced store of 64 values.
template <class MASK, class S, class PX, class F>
PIH_HD void render_strip(const S& sc, const FlyGrid& g, PX* __restrict__ out, size_t row0, int W, int r0, int r1, int tid, const F& pixel) {
  const int lane = tid & 63, wave = tid >> 6;
  const int tcols = (W + TILE_COLS - 1) / TILE_COLS, trows = (r1 - r0 + TILE_ROWS - 1) / TILE_ROWS;
  for (int tile = wave; tile < tcols * trows; tile += RENDER_THREADS / 64) {
    const int ti = tile / tcols, tj = tile - ti * tcols;
    const int i0 = r0 + ti * TILE_ROWS, i1 = min(r1, i0 + TILE_ROWS), j0 = tj * TILE_COLS, j1 = min(W, j0 + TILE_COLS);
    // camera-plane rectangle of the tile's pixel edges (row 0 is the top of the image, v grows upwards)
    const MASK prims = (MASK)__ballot(prim_on_tile(sc, lane, g.xedge(j0), g.xedge(j1), g.yedge(i1), g.yedge(i0)));
    const int j = j0 + lane;
    if (j < j1) {
      const float xc = g.xc(j);
      for (int i = i0; i < i1; i++) out[(row0 + (size_t)i) * W + j] = pixel(prims, xc, g.yc(i));
    }
  }
}
PIH_HD float4 to_float4(const real4& c) { return make_float4(c.x, c.y, c.z, c.w); }
// the walk in the output format FMT (0: float4 (depth, r, g, b) | PIH_RENDER_OUT_RGBA8: one 32-bit word | PIH_RENDER_OUT_DEPTH: one float):
// the format picks the pointer type and the pixel function of `px` (Pixels, lit::LitPixels) once, outside the loops
template <int FMT, class MASK, class S, class P>
PIH_HD void render_image(const S& sc, const FlyGrid& g, void* __restrict__ out, size_t row0, int W, int r0, int r1, int tid, const P& px) {
  if constexpr (FMT == PIH_RENDER_OUT_RGBA8)
    render_strip<MASK>(sc, g, static_cast<unsigned*>(out), row0, W, r0, r1, tid, [&](MASK prims, real xc, real yc) { return px.as_rgba8(prims, xc, yc); });
  else if constexpr (FMT == PIH_RENDER_OUT_DEPTH)
    render_strip<MASK>(sc, g, static_cast<float*>(out), row0, W, r0, r1, tid, [&](MASK prims, real xc, real yc) { return px.as_depth(prims, xc, yc); });
  else
    render_strip<MASK>(sc, g, static_cast<float4*>(out), row0, W, r0, r1, tid, [&](MASK prims, real xc, real yc) { return to_float4(px.as_float4(prims, xc, yc)); });
}
// The scene set-up of a random-fly camera kernel with per-env cameras (every thread of the workgroup calls it; two barriers): threads
// 0 .. 15 read the env's pose and camera row, thread RCAP tests the camera (camera_or_preset) and leaves the code in cam_bad, `hook` adds
// the light (NoLight, lit::LightHook), then the scene's two phases.  -> the env gets the background
template <class Hook>
PIH_HD bool camera_setup(FlyScene& sc, int& cam_bad, const Hook& hook, const float* __restrict__ state, FlyCam& cam, const float* __restrict__ cam_dev,
                        int n, int object, int env, int e, int flags, int tid) {
  if (tid < 16) {
    const FlyPose ps = load_fly_pose(state, env, n);
    load_row(cam.w, cam_dev, e);
    if (tid == RCAP) cam_bad = camera_or_preset(cam, FlyCam{PIH_FLY_CAM_DEFAULT});
    if (tid == Hook::LIGHT_THREAD) hook.light_thread(all_prims(object));
    scene_setup_poses(sc, ps, cam, object, flags, tid);
  }
  __syncthreads();
  scene_setup_bounds(sc, object, tid);
  hook.table(sc, tid);
  __syncthreads();
  return cam_bad != CAM_OK || hook.bad();
}
// the instance of a kernel template for a call's output format: launch(std::integral_constant<int, FMT>) launches kernel<FMT>
template <class F> inline void dispatch_fmt(int fmt, F&& launch) {
  if (fmt == PIH_RENDER_OUT_RGBA8) launch(std::integral_constant<int, PIH_RENDER_OUT_RGBA8>());
  else if (fmt == PIH_RENDER_OUT_DEPTH) launch(std::integral_constant<int, PIH_RENDER_OUT_DEPTH>());
  else launch(std::integral_constant<int, 0>());
}
#endif

}  // namespace fly
}  // namespace pih
