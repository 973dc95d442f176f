// pih_lit.h -- lit camera images of both tasks (pih_render_lit, include/pih_render_light.h): the scenes, cameras, pixel grids and output
// formats of pih_fly_render.h (random-fly) and pih_view.h (peg-in-hole) under a caller-given light, with a specular term and cast shadows.
// The model is stated once, in include/pih_render_light.h; lit_rgb and the two *_shadowed functions below restate it.
//
// The primary ray is the unlit cameras': the scene's walk (fly::nearest_hit, view::nearest_hit with fly::CameraRay), its normal
// (fly::kind_normal, view::hit_normal), fly::depth_value and, for the depth-only format, the scene's own pixel_depth.  What is here is the
// light: its test and set-up, the light-space table, the shadow ray (an ANY-hit walk with a cull of its own, so not the scenes' nearest-hit
// walk) and the colour model.
//
// The shadow ray is the hot path, and the screen-space tile lists are no use for it: an occluder may be anywhere, behind the eye included.
// So each workgroup builds a LIGHT-SPACE table once (light_table_*): per primitive the centre of its bounding sphere projected on two axes
// ex, ey perpendicular to l, the sphere's radius (plus LIT_CULL_SLACK) and the centre's depth along l.  A pixel projects the origin of its
// shadow ray the same way and skips a primitive whose disc does not hold that point or that lies wholly behind it, before any
// intersection.  The skip is conservative, so images with and without it are identical bit for bit (tests/test_render_lit.py).
// Workgroup-uniform branches: shadow factor 1 -> no shadow ray; specular coefficient 0 -> no exp2 / log2.
// The occluders are walked with a scalar bit scan over a mask read from LDS: a counted loop, or a scan of a compile-time mask, is unrolled
// into one intersection routine per primitive (the lesson pih_view.h records).
// Everything here is PIH_HD on `real`: the host build of tests/emul/pih_lit_emul.cpp compiles the same code in fp64 and fp32.
#pragma once
#include "pih_view.h"

namespace pih {
namespace lit {

using fly::FlyScene;
using view::ViewScene;

// the light as the caller gives it: the BIT PATTERNS of its PIH_LIGHT_WORDS floats (passed to the kernel by value).  Integers, because the
// library is built with -ffast-math: a test of a float VALUE for NaN or infinity -- also one written on its bits -- is folded to "finite"
// (on the host a NaN coefficient passed that way, on the device a NaN colour).  The words stay integers from the caller's memory to
// light_degenerate; word_value makes the float of a word that has passed.
struct LightWords { unsigned w[PIH_LIGHT_WORDS]; };
enum : int { LW_DIR = 0, LW_COLOUR = 3, LW_AMBIENT = 6, LW_DIFFUSE = 7, LW_SPECULAR = 8, LW_SHININESS = 9, LW_SHADOW = 10 };
static_assert(LW_SHADOW + 1 == PIH_LIGHT_WORDS, "light words (include/pih_render_light.h)");
static_assert(sizeof(unsigned) == sizeof(float), "a light word is 32 bits");
#define LIT_CULL_SLACK ((real)1e-3)   // [m] added to every light-space radius: 1000 x the fp32 rounding of a projected position 3 m from the origin
PIH_HHD float word_value(unsigned u) { float f; __builtin_memcpy(&f, &u, sizeof f); return f; }
// words of `n` floats in memory, read as integers
PIH_HHD LightWords light_words(const float* p) { LightWords lw; __builtin_memcpy(lw.w, p, sizeof lw.w); return lw; }

// Is the light degenerate?  -> 0 or the code of the first field that is (LIT_LIGHT_FIELD_NAMES: what pih_last_error says).  The host validates
// a light it can read with this; a light in device memory (PIH_RENDER_LIGHT_DEVICE) is tested by the kernel, once per workgroup, and a
// degenerate one gives its env the background.  A word that is not finite is found first, by its exponent bits; with finite words no
// expression below can produce a NaN.
enum : int { LIGHT_OK = 0, LIGHT_BAD_DIRECTION = 1, LIGHT_BAD_COLOUR = 2, LIGHT_BAD_AMBIENT = 3, LIGHT_BAD_DIFFUSE = 4, LIGHT_BAD_SPECULAR = 5, LIGHT_BAD_SHININESS = 6, LIGHT_BAD_SHADOW = 7 };
#define LIT_LIGHT_FIELD_NAMES {nullptr, "direction is zero or not finite", "colour < 0 or not finite", "ambient < 0 or not finite", "diffuse < 0 or not finite", \
                               "specular < 0 or not finite", "shininess <= 0 or not finite", "shadow factor outside [0, 1]"}
PIH_HHD int light_field(int word) { return word < LW_COLOUR ? LIGHT_BAD_DIRECTION : (word < LW_AMBIENT ? LIGHT_BAD_COLOUR : LIGHT_BAD_AMBIENT + word - LW_AMBIENT); }
PIH_HHD int light_degenerate(const LightWords& lw) {
  for (int i = 0; i < PIH_LIGHT_WORDS; i++)
    if ((lw.w[i] & 0x7f800000u) == 0x7f800000u) return light_field(i);
  float w[PIH_LIGHT_WORDS];
  for (int i = 0; i < PIH_LIGHT_WORDS; i++) w[i] = word_value(lw.w[i]);
  const double len = sqrt((double)w[0] * w[0] + (double)w[1] * w[1] + (double)w[2] * w[2]);
  if (!(len > 1e-9 && len < 1e15)) return LIGHT_BAD_DIRECTION;
  for (int k = 0; k < 3; k++)
    if (!(w[LW_COLOUR + k] >= 0.f && w[LW_COLOUR + k] < 1e15f)) return LIGHT_BAD_COLOUR;
  for (int k = 0; k < 3; k++)
    if (!(w[LW_AMBIENT + k] >= 0.f && w[LW_AMBIENT + k] < 1e15f)) return LIGHT_BAD_AMBIENT + k;
  if (!(w[LW_SHININESS] > 0.f && w[LW_SHININESS] < 1e15f)) return LIGHT_BAD_SHININESS;
  if (!(w[LW_SHADOW] >= 0.f && w[LW_SHADOW] <= 1.f)) return LIGHT_BAD_SHADOW;
  return LIGHT_OK;
}

// one env's light and its light-space table of N occluders, in LDS
template <int N> struct LitEnv {
  real l[3], ex[3], ey[3];                  // unit direction towards the light; two unit axes perpendicular to it and to each other
  real colour[3], ambient, diffuse, specular, shininess, shadow;
  real occ[N][4];                           // per primitive: bounding-sphere centre . ex, . ey, radius (with LIT_CULL_SLACK), centre . l
  unsigned long long mask;                  // the occluders to walk: bit i = primitive i exists
  int bad;                                  // light_degenerate's code (the words above are then PIH_LIGHT_DEFAULT's)
};

// the light of the workgroup's env (one thread): tests it, replaces a degenerate one by the default so that everything stays finite
template <int N> PIH_HD void light_setup(LitEnv<N>& le, const LightWords& lw, unsigned long long mask) {
  const int code = light_degenerate(lw);
  const float def[PIH_LIGHT_WORDS] = PIH_LIGHT_DEFAULT;
  real w[PIH_LIGHT_WORDS];
  for (int i = 0; i < PIH_LIGHT_WORDS; i++) w[i] = (real)(code != LIGHT_OK ? def[i] : word_value(lw.w[i]));
  V3 l = mk(w[LW_DIR], w[LW_DIR + 1], w[LW_DIR + 2]);
  l = rsqrt_(dot(l, l)) * l;
  V3 ex = absr(l.x) < (real)0.9 ? mk(0, -l.z, l.y) : mk(l.z, 0, -l.x);      // l x (1, 0, 0) | (0, 1, 0) x l ... whichever is well away from 0
  ex = rsqrt_(dot(ex, ex)) * ex;
  st3(le.l, l); st3(le.ex, ex); st3(le.ey, cross(l, ex));
  for (int k = 0; k < 3; k++) le.colour[k] = w[LW_COLOUR + k];
  le.ambient = w[LW_AMBIENT]; le.diffuse = w[LW_DIFFUSE]; le.specular = w[LW_SPECULAR];
  le.shininess = w[LW_SHININESS]; le.shadow = w[LW_SHADOW];
  le.mask = mask; le.bad = code;
}
// after scene_setup_poses and light_setup, and a barrier (threads 0 .. N - 1): the light-space entry of primitive `tid` of the scene, from
// the sphere that holds it (prim_ball of the scene's header) grown by LIT_CULL_SLACK
template <class S, int N> PIH_HD void light_table(const S& sc, LitEnv<N>& le, int tid) {
  if (tid >= N) return;
  const fly::Ball b = prim_ball(sc, tid, LIT_CULL_SLACK);
  le.occ[tid][0] = dot(b.c, ld3(le.ex)); le.occ[tid][1] = dot(b.c, ld3(le.ey)); le.occ[tid][2] = b.r; le.occ[tid][3] = dot(b.c, ld3(le.l));
}
// the origin of a shadow ray in light space, and the test a primitive has to pass before it is intersected
struct LightPoint { real x, y, depth; };
template <int N> PIH_HD LightPoint to_light(const LitEnv<N>& le, V3 o) { LightPoint p; p.x = dot(o, ld3(le.ex)); p.y = dot(o, ld3(le.ey)); p.depth = dot(o, ld3(le.l)); return p; }
template <int N> PIH_HD bool may_occlude(const LitEnv<N>& le, int i, const LightPoint& p) {
  const real dx = le.occ[i][0] - p.x, dy = le.occ[i][1] - p.y, r = le.occ[i][2];
  return dx * dx + dy * dy <= r * r && le.occ[i][3] + r >= p.depth;
}
// the table plane occludes what the shadow ray crosses it for: only a light from below, and then everything above the table
PIH_HD bool table_occludes(V3 o, V3 l) { return l.z < 0 && ((real)PIH_TABLE_Z - o.z) / l.z > 0; }

// out_k of the model: base = the flat colour, n = the normal, d = the ray, s = 1 or the shadow factor
template <int N> PIH_HD void lit_rgb(const LitEnv<N>& le, const real* base, V3 n, V3 d, real ndl, real s, real4& o) {
  const V3 l = ld3(le.l);
  real spec = 0;
  if (le.specular != 0) {                   // (workgroup-uniform)
    const V3 r = (2 * ndl) * n - l;
    const real x = max_((real)0, -dot(r, d));
    spec = (ndl > 0 && x > 0) ? (real)exp2(le.shininess * (real)log2(x)) : (real)0;
  }
  const real direct = s * (le.diffuse * max_(ndl, (real)0) + le.specular * spec);
  const real r = base[0] * (le.ambient + le.colour[0] * direct), g = base[1] * (le.ambient + le.colour[1] * direct), b = base[2] * (le.ambient + le.colour[2] * direct);
  o.y = r < 255 ? r : (real)255; o.z = g < 255 ? g : (real)255; o.w = b < 255 ? b : (real)255;
}

// ------------------------------------------------------------------------------------------------ random-fly (the scene of pih_fly_render.h)
using fly::FLY_NPRIM;
using fly::RCAP;
typedef LitEnv<FLY_NPRIM> FlyLit;

// does the ray from o towards the light hit an occluder?  cull: use the light-space table (false: the host build's check of it)
PIH_HD bool shadowed(const FlyScene& sc, const FlyLit& le, V3 o, bool cull) {
  const V3 l = ld3(le.l);
  if (table_occludes(o, l)) return true;
  const LightPoint p = to_light(le, o);
  bool sh = false;
  unsigned m = (unsigned)le.mask;
  while (m) {
    const int i = __builtin_ctz(m); m &= m - 1u;
    if (sh || (cull && !may_occlude(le, i, p))) continue;
    const real t = i < RCAP ? ray_capsule(o, l, ld3(sc.cap[i][0]), ld3(sc.cap[i][1]), sc.capr[i]) : ray_sphere(o - ld3(sc.sph[i - RCAP]), l, sc.sphr[i - RCAP]);
    sh = t < PIH_BIG;
  }
  return sh;
}

// one lit pixel: (depth value, r, g, b); kind_out = what the ray hit
PIH_HD real4 lit_kind(const FlyScene& sc, const FlyLit& le, unsigned prims, real xc, real yc, bool cull, int& kind_out) {
  const fly::CameraRay ray = fly::camera_ray(sc, xc, yc);
  const fly::FlyHit h = fly::nearest_hit(sc, prims, ray);
  real4 o; o.x = fly::depth_value(sc, ray, h.t, h.kind != fly::KIND_NONE); o.y = sc.rgb[h.kind][0]; o.z = sc.rgb[h.kind][1]; o.w = sc.rgb[h.kind][2];
  kind_out = h.kind;
  if (h.kind == fly::KIND_NONE) return o;
  const V3 ph = ray.o + h.t * ray.d, n = fly::kind_normal(sc, h, ph);
  const real ndl = dot(n, ld3(le.l));
  real s = 1;
  if (le.shadow != 1 && ndl > 0 && shadowed(sc, le, ph + (real)PIH_SHADOW_BIAS * n, cull)) s = le.shadow;
  lit_rgb(le, sc.rgb[h.kind], n, ray.d, ndl, s, o);
  return o;
}
// the two coloured formats of one pixel (`bad`: the env's camera or light is degenerate, wave-uniform); the depth-only one is fly::pixel_depth
PIH_HD real4 pixel_float4(const FlyScene& sc, const FlyLit& le, unsigned prims, real xc, real yc, bool cull, bool bad) {
  int kind;
  return bad ? fly::background() : lit_kind(sc, le, prims, xc, yc, cull, kind);
}
PIH_HD unsigned pixel_rgba8(const FlyScene& sc, const FlyLit& le, unsigned prims, real xc, real yc, bool cull, bool bad) {
  int kind = fly::KIND_NONE;
  const real4 c = bad ? fly::background() : lit_kind(sc, le, prims, xc, yc, cull, kind);
  return fly::pack_rgba8(c, kind);
}

// ------------------------------------------------------------------------------------------------ peg-in-hole (the scene of pih_view.h)
using view::VIEW_NPRIM;
typedef LitEnv<VIEW_NPRIM> ViewLit;

// does the ray from o towards the light hit an occluder?  The arm's and the pipe's capsules go through ONE call of ray_capsule.
PIH_HD bool shadowed(const ViewScene& sc, const ViewLit& le, V3 o, bool cull) {
  using namespace view;
  const V3 l = ld3(le.l);
  if (table_occludes(o, l)) return true;
  const LightPoint p = to_light(le, o);
  bool sh = false;
  unsigned long long m = le.mask;
  while (m) {
    const int i = __builtin_ctzll(m); m &= m - 1ull;
    if (sh || (cull && !may_occlude(le, i, p))) continue;
    real t;
    if (i < P_HAND || (i >= P_PIPE && i < P_TUBE)) {
      const bool arm = i < P_HAND;
      const real (*v)[3] = arm ? sc.org + i : sc.vtx + (i - P_PIPE);
      t = ray_capsule(o, l, ld3(v[0]), ld3(v[1]), arm ? ARM_R[i] : (real)PIH_PIPE_RADIUS);
    } else if (i < P_BOX) {
      t = ray_sphere(o - ld3(sc.hs[i - P_HAND]), l, ASPH_R[HAND_SPH0 + i - P_HAND]);
    } else if (i < P_PIPE) {
      t = ray_box(o, l, ldm(sc.fR[i - P_BOX]), ld3(sc.fc[i - P_BOX]), ld3(FBOX_H));
    } else {
      t = ray_tube(o, l);
    }
    sh = t < PIH_BIG;
  }
  return sh;
}

// one lit pixel: (depth value, r, g, b); hit_out = what the ray hit
PIH_HD real4 lit_hit(const ViewScene& sc, const ViewLit& le, unsigned long long prims, real xc, real yc, bool cull, int& hit_out) {
  const fly::CameraRay ray = fly::camera_ray(sc, xc, yc);
  const view::ViewHit h = view::nearest_hit(sc, prims, ray);
  const real col = view::hit_colour(h.hit);
  real4 o; o.x = fly::depth_value(sc, ray, h.t, h.hit != view::HIT_NONE); o.y = o.z = o.w = col;
  hit_out = h.hit;
  if (h.hit == view::HIT_NONE) return o;
  const V3 ph = ray.o + h.t * ray.d, n = view::hit_normal(sc, h.hit, ph);
  const real ndl = dot(n, ld3(le.l));
  real s = 1;
  if (le.shadow != 1 && ndl > 0 && shadowed(sc, le, ph + (real)PIH_SHADOW_BIAS * n, cull)) s = le.shadow;
  const real base[3] = {col, col, col};
  lit_rgb(le, base, n, ray.d, ndl, s, o);
  return o;
}
// (the depth-only format is view::pixel_depth)
PIH_HD real4 pixel_float4(const ViewScene& sc, const ViewLit& le, unsigned long long prims, real xc, real yc, bool cull, bool bad) {
  int hit;
  return bad ? fly::background() : lit_hit(sc, le, prims, xc, yc, cull, hit);
}
PIH_HD unsigned pixel_rgba8(const ViewScene& sc, const ViewLit& le, unsigned long long prims, real xc, real yc, bool cull, bool bad) {
  int hit = view::HIT_NONE;
  const real4 c = bad ? fly::background() : lit_hit(sc, le, prims, xc, yc, cull, hit);
  return fly::pack_byte(c.y) | (fly::pack_byte(c.z) << 8) | (fly::pack_byte(c.w) << 16) | (view::seg_of_hit(hit) << 24);
}

// ------------------------------------------------------------------------------------------------ both tasks
// the three formats of one lit pixel, as fly::render_image takes them (`cull`: use the light-space table)
template <class S, class L, class MASK> struct LitPixels {
  const S& sc; const L& le; bool cull, bad;
  PIH_HD unsigned as_rgba8(MASK prims, real xc, real yc) const { return pixel_rgba8(sc, le, prims, xc, yc, cull, bad); }
  PIH_HD real as_depth(MASK prims, real xc, real yc) const { return pixel_depth(sc, prims, xc, yc, bad); }      // (the light does not enter: the scene's own)
  PIH_HD real4 as_float4(MASK prims, real xc, real yc) const { return pixel_float4(sc, le, prims, xc, yc, cull, bad); }
};
// what a lit kernel hooks into its task's camera_setup (fly::NoLight is the unlit kernels'): thread 14 of the workgroup reads the env's row
// of per-env lights, if there are any, and sets the light up (light_setup tests it); the threads that compute the screen bounds then fill
// the light-space table; a degenerate light gives the env the background
template <class L> struct LightHook {
  L& le; LightWords& light; const float* light_dev; int e;
  static constexpr int LIGHT_THREAD = 14;
  PIH_HD void light_thread(unsigned long long occluders /* the mask of the scene's primitives */) const {
    fly::load_row(light.w, reinterpret_cast<const unsigned*>(light_dev), e);      // (as integers: see LightWords)
    light_setup(le, light, occluders);
  }
  template <class S> PIH_HD void table(const S& sc, int tid) const { light_table(sc, le, tid); }
  PIH_HD bool bad() const { return le.bad != LIGHT_OK; }
};

}  // namespace lit
}  // namespace pih
