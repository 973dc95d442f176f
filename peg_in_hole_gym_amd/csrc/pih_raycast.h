// pih_raycast.h -- the task-independent pieces of the analytic ray casters: ray-vs-sphere / capsule, the radial normal of a capsule, the
// conservative screen bound of a sphere, and the light and colour constants all cameras share (the wrist camera of pih_render.h, the free
// cameras of pih_fly_render.h and pih_view.h).
#pragma once
#include "pih_common.h"

namespace pih {

constexpr int RENDER_THREADS = 256;
#define PIH_COL_BG ((real)255)
#define PIH_COL_TABLE ((real)153)
// TinyRenderer defaults as driven by getCameraImage without light arguments [UNVERIFIED restatement; pybullet is absent: parity
// unpinned]: light direction (-50, 30, 100) normalised (z-up world), ambient 0.6, diffuse 0.35.  The cameras that use these constants
// stop there; the specular term (0.05), cast shadows and a caller-given light are pih_render_lit's (pih_lit.h)
#define PIH_LIGHT_X ((real)-0.43193421279068006)
#define PIH_LIGHT_Y ((real)0.25916052767440806)
#define PIH_LIGHT_Z ((real)0.86386842558136012)
#define PIH_LIGHT_AMBIENT ((real)0.6)
#define PIH_LIGHT_DIFFUSE ((real)0.35)

PIH_HD real ray_sphere(V3 oc, V3 d, real r) {   // oc = eye - centre, d unit
  real b = dot(oc, d), c = dot(oc, oc) - r * r, disc = b * b - c;
  real t = -b - (real)sqrt(max_(disc, (real)0));
  return (disc >= 0 && t > 0) ? t : PIH_BIG;
}
PIH_HD real ray_capsule(V3 o, V3 d, V3 a, V3 b, real r) {
  V3 ba = b - a, oa = o - a;
  real baba = dot(ba, ba), bard = dot(ba, d), baoa = dot(ba, oa), rdoa = dot(d, oa), oaoa = dot(oa, oa);
  real A = baba - bard * bard, B = baba * rdoa - baoa * bard, C = baba * oaoa - baoa * baoa - r * r * baba;
  real h = B * B - A * C, best = PIH_BIG;
  if (h >= 0 && A > (real)1e-18) {
    real t = (-B - (real)sqrt(h)) / A, y = baoa + t * bard;
    if (y > 0 && y < baba && t > 0) best = t;
  }
  real t1 = ray_sphere(oa, d, r), t2 = ray_sphere(o - b, d, r);
  best = t1 < best ? t1 : best;
  best = t2 < best ? t2 : best;
  return best;
}
// outward unit normal of the capsule a .. b at the point ph of its surface (a == b: a sphere)
PIH_HD V3 capsule_normal(V3 ph, V3 a, V3 b) {
  const V3 ba = b - a;
  real q = dot(ph - a, ba) / max_(dot(ba, ba), (real)1e-20);
  q = q < 0 ? (real)0 : (q > 1 ? (real)1 : q);
  const V3 r = ph - (a + q * ba);
  return ((real)1 / max_(norm(r), (real)1e-12)) * r;
}
// conservative screen-space bound (in tan-angle units: u = x / depth, v = y / depth) of a sphere; false = cannot bound
// (sphere reaches the eye plane), the caller then keeps the primitive for every strip
PIH_HD bool sphere_bound(V3 rel, real r, real& u0, real& u1, real& v0, real& v1) {
  real dpt = -rel.z;                      // depth along the view axis
  if (dpt <= r + (real)1e-4) return false;
  real u = rel.x / dpt, v = rel.y / dpt;
  real rho = r * (real)sqrt((real)1 + u * u + v * v) / (dpt - r) * (real)1.5 + (real)1e-4;   // generous
  u0 = u - rho; u1 = u + rho; v0 = v - rho; v1 = v + rho;
  return true;
}

}  // namespace pih
