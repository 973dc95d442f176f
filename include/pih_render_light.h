/* pih_render_light.h -- C ABI of the lit camera images of both tasks (libpih_hip.so): a caller-given light, a specular term and cast
 * shadows on top of the free cameras of the random-fly task, pih_render_cam, and of the peg-in-hole task, pih_render_view; an addition to
 * pih.h, which includes this file: include pih.h.  The ABI version stays PIH_ABI_VERSION.
 * Why a file of its own: the reason pih_render_view.h gives.  tests/test_render_lit.py compares _lib.LIGHT_EXPORTS with this file and looks
 * the symbol up in the built library. */
#ifndef PIH_RENDER_LIGHT_H
#define PIH_RENDER_LIGHT_H
#include "pih.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The image calls above with the light arguments of p.getCameraImage (lightDirection, lightColor, shadow, lightAmbientCoeff,
 * lightDiffuseCoeff, lightSpecularCoeff).  One call serves both tasks:
 *   random-fly handle    the scene of pih_render_cam, with its camera words (NULL = PIH_FLY_CAM_DEFAULT), frames, formats and seg bytes
 *   peg-in-hole handle   the scene of pih_render_view, with its camera words (NULL = the wrist preset), frames, formats and seg bytes
 * flags: what that call accepts, plus PIH_RENDER_LIGHT_DEVICE; PIH_RENDER_SHADED is implied and accepted.  Every rule of the two calls
 * holds: out_dev 16-byte aligned, env_count <= 65535, at most one format, at most one frame, a degenerate host camera returns -2, a
 * degenerate device camera gives its env the background.  Depth and seg are those of the unlit call; PIH_RENDER_OUT_DEPTH ignores the light.
 *
 * light: HOST float[PIH_LIGHT_WORDS], one light for all envs of the call; NULL = PIH_LIGHT_DEFAULT.
 *   words 0 .. 2   direction: points TOWARDS the light, in the env-local frame (also under an eye-in-hand camera); parallel rays; any
 *                  length but 0
 *   words 3 .. 5   colour r, g, b, each >= 0
 *   words 6, 7, 8  ambient, diffuse and specular coefficients, each >= 0
 *   word 9         shininess > 0
 *   word 10        shadow factor in [0, 1]: what is left of the direct light in a shadow; 1 = no shadows (no shadow ray is traced)
 * A word that breaks these rules, or one that is not finite, is a degenerate light: -2, and pih_last_error names the field.
 * PIH_RENDER_LIGHT_DEVICE: light is a DEVICE pointer float[env_count, PIH_LIGHT_WORDS], row e = the light of env env_begin + e, read and
 * tested by the kernel (NULL: -2): an env whose row is degenerate gets the background (depth 1, rgb 255, seg PIH_SEG_NONE) in every
 * format; the call returns 0.
 *
 * THE MODEL.  A ray with unit direction d hits a surface of flat colour `base` at the point p, where the surface normal is n (radial on
 * capsules and spheres, the face normal on boxes and the tube's ends, +z on the table); l = the unit direction towards the light:
 *   ndl   = n . l
 *   r     = 2 ndl n - l                                       (l mirrored at the surface)
 *   x     = max(0, r . (-d))
 *   spec  = (ndl > 0 && x > 0) ? exp2(shininess log2(x)) : 0
 *   s     = the shadow factor if ndl > 0 and the ray from p + PIH_SHADOW_BIAS n towards l hits an occluder at any t > 0; else 1
 *   out_k = min(255, base (ambient + s colour_k (diffuse max(0, ndl) + specular spec)))          k = r, g, b
 * Occluders: every primitive of the env's scene, whether the camera sees it or not -- the clip planes do not apply, and a primitive behind
 * the eye counts (under the wrist preset the whole arm is behind the eye; its shadow falls on the table).  The table plane occludes
 * whatever the shadow ray crosses it for, which happens only for a light from below (l.z < 0).  A shadow ray that starts inside a sphere or
 * a capsule does not hit that primitive.
 * Defaults: direction, ambient 0.6 and diffuse 0.35 are the fixed light of PIH_RENDER_SHADED; specular 0.05, shininess 2 and shadow
 * factor 0.8 restate TinyRenderer's [UNVERIFIED restatement; pybullet is absent: parity unpinned]. */
/* PIH_LIGHT_WORDS = 11 (pih.h): direction xyz, colour rgb, ambient, diffuse, specular, shininess, shadow factor */
#define PIH_LIGHT_DEFAULT {-50.f, 30.f, 100.f,  1.f, 1.f, 1.f,  0.6f, 0.35f, 0.05f,  2.f, 0.8f}
#define PIH_RENDER_LIGHT_DEVICE 64   /* light is a DEVICE pointer float[env_count, PIH_LIGHT_WORDS], one light per env */
#define PIH_SHADOW_BIAS 1e-4         /* [m] the shadow ray starts this far off the surface, along its normal */
int pih_render_lit(pih_handle* h, void* out_dev, const float* cam, const float* light,
                   int width, int height, int env_begin, int env_count, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
