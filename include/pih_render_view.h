/* pih_render_view.h -- C ABI of the free camera of the peg-in-hole task (libpih_hip.so); an addition to pih.h, which includes this file:
 * include pih.h.  The ABI version stays PIH_ABI_VERSION.
 * Why a file of its own: tests/test_fly_render.py pins the number of functions pih.h declares (_lib.EXPORTS, 22), and
 * tests/test_abi_exports.py compares that list with pih.h.  So test_every_declared_symbol_is_exported does NOT cover what is declared
 * here; tests/test_peg_view.py does (_lib.VIEW_EXPORTS against this file, and the symbol in the built library).  Once that pin may move,
 * fold this file back into pih.h and VIEW_EXPORTS into EXPORTS. */
#ifndef PIH_RENDER_VIEW_H
#define PIH_RENDER_VIEW_H
#include "pih.h"
#ifdef __cplusplus
extern "C" {
#endif

/* free camera of the peg-in-hole task (peg-in-hole handles only; a fly handle gets -2, and pih_render_cam keeps rejecting peg-in-hole
 * handles): the scene of pih_render -- table plane (153), 24 pipe capsules and the hole tube (232), the two finger-pad boxes (77) -- plus
 * the arm, seen from any viewpoint.  The Panda's visual meshes are not part of this build; the arm is a BUILD-DEFINED stand-in: link
 * L = 0 .. 6 is a capsule from its parent's origin to its own (radius 0.06, or that of the model's collision sphere at the link's origin:
 * links 3, 4, 5), colour 204; the hand is the model's three hand spheres and the flange sphere, colour 77 like the fingers.
 * Camera words, basis, pixel grid, depth buffer, clipping to [near, far] and the output formats are those of pih_render_cam; the call
 * reads the CURRENT state and changes none of it.  out_dev 16-byte aligned, any width, height >= 1, env_count <= 65535.
 * cam: HOST float[PIH_CAM_WORDS], one camera for all envs of the call; a degenerate one returns -2 and pih_last_error names the field.
 *   NULL = the wrist preset: PIH_VIEW_CAM_WRIST with PIH_RENDER_CAM_EE_POS, the camera of PegInHole.render, whatever frame flag is passed.
 * flags (every other bit: -2):
 *   PIH_RENDER_SHADED      ambient + diffuse as in pih_render_ex
 *   PIH_RENDER_CAM_EE      eye, target and up are given in the grasp-target frame (pybullet link 11): the camera turns with the hand
 *   PIH_RENDER_CAM_EE_POS  eye and target are offset by the grasp-target's position, the axes stay env-local: the camera follows the hand
 *                          and does not turn with it (the reference's wrist camera).  Both frame flags: -2.  Neither: the env-local frame
 *   PIH_RENDER_OUT_RGBA8   uint8[env_count, height, width, 4] = (r, g, b, seg), bytes rounded as in pih_render_cam; seg = arm link 0 .. 6
 *                          (the hand is 6), fingers 7 and 8, PIH_VIEW_SEG_HOLE, PIH_VIEW_SEG_TABLE, PIH_VIEW_SEG_PIPE0 + pipe capsule
 *                          0 .. 23, PIH_SEG_NONE
 *   PIH_RENDER_OUT_DEPTH   float[env_count, height, width].  Both formats: -2.  Neither: float[env_count, height, width, 4] = (depth, r, g, b)
 *   PIH_RENDER_CAM_DEVICE  cam is a DEVICE pointer float[env_count, PIH_CAM_WORDS] (NULL: -2), read and tested by the kernel: an env whose
 *                          row is degenerate or holds a NaN gets the background (depth 1, rgb 255, seg PIH_SEG_NONE); the call returns 0 */
#define PIH_RENDER_CAM_EE_POS 32
#define PIH_VIEW_CAM_WRIST {0.f, 0.f, 0.f,  0.f, 0.f, -10.f,  0.f, 1.f, 0.f,  60.f, 1.f, 0.001f, 1000.f}   /* with PIH_RENDER_CAM_EE_POS */
#define PIH_VIEW_CAM_OVERVIEW {1.33f, -0.02f, 1.05f,  0.05f, -0.25f, 0.3f,  0.f, 0.f, 1.f,  40.f, 1.f, 0.01f, 100.f}   /* BUILD-DEFINED third-person default, env-local: the whole arm (the shoulder sphere of link 1 included), pipe, hole and table at the rest pose */
#define PIH_VIEW_SEG_HOLE 9
#define PIH_VIEW_SEG_TABLE 10
#define PIH_VIEW_SEG_PIPE0 32
int pih_render_view(pih_handle* h, void* out_dev, const float* cam /* as pih_render_cam; NULL = the wrist preset */,
                    int width, int height, int env_begin, int env_count, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
