// pih_device.h -- the per-env step of the MI355X-native peg-in-hole environment (ONE WAVEFRONT PER ENV), assembled:
//   pih_common.h  model tables, LDS layout, kinematics helpers, IK, reset, controller, collision, impulse responses, row build
//   pih_ikq.h     the IK with one env per quad of lanes (pih_ik, pih_ik_ur5)
//   pih_wave.h    the gfx950 wave layer: wave context + the phases written with DPP / ds_bpermute / v_readlane (FK and velocity
//                 scans, ABA inward sweep, PGS); the env wavefront's side of the fused-launch handshake
//   pih_mailbox.h the handshake of the fused launch (controller wavefronts -> mailbox -> step wavefronts), both tasks
//   pih_step.h    articulated-body forward dynamics and the step itself
// Included by the kernel translation units (pih_peg.hip, pih_fly.hip and, through pih_render.h, the cameras); the C ABI (pih_hip.hip)
// includes none of it.
// gfx950 only: there is no host path in the product (libpih_hip.so); the test harness in tests/emul brings its own wave layer.
#pragma once
#include "pih_common.h"
#include "pih_ikq.h"
#include "pih_wave.h"
#include "pih_step.h"
