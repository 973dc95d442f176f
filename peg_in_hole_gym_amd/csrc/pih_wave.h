// pih_wave.h -- the gfx950 wave layer of the per-env step: ONE WAVEFRONT (64 lanes, one workgroup) PER ENV.
// The wave context (`Wave`: lane-parallel loops, ballot/popcount stream compaction, shader-clock stamps) and the phases written
// directly with wave primitives: DPP row reductions, ds_bpermute lane exchanges, v_readlane broadcasts, inline v_add_f32_dpp
// row_bcast, 16-byte LDS broadcasts -- forward kinematics as a prefix product of rigid transforms, link velocities as prefix
// sums, the entry-parallel inward sweep of the articulated-body algorithm, and the sequential-impulse PGS.
#pragma once
#include <type_traits>
#include "pih_common.h"
#include "pih_mailbox.h"

namespace pih {

// Debug words PIH_DBG_T_START .. PIH_DBG_XCC_ID (config.debug = 2; tools/sched_trace.py, tools/fly_trace.py): a time of the chip-wide 100 MHz
// clock (s_memrealtime) as three 16-bit pieces, each exact in fp32, and where the wavefront ran (HW_ID, XCC_ID).  Never read by a kernel.
PIH_HD void debug_store_time(real* dbg, int at, long long t) { dbg[at] = (real)(t & 0xFFFF); dbg[at + 1] = (real)((t >> 16) & 0xFFFF); dbg[at + 2] = (real)((t >> 32) & 0xFFFF); }
PIH_HD void debug_store_hw_id(real* dbg) { dbg[PIH_DBG_HW_ID] = (real)(__builtin_amdgcn_s_getreg((15 << 11) | 4) & 0xFFFF); dbg[PIH_DBG_XCC_ID] = (real)__builtin_amdgcn_s_getreg((3 << 11) | 20); }

struct Wave {
  int l;
  int counter;
  static constexpr bool controller_inline = false;          // the controller runs in its own wavefronts (fused launch) or in pih_pre_kernel
  real* dbg = nullptr; int dbgmode = 0; long long t0 = 0, t1 = 0;   // diagnostic shader-clock stamps (config.debug == 2; never read by the kernel)
  PIH_HD void stamp(int k) { if (dbg && dbgmode == 2) { long long t = __builtin_readcyclecounter(); if (l == 0) dbg[PIH_DBG_CYCLES + k] = (real)(t - t0); t0 = t; } }   // sub-phases
  // start / end of the env's wave and where it ran: the launch's dispatch timeline
  PIH_HD void trace(int at, long long t) { if (l != 0) return; debug_store_time(dbg, at, t); if (at == PIH_DBG_T_START) debug_store_hw_id(dbg); }
  PIH_HD void phase_begin() { if (dbg && dbgmode == 2) { t1 = __builtin_readcyclecounter(); trace(PIH_DBG_T_START, (long long)__builtin_amdgcn_s_memrealtime()); } }
  PIH_HD void phase(int k) { if (dbg && dbgmode == 2) { long long t = __builtin_readcyclecounter(); if (l == 0) dbg[PIH_DBG_CYCLES + k] = (real)(t - t1); t1 = t; if (k == 7) trace(PIH_DBG_T_END, (long long)__builtin_amdgcn_s_memrealtime()); } }
  PIH_HD int lane() const { return l; }
  // issue priority of this wavefront among the waves of its SIMD (s_setprio 0..3).  A launch of n envs ends when its heaviest
  // env ends, and that env shares its SIMD with a light one for most of its life: the heavy wave goes first at every issue slot.
  bool prio_on = true;
  PIH_HD void priority(int contacts) {
    if (!prio_on) return;
    if (contacts > 20) __builtin_amdgcn_s_setprio(3);
    else if (contacts > 14) __builtin_amdgcn_s_setprio(2);
    else if (contacts > 10) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
  }
  // Fused launch (pih_step_kernel with a controller role, round 4): the env's controller output arrives in a 16-word mailbox record,
  // published by the controller wavefront of the env's group of 64 (pih_mailbox.h).  After the wait the 13 controller words go into the
  // LDS copy of the state record.  cmail == nullptr: two-launch path (pih_pre_kernel wrote the record before this kernel started), nothing
  // to do.
  const int* cflags = nullptr; const real* cmail = nullptr; int* cerr = nullptr; int cepoch = 0, cenv = 0;
  PIH_HD void await_controller(Shared& sh) {
    if (!cmail) return;
    mailbox_await(cflags + (cenv >> 6), cepoch, cerr, l == 0);
    __syncthreads();
    if (l < 13) {
      const real v = mail_load(cmail + (size_t)cenv * CTRL_WORDS + l);
      const int word = l < 9 ? PIH_S_TARGET + l : (l == 9 ? (int)PIH_S_FSM : l == 10 ? (int)PIH_S_FSMT : l == 11 ? (int)PIH_S_GRASP_ANGLE : (int)PIH_S_ATTACH_QZ);
      sh.S[word] = v;
    }
    __syncthreads();
  }
  PIH_HD void sync() { __syncthreads(); }
  template <class F> PIH_HD void par(int n, F f) {
    __syncthreads();
    for (int b = 0; b < n; b += 64) { int i = b + l; if (i < n) f(i); }
    __syncthreads();
  }
  // all lanes call f(i, in_range) for every chunk so that wave collectives inside f are legal
  template <class F> PIH_HD void par_all(int n, F f) {
    __syncthreads();
    for (int b = 0; b < n; b += 64) { int i = b + l; f(i, i < n); }
    __syncthreads();
  }
  PIH_HD void alloc_reset(int base) { counter = base; }
  PIH_HD int alloc_count() const { return counter; }
  PIH_HD int alloc(bool valid) {   // must be reached by all 64 lanes
    unsigned long long m = __ballot(valid);
    int slot = counter + __popcll(m & ((1ull << l) - 1ull));
    counter += __popcll(m);
    return valid ? slot : -1;
  }
};
// ------------------------------------------------------------------------------------------------ cross-lane helpers
// Two floats in one 64-bit VGPR pair, so that z += b * s moves both halves in ONE instruction (v_pk_fma_f32, s a wave-uniform scalar:
// gs_row2_* below).  Written
// as asm on an integer container on purpose: with float2 vector types this toolchain emits the packed FMA but then reads the wrong
// half of the pair in a following v_readlane (checked on the MI355X); the integer form extracts sub-registers correctly.
typedef unsigned long long pk2;
PIH_HD pk2 pk_pack(real x, real y) { return (pk2)__builtin_bit_cast(unsigned, x) | ((pk2)__builtin_bit_cast(unsigned, y) << 32); }
PIH_HD real pk_lo(pk2 v) { return __builtin_bit_cast(float, (unsigned)v); }
PIH_HD real pk_hi(pk2 v) { return __builtin_bit_cast(float, (unsigned)(v >> 32)); }
// acc += J * w on both halves, w a wave-uniform value held in the LOW (pk_fma_lo) or HIGH (pk_fma_hi) half of the VGPR pair w2
PIH_HD void pk_fma_lo(pk2& acc, pk2 j, pk2 w2) { __asm__("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(j), "v"(w2)); }
PIH_HD void pk_fma_hi(pk2& acc, pk2 j, pk2 w2) { __asm__("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(j), "v"(w2)); }
PIH_HD real rdlane(real v, int lane) {   // broadcast one lane's value (lane must be wave-uniform): v_readlane_b32
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// (x[G] = y[G] for ONE lane G known at compile time -- the "commit" of a row's multiplier -- is  s_lshl_b64 mask, 1, G ; v_cndmask :
//  the lane mask is made on the spot by the scalar unit, as a 64-bit constant operand it would be hoisted out of the solver loop, one
//  SGPR pair per row, and spilled.)
// One Gauss-Seidel row of the two-rows-per-lane solver (pgs_rows2) as ONE issue-ordered block:
//     cand = med3(z, lo, hi);  dl = cand - lam;  sdl = dl[lane G];  lam[G] = cand[G];  zz += col * sdl   (both halves, v_pk_fma_f32)
// (z: the half of zz the row lives in; G: its compile-time lane.)  A wave alone on its SIMD issues one instruction of ANY kind per
// 4 cycles, so what a row costs is its instruction count -- s_nop, s_waitcnt and scalar bookkeeping included -- and the heaviest env
// of a launch, which is what the launch waits for, runs this row 4 800 times per step.  Left to the scheduler a row came out as
// med3, sub, (s_lshl, cndmask), s_nop, readlane, s_waitcnt, pk_fma, s_nop; here the hazards of the gfx940 family are covered by
// instructions the row needs anyway: a VALU result is read by v_readlane one instruction later at the earliest (s_lshl_b64 sits
// between), and the SGPR a v_readlane wrote is read by the FMA two instructions later at the earliest (v_cndmask and the normal row's
// second v_readlane, or one s_nop in a friction row).  The broadcast travels through the fixed pair s[100:101] (an asm operand cannot
// name the low half of a 64-bit scalar operand; the high half is never read: op_sel_hi 0 takes the low half for both products).
// Normal row: also s0 = cand[G], the new normal multiplier the friction bounds follow.  INVARIANT (the compiler's hazard recognizer does
// not look inside an asm block, so every block must be safe by itself): s0's v_readlane is the THIRD instruction of the block
// -- one instruction after the v_max that produced cand, four before the block ends -- so the two wait states between a VALU write of
// an SGPR and a VALU read of it have passed whatever the scheduler places right after the block (round-3 review: it used to be the
// second-to-last instruction and relied on scalar compare / branch instructions happening to follow).  Order in a normal row:
//     v_max cand ; v_sub dl ; v_readlane s0 <- cand ; v_readlane s100 <- dl ; s_lshl mask ; v_cndmask lam ; v_pk_fma (reads s100).
// (A normal row's upper bound is PIH_BIG: its clamp is max(z, lo) -- TWO vector sources.  v_med3_f32 with three different VGPRs pays a
//  register-bank conflict whenever the allocator puts two of them in one bank; with that clamp in every row, builds whose loops were
//  instruction for instruction the same ran at 1 640 or 1 716 cycles per iteration.  The motor rows' bounds are symmetric: -hi, hi.)
PIH_HD void gs_row2_normal(pk2& zz, real z, pk2 col, real lo, real& lam, int G, real& dl, real& s0) {
  real cand; unsigned long long m;
  __asm__ volatile("v_max_f32 %0, %6, %7\n\tv_sub_f32 %1, %0, %3\n\tv_readlane_b32 %2, %0, %9\n\tv_readlane_b32 s100, %1, %9\n\t"
                   "s_lshl_b64 %4, 1, %9\n\tv_cndmask_b32_e64 %3, %3, %0, %4\n\tv_pk_fma_f32 %5, s[100:101], %8, %5 op_sel_hi:[0,1,1]"
                   : "=&v"(cand), "=&v"(dl), "=&s"(s0), "+v"(lam), "=&s"(m), "+v"(zz) : "v"(z), "v"(lo), "v"(col), "n"(G) : "scc", "s100", "s101");
}
// A row with symmetric bounds and no follower rows (the pipe motor rows)
PIH_HD void gs_row2_bounded(pk2& zz, real z, pk2 col, real hi, real& lam, int G, real& dl) {      // bounds -hi .. hi
  real cand; unsigned long long m;
  __asm__ volatile("v_med3_f32 %0, %5, -%6, %6\n\tv_sub_f32 %1, %0, %2\n\ts_lshl_b64 %3, 1, %8\n\tv_readlane_b32 s100, %1, %8\n\t"
                   "v_cndmask_b32_e64 %2, %2, %0, %3\n\ts_nop 0\n\tv_pk_fma_f32 %4, s[100:101], %7, %4 op_sel_hi:[0,1,1]"
                   : "=&v"(cand), "=&v"(dl), "+v"(lam), "=&s"(m), "+v"(zz) : "v"(z), "v"(hi), "v"(col), "n"(G) : "scc", "s100", "s101");
}
// Friction row: bounds -h .. h.  (One block per row, not per pair as in pgs_rows: the second row would have to read the half of zz
// the first one has just written, and an asm operand cannot name a half of a 64-bit operand -- a separate input operand is by
// contract the value at entry.  The s_waitcnt for the row's streamed column sits between two blocks anyway.)
PIH_HD void gs_row2_friction(pk2& zz, real z, pk2 col, real h, real& lam, int G, real& dl) {
  real cand; unsigned long long m;
  __asm__ volatile("v_med3_f32 %0, %5, -%6, %6\n\tv_sub_f32 %1, %0, %2\n\ts_lshl_b64 %3, 1, %8\n\tv_readlane_b32 s100, %1, %8\n\t"
                   "v_cndmask_b32_e64 %2, %2, %0, %3\n\ts_nop 0\n\tv_pk_fma_f32 %4, s[100:101], %7, %4 op_sel_hi:[0,1,1]"
                   : "=&v"(cand), "=&v"(dl), "+v"(lam), "=&s"(m), "+v"(zz) : "v"(z), "v"(h), "v"(col), "n"(G) : "scc", "s100", "s101");
}
// The same for the one-row-per-lane solver (pgs_rows): z += b * sdl with v_fmac_f32, the broadcast in any SGPR; the two friction rows
// of a contact (Bullet runs both or neither) are one block, so that nothing is inserted between them.
PIH_HD void gs_row1_normal(real& z, real b, real lo, real& lam, int G, real& dl, real& s0) {
  real cand, sdl; unsigned long long m;
  __asm__ volatile("v_max_f32 %0, %6, %7\n\tv_sub_f32 %1, %0, %4\n\tv_readlane_b32 %3, %0, %9\n\tv_readlane_b32 %2, %1, %9\n\t"
                   "s_lshl_b64 %5, 1, %9\n\tv_cndmask_b32_e64 %4, %4, %0, %5\n\tv_fmac_f32 %6, %2, %8"
                   : "=&v"(cand), "=&v"(dl), "=&s"(sdl), "=&s"(s0), "+v"(lam), "=&s"(m), "+v"(z) : "v"(lo), "v"(b), "n"(G) : "scc");
}
PIH_HD void gs_row1_friction2(real& z, real b1, real b2, real h, real& lam, int G1, int G2, real& dl1, real& dl2) {
  real cand, sdl; unsigned long long m;
  __asm__ volatile("v_med3_f32 %0, %6, -%7, %7\n\tv_sub_f32 %1, %0, %4\n\ts_lshl_b64 %5, 1, %10\n\tv_readlane_b32 %3, %1, %10\n\t"
                   "v_cndmask_b32_e64 %4, %4, %0, %5\n\ts_nop 0\n\tv_fmac_f32 %6, %3, %8\n\t"
                   "v_med3_f32 %0, %6, -%7, %7\n\tv_sub_f32 %2, %0, %4\n\ts_lshl_b64 %5, 1, %11\n\tv_readlane_b32 %3, %2, %11\n\t"
                   "v_cndmask_b32_e64 %4, %4, %0, %5\n\ts_nop 0\n\tv_fmac_f32 %6, %3, %9"
                   : "=&v"(cand), "=&v"(dl1), "=&v"(dl2), "=&s"(sdl), "+v"(lam), "=&s"(m), "+v"(z) : "v"(h), "v"(b1), "v"(b2), "n"(G1), "n"(G2) : "scc");
}
template <int CTRL> PIH_HD real dpp_add(real x) {   // x + x[dpp-permuted lane]  (v_add_f32_dpp)
  return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
PIH_HD real sum8(real x) {               // sum over each aligned group of 8 lanes, result in all 8
  x = dpp_add<0xB1>(x);                  // quad_perm [1,0,3,2]
  x = dpp_add<0x4E>(x);                  // quad_perm [2,3,0,1]
  return dpp_add<0x141>(x);              // row_half_mirror
}
PIH_HD real from_lane(real v, int byte_addr) {   // v of lane byte_addr / 4 (per-lane source): ds_bpermute_b32, no LDS memory, no VALU slot
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(byte_addr, __builtin_bit_cast(int, v)));
}
// ------------------------------------------------------------------------------------------------ forward kinematics
// GPU form: lane = link.  The world pose of a link is the product of the local transforms along its chain, i.e. an inclusive
// prefix "product" of rigid transforms: five Hillis-Steele steps (12 ds_bpermute + 39 FMA each) instead of a 33-link serial
// composition, and the pose never leaves the lane's registers before the world axes / rotated inertias are written.
// Out-of-chain sources read lane 63, which holds the identity.  Finger 8 is a child of link 6, not of finger 7: it takes
// finger 7's position in the chain order.  The arm's base rotation is folded into link 0's local transform.
PIH_HD int lane_byte(int lane) { return 4 * lane; }
PIH_HD void fk_all(Wave& w, Shared& sh) {
  w.sync();
  const int lane = w.lane();
  const bool active = lane < NL;
  const int L = active ? lane : NL - 1;
  M3 R = ldm(IDENT3); V3 o = mk(0, 0, 0);
  if (active) {
    real T[12];
    const real q = L < ANL ? sh.S[PIH_S_QARM + L] : (L == ANL ? (real)0 : sh.S[PIH_S_QJ + L - ANL - 1]);
    local_transform(L, q, sh.S, T);
    R = ldm(T); o = ld3(T + 9);
    if (L == 0) { const M3 B = ldm(ARM_BASE_R); o = mul(B, o); R = mul(B, R); }
  }
  const int cs = L < ANL ? 0 : ANL;
  const int vidx = L == ANL - 1 ? ANL - 2 : lane;
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) {
    const int src = vidx - off;
    const int sb = lane_byte((active && src >= cs) ? src : 63);
    M3 Rs; V3 os;
#pragma unroll
    for (int k = 0; k < 9; k++) Rs.m[k] = from_lane(R.m[k], sb);
    os = mk(from_lane(o.x, sb), from_lane(o.y, sb), from_lane(o.z, sb));
    o = os + mul(Rs, o); R = mul(Rs, R);
  }
  if (active) {
    stm(sh.a.LR[L], R); st3(sh.LO[L], o);
    st3(sh.LA[L], mul(R, ld3(L_AXIS[L])));
    st3(sh.a.LRC[L], mul(R, ld3(L_COM[L])));
    sts3(sh.a.LIC[L], rot_sym(R, lds3(L_INERTIA[L])));
  }
  w.sync();
}
// ------------------------------------------------------------------------------------------------ link velocities
// link velocities from the generalized velocity sh.u: omega_L and the velocity of the link-origin point
// The same recurrences as two inclusive prefix sums along the chains (lane = link): omega_L = sum over the path of the joint
// angular rates, v_L = sum over the path of (omega_parent x (o_L - o_parent) + prismatic rate).  Hillis-Steele steps through
// ds_bpermute (5 steps cover the 24-link pipe); finger 8 is a child of link 6, not of finger 7, so it drops finger 7's terms.
PIH_HD V3 from_lane3(V3 v, int byte_addr) { return mk(from_lane(v.x, byte_addr), from_lane(v.y, byte_addr), from_lane(v.z, byte_addr)); }
PIH_HD V3 chain_prefix_sum(V3 t, int lane, int chain_start) {
  V3 acc = t;
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) {
    const int src = lane - off;
    const V3 o = from_lane3(acc, 4 * (src < 0 ? 0 : src));
    if (src >= chain_start) acc = acc + o;
  }
  return acc;
}
PIH_HD void link_velocities_scan(Shared& sh, int lane) {
  const bool active = lane < NL;
  const int L = active ? lane : NL - 1;
  const int jt = L == ANL ? PIH_JT_FLOATING : ((L == ANL - 1 || L == ANL - 2) ? PIH_JT_PRISMATIC : PIH_JT_REVOLUTE);
  const int par = (L == 0 || L == ANL) ? -1 : (L == ANL - 1 ? ANL - 3 : L - 1);
  const int cs = L < ANL ? 0 : ANL, d = link_dof(L);
  const V3 aq = sh.u[d] * ld3(sh.LA[L]);
  const V3 tw = jt == PIH_JT_FLOATING ? ld3(&sh.u[d + 3]) : (jt == PIH_JT_REVOLUTE ? aq : mk(0, 0, 0));
  V3 wv = chain_prefix_sum(tw, lane, cs);
  const V3 tw7 = from_lane3(tw, 4 * (ANL - 2));
  if (L == ANL - 1) wv = wv - tw7;
  const V3 wp = from_lane3(wv, 4 * (par < 0 ? 0 : par));
  V3 tv;
  if (jt == PIH_JT_FLOATING) tv = ld3(&sh.u[d]);
  else {
    tv = jt == PIH_JT_PRISMATIC ? aq : mk(0, 0, 0);
    if (par >= 0) tv = tv + cross(wp, ld3(sh.LO[L]) - ld3(sh.LO[par]));
  }
  V3 vv = chain_prefix_sum(tv, lane, cs);
  const V3 tv7 = from_lane3(tv, 4 * (ANL - 2));
  if (L == ANL - 1) vv = vv - tv7;
  if (active) { st3(sh.VW[L], wv); st3(sh.VV[L], vv); }
}
PIH_HD void link_velocities(Wave& w, Shared& sh) { w.sync(); link_velocities_scan(sh, w.lane()); w.sync(); }

// ------------------------------------------------------------------------------------------------ collision detection
// GPU form of collide<W> (pih_common.h; the host harness keeps the template): the same tests (sphere_vs_table, sample_vs_tube, ...), the
// same contacts in the same slots, in three parts instead of nine passes that each fetched their table entries and sample positions anew.
//   1. Model constants once: lane l holds link, y and vertex flag of its two samples l and l + 64 (lanes >= 59: one), lanes 0..8 those of
//      their arm sphere -- one batch of independent loads, one wait.  Tables read at compile-time indices (sphere radii in the unrolled
//      loop, pad boxes, the hole) and the friction of a link picked at run time (link_mu) come from constexpr copies of the pih_model.h
//      macros: immediates, and a select where a dependent load L_MU[ANL + SAMP_LINK[i]] stood in front of every emit.
//   2. One walk: the lane computes its samples' positions (stored to LDS for the pair pass; its own consumers start from the pinned
//      register, a rounded value as the one read back would be) and, per sample, the table, tube, pad 0, pad 1 and arm-sphere
//      candidates into registers.  The five tests share nothing but the position, so their chains overlap.
//   3. Slots afterwards, in the order of the template -- ORDER CONTRACT: pass-major, chunk-minor: table, tube, attach ball, weld, arm
//      spheres vs table, pad 0, pad 1, arm spheres vs pipe, then the 253 pairs in key order (one list of the pairs in reach).  Every capped pass takes
//      allowed = CAMAX - nca at its start, emits under slot < CMAX and slot - before < allowed, and on overflow puts the counter back to
//      before + allowed; nca counts `used` whether or not the slots lie below CMAX.  Every w.alloc (a ballot) is reached by all 64
//      lanes; a lane whose sample index is >= NSAMP never holds a candidate.
constexpr double K_LMU[NL] = PIH_LINK_MU;
constexpr int K_ASPH_LINK[PIH_ARM_NSPH] = PIH_ARM_SPH_LINK;
constexpr double K_ASPH_R[PIH_ARM_NSPH] = PIH_ARM_SPH_R;
constexpr double K_FBOX_C[2][3] = PIH_FINGER_BOX_C;
constexpr double K_FBOX_H[3] = PIH_FINGER_BOX_H;
constexpr double K_HOLE_POS[3] = PIH_HOLE_POS;
// L_MU[L0 + k], k = 0 .. N - 1 picked at run time: the value most links share, and one select per link that differs
template <int L0, int N> PIH_HD real link_mu(int k) {
  real mu = (real)K_LMU[L0 + N / 2];
#pragma unroll
  for (int j = 0; j < N; j++) if (K_LMU[L0 + j] != K_LMU[L0 + N / 2]) mu = k == j ? (real)K_LMU[L0 + j] : mu;
  return mu;
}
PIH_HD real pipe_link_mu(int s) { return link_mu<ANL, ONL>(s); }                  // L_MU[ANL + s]
PIH_HD void arm_sphere_link(int s, int& link, real& mu) {                          // ASPH_LINK[s], L_MU[ASPH_LINK[s]]
  link = K_ASPH_LINK[0]; mu = (real)K_LMU[K_ASPH_LINK[0]];
#pragma unroll
  for (int j = 1; j < PIH_ARM_NSPH; j++) { link = s == j ? K_ASPH_LINK[j] : link; mu = s == j ? (real)K_LMU[K_ASPH_LINK[j]] : mu; }
}
PIH_HD void pin(V3& v) { __asm__ volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z)); }
// Where -ffast-math associates a sum differently once its terms are constants or sit in another block, the contact's last bits move
// (tests/test_gpu_collision_bits.py).  Two places did, and are written in the association of the nine-pass form:
//   - arm sphere vs table: depth = c.z + (-TABLE_Z - rs), p.z = c.z - (rs + 0.5 depth), each bracket rounded on its own;
//   - arm spheres vs pipe: the radii are held as opaque scalar values (arm_sphere_radius), so that reach = (margin + r) + R and
//     dep = dist + (-r - R) are formed as with the radii loaded from the table.
PIH_HD Cand arm_sphere_vs_table(V3 c, real rs, real margin) {
  Cand o;
  real k = -(real)PIH_TABLE_Z - rs; __asm__ volatile("" : "+v"(k));
  o.depth = c.z + k; o.valid = o.depth < margin;
  real t = rs + (real)0.5 * o.depth; __asm__ volatile("" : "+v"(t));
  o.p = mk(c.x, c.y, c.z - t); o.n = mk(0, 0, 1);
  return o;
}
PIH_HD real arm_sphere_radius(int s) { real v = (real)K_ASPH_R[s]; __asm__ volatile("" : "+s"(v)); return v; }
// pair_of_index for idx = lane + 64 k, k a constant after unrolling: row s starts at C(s) = s (45 - s) / 2, and only a few rows start
// inside a chunk of 64 (3, 3, 5, 10), so s is the rows that start at or before the chunk plus one compare per row that starts inside
// it: no square root, no corrections.  Lanes past the last pair (chunk 3, lanes 61 ..) get the last pair.
PIH_HD void pair_of_chunk_lane(int k, int lane, int& s, int& t) {
  const int lo = 64 * k, idx = k < 3 ? lo + lane : (lane < 253 - 192 ? lo + lane : 252);
  s = 0;
#pragma unroll
  for (int j = 1; j < 22; j++) {
    const int cj = j * (45 - j) / 2;
    if (cj <= lo) s++;
    else if (cj <= lo + 63) s += idx >= cj;
  }
  t = s + 2 + idx - s * (45 - s) / 2;
}
// vertex_sample without its two branches: 7 + 5 (v - 1) is NSAMP - 1 at v = 24 by itself, only vertex 0 is apart (the narrow rounds call
// it at four run-time indices per lane; as written in pih_common.h each call became two divergent blocks)
static_assert(7 + 5 * (24 - 1) == NSAMP - 1, "the last vertex is the last sample");
PIH_HD int vertex_sample_flat(int v) { return 5 * v + (v == 0 ? 0 : 2); }
constexpr int PAIR_REC_WORDS = 4 * 24;                     // the pair pass's per-segment records, then its survivor list, in sh.a.IAP
static_assert(PAIR_REC_WORDS + 253 <= NL * 28 && PAIR_REC_WORDS % 4 == 0, "records and list of the pair pass alias ArenaA::IAP");
PIH_HD void collide(Wave& w, Shared& sh, const Params& P) {
  const real r = (real)PIH_PIPE_RADIUS, margin = P.margin;
  const int lane = w.lane();
  w.stamp(16);
  // ---- 1. constants
  bool inr[2]; int sidx[2], slink[2], svert[2]; real sy[2];
#pragma unroll
  for (int c = 0; c < 2; c++) {
    sidx[c] = lane + 64 * c; inr[c] = sidx[c] < NSAMP;
    const int j = inr[c] ? sidx[c] : NSAMP - 1;
    slink[c] = SAMP_LINK[j]; sy[c] = SAMP_Y[j]; svert[c] = SAMP_VERTEX[j];
  }
  const bool isph = lane < PIH_ARM_NSPH;
  const int jsph = isph ? lane : 0;
  const int alink = ASPH_LINK[jsph]; const real arad = ASPH_R[jsph]; const V3 acen = ld3(ASPH_C[jsph]);
  // ---- 2. sample positions, arm sphere centres
  w.sync();
  V3 sp[2];
#pragma unroll
  for (int c = 0; c < 2; c++) {
    sp[c] = sample_point(sh, ANL + slink[c], sy[c]);
    if (inr[c]) st3(sh.a.SP[sidx[c]], sp[c]);
    pin(sp[c]);
  }
  // arm collision spheres (pih_model.h PIH_ARM_SPH_*, PROVISIONAL stand-ins for the Panda collision meshes of pybullet_data)
  V3 cw = mk(0, 0, 0);
  if (P.armcol) {
    cw = ld3(sh.LO[alink]) + mul(ldm(sh.a.LR[alink]), acen);
    if (isph) st3(sh.a.ASP[lane], cw);
    pin(cw);
  }
  w.sync();
  // ... the candidates of both samples
  const V3 hole = mk((real)K_HOLE_POS[0], (real)K_HOLE_POS[1], (real)K_HOLE_POS[2]);
  const V3 bh = mk((real)K_FBOX_H[0], (real)K_FBOX_H[1], (real)K_FBOX_H[2]);
  const real padreach = pad_reach(bh, r, margin);
  M3 Rf[2]; V3 bc[2];
#pragma unroll
  for (int f = 0; f < 2; f++) {
    Rf[f] = ldm(sh.a.LR[PIH_FINGER_LINK0 + f]);
    bc[f] = ld3(sh.LO[PIH_FINGER_LINK0 + f]) + mul(Rf[f], mk((real)K_FBOX_C[f][0], (real)K_FBOX_C[f][1], (real)K_FBOX_C[f][2]));
  }
  const bool armpipe = (P.armcol & 2) != 0;
  V3 ac[PIH_ARM_NSPH]; real ar[PIH_ARM_NSPH];
#pragma unroll
  for (int s = 0; s < PIH_ARM_NSPH; s++) { ac[s] = armpipe && s >= PIH_ARM_PIPE_SPH0 ? ld3(sh.a.ASP[s]) : mk(0, 0, 0); ar[s] = arm_sphere_radius(s); }
  Cand ct[2], ch[2], cp[2][2], ca[2]; int bs[2];
#pragma unroll
  for (int c = 0; c < 2; c++) {
    ct[c] = no_cand(); ch[c] = no_cand(); cp[0][c] = no_cand(); cp[1][c] = no_cand(); ca[c] = no_cand(); bs[c] = 0;
    if (inr[c] && svert[c]) ct[c] = sphere_vs_table(sp[c], r, margin);                       // table plane: vertices only
    if (inr[c]) ch[c] = sample_vs_tube(sp[c], hole, r, margin);
    if (inr[c]) cp[0][c] = sample_vs_pad(sp[c], Rf[0], bc[0], bh, padreach, r, margin);
    if (inr[c]) cp[1][c] = sample_vs_pad(sp[c], Rf[1], bc[1], bh, padreach, r, margin);
    if (armpipe && inr[c]) ca[c] = sample_vs_arm_spheres(sp[c], [&](int s) { return ac[s]; }, [&](int s) { return ar[s]; }, r, margin, bs[c]);
  }
  w.stamp(17);
  // ---- 3. slots
  w.alloc_reset(0);
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const int slot = w.alloc(ct[c].valid);
    if (ct[c].valid && slot < CMAX)
      emit_contact(sh, slot, ANL + slink[c], -1, vertex_key(slink[c], sy[c]), ct[c].p, ct[c].n, ct[c].depth, pipe_link_mu(slink[c]) * (real)PIH_TABLE_MU);
  }
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const int slot = w.alloc(ch[c].valid);
    if (ch[c].valid && slot < CMAX) emit_contact(sh, slot, ANL + slink[c], -1, 100 + sidx[c], ch[c].p, ch[c].n, ch[c].depth, pipe_link_mu(slink[c]) * (real)PIH_HOLE_MU);
  }
  // attach ball and weld (scripted mode, FSM states 4..6; mu = -1 / -2 marks their bilateral rows): in front of every capped pass, never dropped
  int nca = 0;
  {
    const bool attached = P.mode == 1 && sh.S[PIH_S_FSM] >= 4 && sh.S[PIH_S_FSM] <= 6;
    const int before = w.alloc_count();
    {
      const bool valid = lane == 0 && attached;
      const int slot = w.alloc(valid);
      if (valid && slot < CMAX) { int L; const Cand c = attach_ball_contact(sh, L); emit_contact(sh, slot, L, PIH_EE_PARENT, 2000, c.p, c.n, c.depth, (real)-1); }
    }
    {
      const bool valid = lane == 0 && attached && !P.attachball;
      const int slot = w.alloc(valid);
      if (valid && slot < CMAX) { int L; const Cand c = attach_weld_contact(sh, L); emit_contact(sh, slot, L, PIH_EE_PARENT, 2001, c.p, c.n, c.depth, (real)-2); }
    }
    nca += w.alloc_count() - before;
  }
  // arm spheres vs the table plane (enable_arm_collision bit 0; keys 3000+): they count against the arm-contact cap and come before the
  // finger contacts, so a finger-vs-pipe contact is what gets dropped first
  if (P.armcol & 1) {
    const int before = w.alloc_count();
    const int allowed = CAMAX - nca;
    Cand c = no_cand();
    if (isph) c = arm_sphere_vs_table(cw, arad, margin);
    const int slot = w.alloc(c.valid);
    if (c.valid && slot < CMAX && (slot - before) < allowed) {
      int L; real mu; arm_sphere_link(lane, L, mu);
      emit_contact(sh, slot, L, -1, 3000 + lane, c.p, c.n, c.depth, mu * (real)PIH_TABLE_MU);
    }
    int used = w.alloc_count() - before;
    if (used > allowed) { used = allowed; w.alloc_reset(before + allowed); }
    nca += used;
  }
  w.stamp(18);
  // finger pad boxes (arm links 7, 8): arm-involving contacts are capped, the dropped ones are the tail of the pass
#pragma unroll
  for (int f = 0; f < 2; f++) {
    const int LF = PIH_FINGER_LINK0 + f;
    const int before = w.alloc_count();
    const int allowed = CAMAX - nca;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const Cand& k = cp[f][c];
      const int slot = w.alloc(k.valid);
      if (k.valid && slot < CMAX && (slot - before) < allowed)
        emit_contact(sh, slot, ANL + slink[c], LF, 300 + f * NSAMP + sidx[c], k.p, k.n, k.depth, pipe_link_mu(slink[c]) * (real)K_LMU[LF]);
    }
    int used = w.alloc_count() - before;
    if (used > allowed) { used = allowed; w.alloc_reset(before + allowed); }
    nca += used;
  }
  w.stamp(19);
  // arm spheres vs the pipe (enable_arm_collision bit 1; keys 5000 + sphere * NSAMP + sample): last of the arm-involving contacts, the
  // first to be dropped at the cap
  if (armpipe) {
    const int before = w.alloc_count();
    const int allowed = CAMAX - nca;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int slot = w.alloc(ca[c].valid);
      if (ca[c].valid && slot < CMAX && (slot - before) < allowed) {
        int lb; real mub; arm_sphere_link(bs[c], lb, mub);
        emit_contact(sh, slot, ANL + slink[c], lb, 5000 + bs[c] * NSAMP + sidx[c], ca[c].p, ca[c].n, ca[c].depth, pipe_link_mu(slink[c]) * mub);
      }
    }
    int used = w.alloc_count() - before;
    if (used > allowed) { used = allowed; w.alloc_reset(before + allowed); }
    nca += used;
  }
  w.stamp(20);
  // pipe self collision: capsule segments s < t, non adjacent (253 pairs, enumerated in key order).  The template filters every pair by
  // itself (four vertices, two square roots per pair, chunk after chunk); in the benchmark's steady state 70 % of the envs have NO pair
  // in reach and the rest a handful, so here the filter runs from 24 per-segment records, branch-free for all four chunks at once, and
  // the closest-point code runs over ONE compacted list of the survivors, 64 at a time: no round without a survivor.
  //   - records (lanes 0 .. 23): m = p + q, len = |q - p| of the lane's segment, from the vertex samples stored above
  //   - broad phase: lane l holds the pairs l, l + 64, l + 128, l + 192; eight 16-byte record reads in one batch, four predicates
  //     (segments_in_reach: a filter that may round differently from the template's, see there)
  //   - list: four ballots; the prefix popcounts put every survivor at its position in pair-index order -- which is key order, so the
  //     slots handed out below are the template's (ORDER CONTRACT).  An entry is s * 32 + t.
  //   - narrow rounds: lane l takes entry j0 + l, segment_closest (the template's arithmetic), then w.alloc and emit_contact as ever:
  //     a pair emits under slot < CMAX, the counter counts on beyond CMAX.
  // Records and list live in the first 96 + 253 words of sh.a.IAP, which nothing reads or writes between the end of the last step and
  // aba()'s own-inertia pass (pih_step.h), after collide.  The ballots and w.alloc are reached by all 64 lanes: the round count is
  // wave-uniform.
  if (P.selfcol) {
    real4* const rec = reinterpret_cast<real4*>(&sh.a.IAP[0][0]);
    int* const list = reinterpret_cast<int*>(&sh.a.IAP[0][0] + PAIR_REC_WORDS);
    if (lane < 24) {
      const SegRec g = segment_record(ld3(sh.a.SP[vertex_sample(lane)]), ld3(sh.a.SP[vertex_sample(lane + 1)]));
      real4 o; o.x = g.m.x; o.y = g.m.y; o.z = g.m.z; o.w = g.len;
      rec[lane] = o;
    }
    int ps[4], pt[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pair_of_chunk_lane(k, lane, ps[k], pt[k]);
    w.sync();
    real4 rs[4], rt[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { rs[k] = rec[ps[k]]; rt[k] = rec[pt[k]]; }
    unsigned long long hit[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool in = segments_in_reach(mk(rs[k].x, rs[k].y, rs[k].z), rs[k].w, mk(rt[k].x, rt[k].y, rt[k].z), rt[k].w, r, margin);
      hit[k] = __ballot(k < 3 ? in : in & (lane < 253 - 192));                          // (no &&: the four predicates stay one block)
    }
    int nsurv = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if ((hit[k] >> lane) & 1) list[nsurv + __popcll(hit[k] & ((1ull << lane) - 1ull))] = ps[k] * 32 + pt[k];
      nsurv += __popcll(hit[k]);
    }
    w.sync();
    for (int j0 = 0; j0 < nsurv; j0 += 64) {
      const bool has = j0 + lane < nsurv;
      const int e = has ? list[j0 + lane] : 2;                 // (an idle lane reads the vertices of the pair (0, 2) and keeps no candidate)
      const int s = e >> 5, t = e & 31;
      auto vtx = [&](int v) -> V3 { return ld3(sh.a.SP[vertex_sample_flat(v)]); };
      Cand c = segment_closest(vtx(s), vtx(s + 1), vtx(t), vtx(t + 1), r, margin);
      c.valid = c.valid && has;
      const int slot = w.alloc(c.valid);
      if (c.valid && slot < CMAX) emit_contact(sh, slot, ANL + s, ANL + t, 1000 + s * 24 + t, c.p, c.n, c.depth, pipe_link_mu(s) * pipe_link_mu(t));
    }
  }
  w.stamp(21);
  int nc = w.alloc_count(); if (nc > CMAX) nc = CMAX;
  sh.nc = nc; sh.nca = nca;
  w.sync();
}

// ------------------------------------------------------------------------------------------------ ABA inward sweep
// Inward sweep of the articulated-body algorithm, LANE = ENTRY of the articulated inertia: lane l < 48 owns entry
// (i, j) = (l >> 3, l & 7) of the 6 x 8 array [ I^A (6 x 6, rows/cols 0-2 angular, 3-5 linear, i.e. [[A, B], [B^T, C]]) |
// p^A (column 6) | - ].  Per link:
//   1. m = own inertia of the link + what the child handed up
//   2. U = I^A S  (S = [a; 0] revolute, [0; a] prismatic), D = S.U, u = tau - S.p^A
//   3. I^a = I^A - U U^T / D ;  column 6 = p^a = p^A + I^a c + U u / D
//   4. translate to the parent's origin (r = o_L - o_parent):  B' = B + [r]x C,  A' = A + [r]x B^T - B' [r]x,
//      p_a' = p_a + r x p_l   (entry formulas: ([r]x X)_ij = r_i1 X_i2,j - r_i2 X_i1,j ; (X [r]x)_ij = X_i,j1 r_j2 - X_i,j2 r_j1)
// The arm's two fingers (links 7, 8) both feed link 6: finger 8's hand-up is parked in a register until finger 7 is done.
PIH_HD void aba_inward(Wave& w, Shared& sh, areal* rootp) {
  real* const Mx = sh.r_lam;      // 48 words of scratch for the root inversion (r_lam is dead until the rows are built)
  // GPU form of the same four steps: the entry stays in a register of its lane; row sums are DPP reductions over the 8-lane
  // row group, entries of other rows come through ds_bpermute (no LDS memory, no VALU slot), wave-uniform scalars (D, u, the
  // U vector) through v_readlane.  The translation is branch-free: every lane evaluates
  //     v + rA X1 - rB X2 - ( (X3 + rA X4 - rB X5) rG - (X6 + rA X7 - rB X8) rK )
  // with per-lane source lanes and 0/1 masks fixed before the loop (B, B^T and p_a lanes use the first two terms only,
  // C / p_l / idle lanes none), so one batch of 8 bpermutes and one wait serve the whole step.
  {
    const int l = w.lane(), i = l >> 3, j = l & 7;
    const int ia = i < 3 ? i : (i < 6 ? i - 3 : 0), ja = j < 3 ? j : (j < 6 ? j - 3 : 0);
    const int i1 = ia == 2 ? 0 : ia + 1, i2 = ia == 0 ? 2 : ia - 1, j1 = ja == 2 ? 0 : ja + 1, j2 = ja == 0 ? 2 : ja - 1;
    const bool typeA = i < 3 && j < 3, typeB = i < 3 && j >= 3 && j < 6, typeBt = i >= 3 && i < 6 && j < 3, typeP = i < 3 && j == 6;
    const int own_off = aba_own_word(i, j);
    // first pair of terms: coefficient indices into r and source lanes
    int kA = 0, kB = 0, s1 = l, s2 = l;
    if (typeA) { kA = i1; kB = i2; s1 = 8 * j + 3 + i2; s2 = 8 * j + 3 + i1; }
    else if (typeB) { kA = i1; kB = i2; s1 = 8 * (3 + i2) + j; s2 = 8 * (3 + i1) + j; }
    else if (typeBt) { kA = j1; kB = j2; s1 = 8 * (3 + j2) + i; s2 = 8 * (3 + j1) + i; }
    else if (typeP) { kA = i1; kB = i2; s1 = 8 * (3 + i2) + 6; s2 = 8 * (3 + i1) + 6; }
    const real m1 = (typeA || typeB || typeBt || typeP) ? (real)1 : (real)0, m2 = typeA ? (real)1 : (real)0;
    int s3 = l, s4 = l, s5 = l, s6 = l, s7 = l, s8 = l;
    if (typeA) { s3 = 8 * i + 3 + j1; s4 = 8 * (3 + i2) + 3 + j1; s5 = 8 * (3 + i1) + 3 + j1; s6 = 8 * i + 3 + j2; s7 = 8 * (3 + i2) + 3 + j2; s8 = 8 * (3 + i1) + 3 + j2; }
    const int sUj = j < 6 ? 8 * j : l;                                 // any lane of row j holds U_j
    // one link with a joint (steps 2-4): stores U, 1/D, u; returns the lane's entry of what is handed up to the parent (garbage for
    // the arm root, whose parent is the fixed world: `up` = false skips the translation)
    auto link = [&](int L, real m, bool up) __attribute__((always_inline)) -> real {
      const int jt = joint_type(L);                                    // (no table load on the chain: pih_common.h)
      const int sb = jt == PIH_JT_REVOLUTE ? 0 : 3;
      const V3 a = ld3(sh.LA[L]);
      const real rA = m1 * sh.AR[L][kA], rB = m1 * sh.AR[L][kB], rG = m2 * sh.AR[L][j2], rK = m2 * sh.AR[L][j1];
      const real cj = j < 6 ? sh.a.CB[L][j] : (real)0;
      const int js = j - sb;
      const real sj = js == 0 ? a.x : (js == 1 ? a.y : (js == 2 ? a.z : (real)0));
      const real Ui = sum8(m * sj);                                    // U_i = sum_k I^A[i][sb + k] a_k, in every lane of row i
      const real Uj = from_lane(Ui, 4 * sUj);
      const real D = a.x * rdlane(Ui, 8 * sb) + a.y * rdlane(Ui, 8 * (sb + 1)) + a.z * rdlane(Ui, 8 * (sb + 2));
      const real tau = 0;                                               // (-L_DAMPING[L] * u: no joint damping in the model, asserted in pih_common.h)
      const real u = tau - (a.x * rdlane(m, 8 * sb + 6) + a.y * rdlane(m, 8 * (sb + 1) + 6) + a.z * rdlane(m, 8 * (sb + 2) + 6));
      const real Di = (real)1 / D;
      if (j == 0 && i < 6) sh.AU[L][i] = Ui;
      if (l == 0) { sh.ADinv[L] = Di; sh.Au[L] = u; }
      if (!up) return 0;
      real ma = j < 6 ? m - Ui * Uj * Di : m;                          // I^a ; column 6 is fixed up next
      const real s = sum8(j < 6 ? ma * cj : (real)0);                  // (I^a c)_i in every lane of row i
      if (j == 6) ma = m + s + Ui * (u * Di);                          // p^a = p^A + I^a c + U u / D
      const real X1 = from_lane(ma, 4 * s1), X2 = from_lane(ma, 4 * s2), X3 = from_lane(ma, 4 * s3), X4 = from_lane(ma, 4 * s4),
                 X5 = from_lane(ma, 4 * s5), X6 = from_lane(ma, 4 * s6), X7 = from_lane(ma, 4 * s7), X8 = from_lane(ma, 4 * s8);
      return ma + rA * X1 - rB * X2 - ((X3 + rA * X4 - rB * X5) * rG - (X6 + rA * X7 - rB * X8) * rK);
    };
    // The arm chain (links 8 .. 0) and the pipe chain (33 .. 9) are independent: the first eight steps take one link of each in
    // the same basic block, so that the two dependent chains (LDS read -> DPP sums -> bpermute -> rcp -> DPP sums -> 8 bpermutes)
    // fill each other's latencies; the remaining sixteen pipe links, the floating pipe root and the arm root follow.
    real carry_p = 0, carry_a = 0, hold = 0;
#pragma nounroll
    for (int k = 0; k < 8; k++) {
      const int Lp = NL - 1 - k, La = ANL - 1 - k;                     // pipe 33 .. 26, arm 8 .. 1
      const real own_p = sh.a.IAP[Lp][own_off], own_a = sh.a.IAP[La][own_off];
      const real mp = k == 0 ? own_p : own_p + carry_p;                // link 33 is the pipe's leaf
      const real ma = k < 2 ? own_a : own_a + carry_a;                 // links 8 and 7 (the fingers) are leaves
      const real vp = link(Lp, mp, true), va = link(La, ma, true);
      carry_p = vp;
      if (k == 0) hold = va;                                           // finger 8: parked until finger 7 is done
      else if (k == 1) carry_a = va + hold;                            // finger 7: both fingers feed link 6
      else carry_a = va;
    }
#pragma nounroll
    for (int L = NL - 9; L > ANL; L--) carry_p = link(L, sh.a.IAP[L][own_off] + carry_p, true);
    {                                                                  // floating pipe root
      const real m = sh.a.IAP[ANL][own_off] + carry_p;
      w.sync(); if (l < 48) Mx[l] = m; w.sync();
      aba_root_inverse(sh, Mx, rootp);
    }
    link(0, sh.a.IAP[0][own_off] + carry_a, false);                    // arm root: parent is the fixed world
    w.sync();
  }
}

// ------------------------------------------------------------------------------------------------ motor response rows
// pull the 32 motor response rows out of their LDS staging words into registers (lane = DOF: arm lanes hold column d of the
// 9 x 9 arm block, pipe lanes column d - 9 of the 23 x 29 pipe block) before the contact rows of the second pass overwrite them
PIH_HD void pull_motor_rows(Wave& w, Shared& sh, MotorW& mw) {
  const int d = w.lane();
#pragma unroll
  for (int j = 0; j < PIH_OBJ_NJ; j++) mw.w[j] = d < 9 ? (j < 9 ? wma_row(sh, j)[d] : (real)0) : (d < ND ? wmp_row(sh, j)[d - 9] : (real)0);
}

// ------------------------------------------------------------------------------------------------ PGS
// after row16_sum3: rows 1,3 += lane 15 of the previous row (row_bcast:15), rows 2,3 += lane 31 (row_bcast:31)
// => lanes 32..47 hold the sum over lanes 0..47 (all 38 DOF lanes).  Written as inline asm because hipcc lowers the
// masked-row form to v_mov 0 + v_mov_dpp + v_add (3 instructions) instead of one fused v_add_f32_dpp; the s_nop covers the
// VALU-write -> DPP-read hazard that the compiler does not pad inside asm.
PIH_HD void rows012_total3(real& a, real& b, real& c) {
  __asm__ volatile("s_nop 1\n\t"
                   "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa\n\t"
                   "v_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa\n\t"
                   "v_add_f32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa\n\t"
                   "s_nop 1\n\t"
                   "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc\n\t"
                   "v_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc\n\t"
                   "v_add_f32_dpp %2, %2, %2 row_bcast:31 row_mask:0xc\n\t"
                   "s_nop 1"
                   : "+v"(a), "+v"(b), "+v"(c));
}
// after this every lane holds the sum over its 16-lane row; three independent reductions interleaved for ILP
PIH_HD void row16_sum3(real& a, real& b, real& c) {
  a = dpp_add<0xB1>(a); b = dpp_add<0xB1>(b); c = dpp_add<0xB1>(c);        // quad_perm [1,0,3,2]
  a = dpp_add<0x4E>(a); b = dpp_add<0x4E>(b); c = dpp_add<0x4E>(c);        // quad_perm [2,3,0,1]
  a = dpp_add<0x141>(a); b = dpp_add<0x141>(b); c = dpp_add<0x141>(c);     // row_half_mirror
  a = dpp_add<0x140>(a); b = dpp_add<0x140>(b); c = dpp_add<0x140>(c);     // row_mirror
}


// ---- PGS in ROW space for envs with few contacts (the common case: 70-80 % of the env-steps of the benchmark workload)
// When all rows fit one wavefront -- 32 motor rows + 3 x (<= MERGED_CONTACTS) contact rows <= 62 -- lane g owns row g and holds
//   z = lambda + rhs - dinv (J_g . du)   "the multiplier the row would take if it were not clamped", given every impulse applied so
//                                        far (the arm joints' lanes, whose three rows share one lane, hold -dinv (J_g . du)), and
//   Bn[i] = [g == i] - dinv A[g][i]      from the lane's row of the Delassus matrix A = J M^-1 J^T, for EVERY row i (62 registers;
//                                        motor columns by symmetry from the lane's own response row, contact columns as J_g . W_i
//                                        against the response rows that build_rows staged in LDS).
// A row update then needs no Jacobian and no cross-lane reduction: every lane clamps its own z (v_med3), subtracts its multiplier,
// the row's lane supplies the step through one v_readlane, and ONE FMA moves every z (z += Bn[i] * step; the updated row's own z
// stays put because dinv A[i][i] = 1) -- with the same sequence of row updates as Bullet (per arm joint: motor, lower, upper
// limit; the 23 pipe motors; per contact: normal, dir1, dir2).  The DOF velocities are recovered at the end as du = sum_i W_i
// lambda_i.  The arm-row and pipe-row columns are disjoint (A[arm][pipe motor] = 0), so the motor chain runs on two accumulators
// for ILP exactly like the DOF-space chain.  (tools/micro/rowchain.hip times the row chain in isolation.)
// (The iteration loop of all three solvers and the cadence of the exit test: pgs_iteration_loop, pih_common.h.)
// Word W (a CR_* / MR_* / LR_* name, pih_common.h) of a record held in registers as 16-byte groups: component W % 4 of group W / 4,
// picked at compile time; rec4v: words W .. W + 2 as a vector
template <int W> PIH_HD real rec4(const real4* q) { constexpr int c = W % 4; return c == 0 ? q[W / 4].x : c == 1 ? q[W / 4].y : c == 2 ? q[W / 4].z : q[W / 4].w; }
template <int W> PIH_HD V3 rec4v(const real4* q) { return mk(rec4<W>(q), rec4<W + 1>(q), rec4<W + 2>(q)); }
// One arm joint block of the row-space solvers (pgs_rows, pgs_rows2): the motor row, then -- LIMITS -- the lower and the upper limit row,
// in Bullet's order.  ca / cl: the joint's motor and limit record (MR_* / LR_*), y = dinv (J du) of the joint; la / llo / lhi: its three
// wave-uniform multipliers.  Returns the motor row's step, d2 / d3 the limit rows' (0 without LIMITS); CHECK: the rows' exit test into busy.
template <bool CHECK, bool LIMITS> PIH_HD real arm_joint_rows(const real4& ca, const real4& cl, real y, real& la, real& llo, real& lhi,
                                                              unsigned long long& busy, real& d2, real& d3) {
  const real rh = rec4<MR_RHS>(&ca), th = rec4<MR_THRESH>(&ca), lim = rec4<MR_IMP>(&ca);
  const real lor = rec4<LR_LO>(&cl), hir = rec4<LR_HI>(&cl), wd = rec4<LR_JWDINV>(&cl);
  real sum = la + (rh - y);
  sum = med3_(sum, -lim, lim);
  const real dl = sum - la; la = sum;
  if (CHECK) busy |= __ballot(absr(dl) > th);
  d2 = 0; d3 = 0;
  if (LIMITS) {
    y += dl * wd;
    real s2 = llo + (lor - y); s2 = max_(s2, (real)0);
    d2 = s2 - llo; llo = s2;
    if (CHECK) busy |= __ballot(absr(d2) > th);
    y += d2 * wd;
    real s3 = lhi + (hir + y); s3 = max_(s3, (real)0);
    d3 = s3 - lhi; lhi = s3;
    if (CHECK) busy |= __ballot(absr(d3) > th);
  }
  return dl;
}
constexpr int FR = NMOT + 3 * MERGED_CONTACTS;
PIH_HD int pgs_rows(Wave& w, Shared& sh, const Params& P) {
  const int nc = __builtin_amdgcn_readfirstlane(sh.nc);
  w.sync();
  const int lane = w.lane();
  const bool hasarm = __builtin_amdgcn_readfirstlane(sh.nca) != 0;       // does any contact involve an arm link?
  // ---- this lane's Jacobian row (38 entries, registers): unit vector for a motor row, point Jacobian for a contact row
  real J[ND];
  {
    const bool ismotor = lane < NMOT;
    const int row = ismotor ? 0 : lane - NMOT, c = row / 3, k = row - 3 * c;
    const bool live = !ismotor && c < nc;
    int la = -1, lb = -1; V3 p = mk(0, 0, 0), dir = mk(0, 0, 0); bool ang = false;
    if (live) { la = sh.c_la[c]; lb = sh.c_lb[c]; const real* R = sh.b.crec[c]; p = ld3(R + CR_P); dir = ld3(R + CR_DIR0 + CR_KSTRIDE * k); ang = R[CR_ANG] != 0; }
    const int md = lane < 9 ? lane : 15 + (lane - 9);
    // No contact involves the arm in 99.9 % of the env-steps of a random-action rollout (sh.nca, counted by collide): the nine arm
    // entries of every contact row's Jacobian and response row are then exact zeros, and both the entries and their products are
    // left out (wave-uniform branches; the sums are unchanged, a skipped term is 0 x 0)
    if (!hasarm) {
#pragma unroll
      for (int d = 0; d < 9; d++) J[d] = ismotor && d == md ? (real)1 : (real)0;
    }
    DofGeom gn = dof_geom(sh, hasarm ? 0 : 9);
#pragma unroll
    for (int d = 0; d < ND; d++) {
      if (d < 9 && !hasarm) continue;
      const DofGeom g = gn;
      if (d + 1 < ND) gn = dof_geom(sh, d + 1);           // the next DOF's axis / origin are in flight while this entry is computed
      const real jc = live ? jac_entry(g, la, lb, p, dir, ang) : (real)0;
      J[d] = ismotor ? (d == md ? (real)1 : (real)0) : jc;
      __asm__ volatile("" : "+v"(J[d]) :: "memory");     // one DOF at a time (same reason as for the columns of A below)
    }
  }
  // ---- this lane's row of A.  Motor columns need no dot product: the Delassus matrix is symmetric, A[r][motor m] = (M^-1 J_r^T)[dof(m)]
  // = W_r[dof(m)] -- a contact row reads entry dof(m) of its OWN response row, a motor row the entry of motor m's staged row at its
  // own DOF (arm x pipe entries are 0): 32 LDS reads per lane instead of 748 FMAs + 748 broadcasts
  real A[FR];
  {
    const int row = lane - NMOT;                                         // contact-row index (lanes >= 32)
    const bool crow = row >= 0 && row < 3 * nc;
    const real* wown = crow ? sh.b.Wp[row] : sh.b.Wp[0];
#pragma unroll
    for (int m = 0; m < NMOT; m++) {
      const int dm = m < 9 ? m : 15 + (m - 9);                            // the motor's DOF
      real a = 0;
      if (crow) a = wown[dm];
      else if (m < 9) { if (lane < 9) a = wma_row(sh, m)[lane]; }
      else if (lane >= 9 && lane < NMOT) a = wmp_row(sh, m - 9)[lane - 3];   // DOF of pipe motor lane: 15 + (lane - 9); row entries start at DOF 9
      if (m % 4 == 3) __asm__ volatile("" : "+v"(a) :: "memory");          // four LDS reads in flight, not one (and not all 32: spills)
      A[m] = a;
    }
  }
#pragma unroll
  for (int c = 0; c < MERGED_CONTACTS; c++) {
    if (c < nc) {
      // (the three response rows of a contact are requested together: one LDS round trip per contact instead of one per column)
      real a0 = 0, a1 = 0, a2 = 0;
      const real* wr = sh.b.Wp[3 * c];
      if (hasarm) {
#pragma unroll
        for (int d = 0; d < 9; d++) { a0 += J[d] * wr[d]; a1 += J[d] * wr[WPS + d]; a2 += J[d] * wr[2 * WPS + d]; }
      }
#pragma unroll
      for (int d = 9; d < ND; d++) { a0 += J[d] * wr[d]; a1 += J[d] * wr[WPS + d]; a2 += J[d] * wr[2 * WPS + d]; }
      __asm__ volatile("" : "+v"(a0), "+v"(a1), "+v"(a2) :: "memory");
      A[NMOT + 3 * c] = a0; A[NMOT + 3 * c + 1] = a1; A[NMOT + 3 * c + 2] = a2;
    } else { A[NMOT + 3 * c] = 0; A[NMOT + 3 * c + 1] = 0; A[NMOT + 3 * c + 2] = 0; }
  }
  // ---- per-lane row constants.  The solve runs on z = lambda + rhs - dinv (J du) of the lane's own row ("the multiplier the row
  // would take if it were not clamped"): a row update is then  lambda' = clamp(z),  d = lambda' - lambda,  and every lane's z moves
  // by  -dinv A[i] d  -- except the updated row's own z, which stays where it is (dinv A[i][i] = 1).  With Bn[i] = [lane == i] -
  // dinv A[i] (in the registers that held A) the whole update of row i is
  //     clamp (v_med3) -> subtract -> v_readlane -> one FMA on z
  // three dependent VALU operations and a readlane instead of readlane -> FMA -> clamp -> subtract -> FMA, no row constant is
  // fetched inside the loop (bounds, threshold and multiplier of a row live in its lane), and the running multipliers of the pipe
  // motors and the contacts need no wave-uniform registers.  The arm joints keep their uniform chain (motor, lower, upper limit
  // share one lane): their lanes hold z = -dinv (J du).
  w.sync();
  real di = 0, rhs = 0, thr = PIH_BIG, lbv = 0, ubv = 0, cmu = 0, cfl = 0, lam0 = 0, rhsa = 0;
  // (thr / rhsa of lanes 0..6: read by the residual form of the arm motor rows only; the clamped arm blocks take both from the record)
  if (lane < 9) { di = sh.mrec[lane][MR_DINV]; if (lane < 7) { thr = sh.mrec[lane][MR_THRESH]; rhsa = sh.mrec[lane][MR_RHS]; } }
  else if (lane < NMOT) { di = sh.mrec[lane][MR_DINV]; rhs = sh.mrec[lane][MR_RHS]; thr = sh.mrec[lane][MR_THRESH]; ubv = sh.mrec[lane][MR_IMP]; lbv = -ubv; }
  else {
    const int row = lane - NMOT, c = row / 3, k = row - 3 * c;
    if (c < nc) {
      const real* R = sh.b.crec[c];
      di = R[CR_DINV0 + CR_KSTRIDE * k]; rhs = R[CR_RHS + k]; thr = R[CR_THRESH + k]; cmu = R[CR_MU]; cfl = R[CR_FLOOR];
      if (k == 0) { lbv = R[CR_LB]; ubv = PIH_BIG; lam0 = sh.r_lam[3 * c]; }      // friction rows: bounds set per iteration from the normal multiplier
    }
  }
  // (sqrt(resid) * dinv of a contact row sits in words CR_THRESH.. of its record, the multipliers go back to sh.r_lam)
#pragma unroll
  for (int i = 0; i < FR; i++) { A[i] = (lane == i && lane >= 9 ? (real)1 : (real)0) - di * A[i]; }
  real* const Bn = A;
  unsigned angmask = 0;                    // contacts whose friction rows are always solved (mu < 0: the attach weld's rows)
#pragma unroll
  for (int c = 0; c < MERGED_CONTACTS; c++) if (c < nc && sh.b.crec[c][CR_MU] < 0) angmask |= 1u << c;
  angmask = (unsigned)__builtin_amdgcn_readfirstlane((int)angmask);
  // ---- the limit rows of arm joints 0..6 are exact no-ops for the whole solve when (a) the joint's motor row is never clamped --
  // an unclamped velocity motor sets the joint's velocity change to (target - current) whatever it was, because J W dinv = 1 -- and
  // (b) that target velocity violates neither limit speed: then  rhs_limit - (J du) dinv = (v_limit - v_target) dinv < 0  every time
  // and the multiplier stays 0.  (b) is known before the solve (skip7, wave-uniform); (a) is watched during the solve (one compare
  // per arm motor row) and, should a motor ever clamp, the solve is simply run again with every limit row in place.  The finger
  // joints (targets far outside [0, 0.04] most of the time) always keep their limit rows.
  bool skip7 = true;
  {
    const real dt = P.dt;
#pragma unroll
    for (int j = 0; j < 7; j++) {
      const real q = sh.S[PIH_S_QARM + j], uj = sh.u[j];
      const real vt = sh.mrec[j][MR_RHS] * sh.lrec[j][LR_JW] + uj;                         // rhs / dinv + u = the motor's target velocity
      const real plo = q - L_LO[j], phi = L_HI[j] - q;
      const real vlo = plo > 0 ? -plo / dt : -P.erp * plo / dt, vhi = phi > 0 ? -phi / dt : -P.erp * phi / dt;
      const real tol = (real)1e-4 * ((real)1 + absr(vt) + absr(uj) + absr(vlo) + absr(vhi));
      skip7 = skip7 && (vt - vlo > tol) && (-vhi - vt > tol);
    }
    // only with the huge impulse bound of the action-mode controller (1e5 dt): the scripted controller's 1200 dt does clamp
    skip7 = skip7 && sh.mrec[0][MR_IMP] >= (real)100;
    skip7 = __builtin_amdgcn_readfirstlane((int)skip7) != 0;
  }
  real armlim = sh.mrec[0][MR_IMP];
#pragma unroll
  for (int j = 1; j < 7; j++) armlim = sh.mrec[j][MR_IMP] < armlim ? sh.mrec[j][MR_IMP] : armlim;
  if (lane < 9) sh.lrec[lane][LR_JWDINV] = sh.lrec[lane][LR_JW] * sh.mrec[lane][MR_DINV];          // (J W) dinv of the arm joint (1 up to rounding)
  w.sync();
  // ---- residual rows.  A motor row whose clamp never acts takes  dl = z_g - lambda_g  in every update, so its lane carries the
  // residual r = z - lambda instead of z: the step is the lane's own value (ONE v_readlane, no clamp, no subtraction), every lane adds
  // Bn[g] * dl exactly as before -- for the other lanes r and z receive the same increment, the contact lanes keep holding z in the same
  // register -- and only the row's own lane differs: its coefficient is Bn[g][g] - 1 = -dinv A[g][g], so r_g falls to about 0.  The
  // multiplier is accumulated off the chain in the row's own lane (lam += [lane == g] dl: one v_fmac with an indicator register, where
  // the clamped row spends one v_add on its wave-uniform lamr[g]).  A residual row is v_readlane, v_fmac, v_fmac: three instructions
  // against the clamped row's five.  Inside a residual solve's iterations the 30 indicators are live and lamr[] is not -- it is filled
  // once after the verification (23 v_readlane), because the tail reads the motor multipliers as wave-uniform values.  Such rows are
  //   - the 23 pipe motor rows (PyBullet's load-time velocity motor: target 0, max impulse MR_IMP = 1), in both instantiations;
  //   - the arm motor rows 0..6 where their limit rows are left out (FULL == false): r_j = rhs_j + za_j, rhs_j folded in once.
  // That the clamp never acts is SPECULATED and VERIFIED: one v_max per iteration keeps the largest |lambda| every lane has held, and
  // after the solve each residual lane compares it with its own bound (verify below); if any fails the whole solve is run again with
  // the clamped rows and every arm limit row (PIH_S_SOLVER = 4), which is the arithmetic of the z form bit for bit.
  // pih_config.schedule + 64 (P.nospec): no residual rows at all, every env takes the clamped rows (A/B switch).
  real ind[NMOT];                            // [lane == g]: multiplier accumulation of residual row g (0..6: read by variant 1 only)
  real bown = 0;                             // Bn[lane] of a pipe motor lane in the z form (what the fallback puts back)
  const bool spec = __builtin_amdgcn_readfirstlane((int)P.nospec) == 0;
  if (spec) {
#pragma unroll
    for (int g = 0; g < NMOT; g++) {
      if (g == 7 || g == 8) { ind[g] = 0; continue; }
      const bool own = lane == g;
      ind[g] = own ? (real)1 : (real)0;
      if (g >= 9) { bown = own ? Bn[g] : bown; Bn[g] -= ind[g]; }      // own lane: (1 - dinv A_gg) - 1; every other lane: - 0
      __asm__ volatile("" : "+v"(ind[g]));     // a register, not a compare + select inside the loop
    }
  } else {
#pragma unroll
    for (int g = 0; g < NMOT; g++) ind[g] = 0;
  }
  // ---- multipliers: arm rows wave-uniform in VGPRs, every other row in its own lane
  real lam_a[9], lam_lo[9], lam_hi[9], lamr[NMOT];     // clamped pipe motor rows: wave-uniform multipliers (lam[g] += step: one issue slot)
  real lam = 0, z = 0;
  int it = 0;
  // FULL: every arm limit row; RES: pipe motor rows (and, without FULL, arm motor rows 0..6) in residual form.
  // Returns true if the solve has to be run again: an arm motor row clamped (!RES, !FULL) or the verification failed (RES).
  auto solve = [&](auto FULLTAG, auto RESTAG) __attribute__((always_inline)) -> bool {
    constexpr bool FULL = decltype(FULLTAG)::value;
    constexpr bool RES = decltype(RESTAG)::value;
    constexpr bool RESARM = RES && !FULL;
#pragma unroll
    for (int j = 0; j < 9; j++) { lam_a[j] = 0; lam_lo[j] = 0; lam_hi[j] = 0; }
#pragma unroll
    for (int g = 9; g < NMOT; g++) lamr[g] = 0;
    lam = lam0;
    {
      real v = 0;                          // warm start: J du of the cached normal multipliers, z = lambda + rhs - dinv (J du)
#pragma unroll
      for (int c = 0; c < MERGED_CONTACTS; c++)
        if (c < nc) v += Bn[NMOT + 3 * c] * sh.r_lam[3 * c];
      z = rhs + v;                         // (Bn = [own] - dinv A: the sum is  [own normal row] lam0 - dinv (J du))
      if (RESARM) z += rhsa;               // residual of arm motor rows 0..6 (lambda = 0)
    }
    real amax = 0;                           // largest |multiplier| any arm motor row 0..6 took during the solve (limit rows left out)
    real wmax = 0;                           // RES: largest |lam| this lane has held after any iteration
    auto iterate = [&](auto CHECKTAG, auto WELDTAG) __attribute__((always_inline)) -> bool {
      constexpr bool CHECK = decltype(CHECKTAG)::value;     // evaluate the early-exit test in this iteration? (see pgs_iteration_loop)
      constexpr bool WELD = decltype(WELDTAG)::value;       // attach / weld rows present (scripted mode): see pgs_rows2
      unsigned long long busy = 0;
      __asm__ volatile("" ::: "memory");      // keep the arm row constants in LDS (see pgs(): LICM would hoist and spill them)
      constexpr int PF = 4;
      real4 pa4[PF], pl4[PF];
#pragma unroll
      for (int k = 0; k < PF; k++) { pa4[k] = *reinterpret_cast<const real4*>(sh.mrec[k]); pl4[k] = *reinterpret_cast<const real4*>(sh.lrec[k]); }
      // the arm rows and the pipe motor rows do not see each other (A[arm row][pipe motor row] = 0): two accumulators, two chains
      real za = z, zp = z;
      // The 9 arm joint blocks are spread evenly over the 23 pipe motor rows (block k in front of row 23 k / 9): a clamped pipe row is
      // med3, sub, <1 wait state>, v_readlane, <2 wait states>, fmac, a residual one v_readlane, <2 wait states>, fmac, and the
      // instructions of an arm block are what fills those slots (with all arm blocks up front the last 14 pipe rows ran with three
      // s_nop slots each).  The two chains commute exactly.
#pragma unroll
      for (int jp = 0; jp < PIH_OBJ_NJ; jp++) {
        const int j = (jp * 9 + PIH_OBJ_NJ - 1) / PIH_OBJ_NJ;         // the arm block in front of pipe row jp, if 23 j / 9 == jp
        if (j < 9 && (PIH_OBJ_NJ * j) / 9 == jp) {   // arm joint block: motor, lower limit, upper limit; y = dinv (J du) of the joint
          if (RESARM && j < 7) {
            // residual arm motor row: the step is the lane's own value (the record ring still turns: joints 7, 8 read their slots)
            if (j + PF < 9) { pa4[j % PF] = *reinterpret_cast<const real4*>(sh.mrec[j + PF]); pl4[j % PF] = *reinterpret_cast<const real4*>(sh.lrec[j + PF]); }
            const real dl = rdlane(za, j);
            if (CHECK) busy |= __ballot(absr(za) > thr) & (1ull << j);
            lam += ind[j] * dl;
            za += Bn[j] * dl;
          } else {
            const real4 ca = pa4[j % PF], cl = pl4[j % PF];
            if (j + PF < 9) { pa4[j % PF] = *reinterpret_cast<const real4*>(sh.mrec[j + PF]); pl4[j % PF] = *reinterpret_cast<const real4*>(sh.lrec[j + PF]); }
            real d2, d3;
            if (FULL || j >= 7) {
              const real dl = arm_joint_rows<CHECK, true>(ca, cl, -rdlane(za, j), lam_a[j], lam_lo[j], lam_hi[j], busy, d2, d3);
              za += Bn[j] * (dl + d2 - d3);
            } else {
              const real dl = arm_joint_rows<CHECK, false>(ca, cl, -rdlane(za, j), lam_a[j], lam_lo[j], lam_hi[j], busy, d2, d3);
              amax = max_(amax, absr(lam_a[j]));                    // watched in EVERY iteration (one v_max): a multiplier may touch its bound and leave it again
              za += Bn[j] * dl;
            }
          }
        }
        const int g = 9 + jp;
        if (RES) {
          // residual pipe motor row 9 + jp: the row's lane supplies the step, |r_g| before the update is the |dl| of the exit test
          const real sdl = rdlane(zp, g);
          if (CHECK) busy |= __ballot(absr(zp) > thr) & (1ull << g);
          lam += ind[g] * sdl;
          zp += Bn[g] * sdl;
        } else {
          // pipe motor row 9 + jp: every lane clamps its own z, the row's lane supplies the step
          const real cand = med3_(zp, -ubv, ubv);              // (the motor rows' bounds are symmetric; two vector sources, see gs_row2_normal)
          const real dlv = cand - lamr[g];
          const real sdl = rdlane(dlv, g);
          if (CHECK) busy |= __ballot(absr(dlv) > thr) & (1ull << g);
          lamr[g] += sdl;
          zp += Bn[g] * sdl;
        }
      }
      z = (za + zp) - z;
      if (RES) wmax = max_(wmax, absr(lam));   // (every lane: the contact lanes' values are never looked at)
      // contacts: normal, dir1, dir2 -- the friction bounds follow the normal multiplier; Bullet leaves the friction rows of an
      // unloaded contact alone: a wave-uniform branch (half of the listed contacts are unloaded; collapsing their bounds onto the
      // current multiplier instead -- branch-free, step 0 -- costs the 14 VALU of two rows for nothing: 263 k vs 247 k cycles at 8-10)
      // (nc and angmask through scalars that are opaque at every contact: the loop-invariant exit / friction conditions would otherwise
      //  be precomputed as 64-bit lane masks outside the iteration loop, spilled to VGPR lanes and read back with v_readlane in every
      //  iteration -- or the loop given a run-time trip count.  One copy per iteration, "modified" in place: no instruction per contact)
      int ncl = nc; unsigned am = angmask;
#pragma unroll
      for (int c = 0; c < MERGED_CONTACTS; c++) {
        __asm__ volatile("" : "+s"(ncl), "+s"(am));
        if (c >= ncl) break;
        const int g0 = NMOT + 3 * c;
        real dl, s0;
        gs_row1_normal(z, Bn[g0], lbv, lam, g0, dl, s0);
        if (CHECK) busy |= __ballot(absr(dl) > thr) & (1ull << g0);
        // wave-uniform branch on  s0 > 0 || weld row  (as integers, on the scalar unit: see pgs_rows2)
        const int s0i = __builtin_bit_cast(int, s0), weld = WELD ? (int)((am >> c) & 1u) : 0;
        if (WELD ? (s0i > weld ? s0i : weld) > 0 : s0i > 0) {
          const real hi = max_(cmu * s0, cfl);
          real dl2;
          gs_row1_friction2(z, Bn[g0 + 1], Bn[g0 + 2], hi, lam, g0 + 1, g0 + 2, dl, dl2);
          if (CHECK) busy |= (__ballot(absr(dl) > thr) & (1ull << (g0 + 1))) | (__ballot(absr(dl2) > thr) & (1ull << (g0 + 2)));
        }
      }
      return CHECK && busy == 0;
    };
    // (the speculating instantiations carry the doubled unchecked body; the clamped ones -- the fallback, fewer than 1 in 10^4 env-steps,
    //  and the A/B switch -- a single copy, which holds the code size)
    if (angmask != 0) it = pgs_iteration_loop<RES>(P.iters, P.checkstride, [&]() __attribute__((always_inline)) { return iterate(std::true_type{}, std::true_type{}); }, [&]() __attribute__((always_inline)) { return iterate(std::false_type{}, std::true_type{}); });
    else it = pgs_iteration_loop<RES>(P.iters, P.checkstride, [&]() __attribute__((always_inline)) { return iterate(std::true_type{}, std::false_type{}); }, [&]() __attribute__((always_inline)) { return iterate(std::false_type{}, std::false_type{}); });
    if (RES) {
      // ---- verification.  A residual row is the clamped row as long as its multiplier stays inside (-bound, bound).  The two forms round
      // differently: each accumulates at most 50 x 30 increments, every one rounded to 2^-24 relative, so their multipliers can part by
      // about 1 500 x 2^-24 ~ 1e-4 of their size.  The test asks for |lambda| < bound (1 - 2^-7) at every iteration's end -- eighty times
      // that -- so a row that passes is not clamped in the z form either.  (Measured multipliers stay an order of magnitude below the
      // bound: DESIGN 6.2.)  Compared as bit patterns -- for non-negative floats the integer order is the float order, NaN and Inf
      // lie above every finite value -- so that a non-finite multiplier, bound or maximum fails the test whatever -ffast-math assumes;
      // v_max may drop a NaN operand, hence the final lam is tested as well (a non-finite multiplier stays non-finite).
      const bool resrow = (lane >= 9 && lane < NMOT) || (RESARM && lane < 7);
      const real bound = lane < 7 ? armlim : ubv;
      const unsigned lb = __builtin_bit_cast(unsigned, bound * (real)0.9921875);
      const unsigned wb = __builtin_bit_cast(unsigned, wmax), fb = __builtin_bit_cast(unsigned, lam) & 0x7fffffffu;
      const bool ok = lb < 0x7f800000u && wb < lb && fb < lb;
      if (__ballot(resrow && !ok) != 0) return true;
      // the tail below reads the multipliers of the motor rows as wave-uniform values
#pragma unroll
      for (int g = 9; g < NMOT; g++) lamr[g] = rdlane(lam, g);
      if (RESARM) {
#pragma unroll
        for (int j = 0; j < 7; j++) lam_a[j] = rdlane(lam, j);
      }
      return false;
    }
    return !FULL && __builtin_amdgcn_readfirstlane(amax >= armlim ? 1 : 0) != 0;   // (armlim = the smallest bound of rows 0..6: conservative if they differ, exact if equal)
  };
  // one call site per instantiation (each is some 10^4 instructions)
  int variant = skip7 ? 1 : 2;
  bool again;
  if (spec) again = skip7 ? solve(std::false_type{}, std::true_type{}) : solve(std::true_type{}, std::true_type{});
  else again = skip7 ? solve(std::false_type{}, std::false_type{}) : true;
  if (again) {
    if (spec) {                              // back to the z form: the own-lane coefficients of the pipe motor rows
#pragma unroll
      for (int g = 9; g < NMOT; g++) Bn[g] = lane == g ? bown : Bn[g];
    }
    solve(std::true_type{}, std::false_type{});
    if (spec || skip7) variant = 4;
  }
  if (lane == 0) sh.S[PIH_S_SOLVER] = (real)variant;
  // multipliers back to LDS: contacts -> r_lam, pipe motors -> MR_LAM of their (now unused) constant record
  if (lane >= NMOT && lane < NMOT + 3 * nc) sh.r_lam[lane - NMOT] = lam;
#pragma unroll
  for (int g = 9; g < NMOT; g++) if (lane == 0) sh.mrec[g][MR_LAM] = lamr[g];
  w.sync();
  {
    const int d = lane, dw = d < ND ? d : ND;
    real du = 0;
    if (d < 9) {
#pragma unroll
      for (int j = 0; j < 9; j++) du += wma_row(sh, j)[d] * (lam_a[j] + lam_lo[j] - lam_hi[j]);
    } else if (d < ND) {
#pragma unroll
      for (int j = 0; j < PIH_OBJ_NJ; j++) du += wmp_row(sh, j)[d - 9] * sh.mrec[9 + j][MR_LAM];
    }
#pragma unroll
    for (int c = 0; c < MERGED_CONTACTS; c++)
      if (c < nc) du += sh.b.Wp[3 * c][dw] * sh.r_lam[3 * c] + sh.b.Wp[3 * c + 1][dw] * sh.r_lam[3 * c + 1] + sh.b.Wp[3 * c + 2][dw] * sh.r_lam[3 * c + 2];
    if (d < ND) sh.u[d] += du;
  }
  w.sync();
  return it;
}

// ---- the same solver with TWO rows per lane, for envs with 11 .. HC contacts (128 rows; a fifth of the env-steps of the benchmark
// workload and every one of its slowest: their DOF-space blocks were what a launch of 4096 envs waited for).  Row g lives in lane
// g % 64 of register set g / 64.  The 128 x 128 matrix no longer fits the register file: the columns of the 32 motor rows (KREG = NMOT)
// stay in registers, those of the contact rows are written once per step to the env's scratch in global memory
// ([column][lane][2], 512 B per column, L2-resident) and streamed through a ring of D prefetched columns in every iteration --
// the addresses do not depend on the solve, so the loads are issued a ring ahead and never sit on the row chain.
// Motor columns come from the symmetry of the Delassus matrix, A[r][motor m] = W_r[dof(m)], without a dot product.
PIH_HD int pgs_rows2(Wave& w, Shared& sh, const Params& P, const Ovf& ov, const MotorW& mw) {
  const int nc = __builtin_amdgcn_readfirstlane(sh.nc);
  w.sync();
  const int lane = w.lane();
  constexpr int D = 12;                                    // ring depth (columns in flight)
  real* const Bg = ov.base + OVF_B_OFF + 2 * lane;         // this lane's slot of streamed column s: Bg[s * 128 .. +1]
  // one streamed column (both rows of the lane) = one 8-byte load at  (uniform column pointer) + lane * 8: global_load_dwordx2 with the
  // pointer in an SGPR pair and the column in the instruction's immediate offset.  The pointer is made opaque once per iteration
  // (otherwise the addresses of all 96 columns are loop invariants: hoisted out of the iteration loop and spilled).  No clamp on the
  // column index: the ring runs up to D columns past the last one written, inside the env's own scratch (the parked motor rows
  // behind the column area and, for the last env of the batch, OVF_PAD_WORDS of slack), and those values are never used.
  static_assert(OVF_MW_WORDS + OVF_PAD_WORDS >= D * 128, "the ring reads D columns past the streamed-column area");
  const unsigned l8 = (unsigned)lane * 8u;
  // ---- rows of this lane: r0 = lane (motor row, or contact row lane - 32), r1 = 64 + lane (contact row 32 + lane)
  struct RowC { real di, rhs, thr, lb, ub, mu, fl, lam0; };
  auto rowconst = [&](int g) __attribute__((always_inline)) -> RowC {
    RowC r; r.di = 0; r.rhs = 0; r.thr = PIH_BIG; r.lb = 0; r.ub = 0; r.mu = 0; r.fl = 0; r.lam0 = 0;
    if (g < 9) r.di = sh.mrec[g][MR_DINV];
    else if (g < NMOT) { r.di = sh.mrec[g][MR_DINV]; r.rhs = sh.mrec[g][MR_RHS]; r.thr = sh.mrec[g][MR_THRESH]; r.ub = sh.mrec[g][MR_IMP]; r.lb = -r.ub; }
    else {
      const int row = g - NMOT, c = row / 3, k = row - 3 * c;
      if (c < nc) {
        const real* R = crec_of(sh, ov, c);
        r.di = R[CR_DINV0 + CR_KSTRIDE * k]; r.rhs = R[CR_RHS + k]; r.thr = R[CR_THRESH + k]; r.mu = R[CR_MU]; r.fl = R[CR_FLOOR];
        if (k == 0) { r.lb = R[CR_LB]; r.ub = PIH_BIG; r.lam0 = sh.r_lam[3 * c]; }
      }
    }
    return r;
  };
  const RowC c0 = rowconst(lane), c1 = rowconst(64 + lane);
  // ---- columns.  Bn[i] = [own row] - dinv A[i]
  pk2 BB[KREG];                                            // (row of register set 0, row of register set 1) per column
  // motor columns by symmetry: A[r][m] = W_r[dof(m)].  Contact rows read their own response row; motor rows take the (lane = DOF)
  // registers of the motor rows: arm lane r holds W_m[r] itself, pipe lane r finds W_m[dof(r)] six lanes up
  {
    const int row0 = lane - NMOT, row1 = 32 + lane;                 // contact-row index of r0 (if >= 0) and r1
    const real* w0 = row0 >= 0 && row0 < 3 * nc ? wp_row(sh, ov, row0) : nullptr;
    const real* w1 = row1 < 3 * nc ? wp_row(sh, ov, row1) : nullptr;
#pragma unroll
    for (int m = 0; m < NMOT; m++) {
      const int dm = m < 9 ? m : 15 + (m - 9);
      real a0;
      if (m < 9) a0 = lane < 9 ? mw.w[m] : (real)0;
      else {
        const real up = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(4 * ((lane + 6) & 63), __builtin_bit_cast(int, mw.w[m - 9])));
        a0 = (lane >= 9 && lane < NMOT) ? up : (real)0;
      }
      if (w0) a0 = w0[dm];
      const real a1 = w1 ? w1[dm] : (real)0;
      // (no pin between the 32 columns: the 64 reads -- LDS, or the scratch in global memory for rows of contacts >= CL -- target the
      //  registers that stay, and all are in flight together instead of 32 serialised round trips)
      BB[m] = pk_pack(((lane == m && m >= 9) ? (real)1 : (real)0) - c0.di * a0, -c1.di * a1);
    }
  }
  // the motor rows' registers are not needed again before the very end: park them in the env's scratch
  real* const Mg = ov.base + OVF_MW_OFF + lane;
#pragma unroll
  for (int j = 0; j < PIH_OBJ_NJ; j++) Mg[j * 64] = mw.w[j];
  // ---- Jacobian rows (registers) of both rows of the lane
  pk2 JJ[ND];                                              // (entry d of the row in register set 0, of the row in set 1)
  {
    auto geom = [&](int g, int& la, int& lb, V3& p, V3& dir, bool& ang, bool& live) __attribute__((always_inline)) {
      la = -1; lb = -1; p = mk(0, 0, 0); dir = mk(0, 0, 0); ang = false; live = false;
      if (g < NMOT) return;
      const int row = g - NMOT, c = row / 3, k = row - 3 * c;
      if (c >= nc) return;
      live = true; la = sh.c_la[c]; lb = sh.c_lb[c];
      const real* R = crec_of(sh, ov, c);
      p = ld3(R + CR_P); dir = ld3(R + CR_DIR0 + CR_KSTRIDE * k); ang = R[CR_ANG] != 0;
    };
    int la0, lb0, la1, lb1; V3 p0, d0, p1, d1; bool a0, a1, l0, l1;
    geom(lane, la0, lb0, p0, d0, a0, l0); geom(64 + lane, la1, lb1, p1, d1, a1, l1);
    const int md = lane < 9 ? lane : 15 + (lane - 9);
    DofGeom gn = dof_geom(sh, 0);
#pragma unroll
    for (int d = 0; d < ND; d++) {
      const DofGeom g = gn;
      if (d + 1 < ND) gn = dof_geom(sh, d + 1);
      real j0 = lane < NMOT ? (d == md ? (real)1 : (real)0) : (l0 ? jac_entry(g, la0, lb0, p0, d0, a0) : (real)0);
      real j1 = l1 ? jac_entry(g, la1, lb1, p1, d1, a1) : (real)0;
      __asm__ volatile("" : "+v"(j0), "+v"(j1) :: "memory");
      JJ[d] = pk_pack(j0, j1);
    }
  }
  // contact columns: J . W_i, the response row W_i broadcast from LDS (contacts < CL) or from the env's scratch
  w.sync();
  // Both rows of the lane advance with one v_pk_fma_f32 per response-row entry; the entries are read in pairs (w_d, w_d+1) and the
  // packed FMA picks the half (op_sel), so that the 228 FMAs + 114 reads of a contact become 114 + 57.  Two loops, because the rows of
  // contacts < CL are LDS words and those of contacts >= CL global words: one loop over a generic pointer made every read a flat_load
  // under a branch.  (Rows are 39 words apart: 4-byte aligned pairs, which ds_read2_b32 / global_load_dwordx2 accept.)
  static_assert(ND % 2 == 0 && KREG == NMOT, "entries are consumed in pairs; every contact column is streamed");
  real wv0 = 0, wv1 = 0;                                     // warm start: sum over the contacts of (normal column) x (cached multiplier), see below
  auto column = [&](int cb, auto pairof) __attribute__((always_inline)) {
    pk2 acc[3] = {0, 0, 0};
    // (blocks of 4 DOFs = 6 pairs, requested one block ahead of their use: left alone the scheduler, at the register limit, issues
    //  each read right in front of its FMA -- 57 serialised LDS round trips per contact)
    constexpr int NB = (ND + 3) / 4;
    pk2 wq[2][6];
    auto request = [&](int blk, pk2* q) __attribute__((always_inline)) {
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int k = 0; k < 3; k++) { const int d = 4 * blk + 2 * h; q[3 * h + k] = d < ND ? pairof(k * WPS + d) : (pk2)0; }
    };
    request(0, wq[0]);
#pragma unroll
    for (int blk = 0; blk < NB; blk++) {
      if (blk + 1 < NB) request(blk + 1, wq[(blk + 1) & 1]);
      __asm__ volatile("" ::: "memory");                   // the next block's reads stay in front of this block's FMAs
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int d = 4 * blk + 2 * h;
        if (d < ND) {
#pragma unroll
          for (int k = 0; k < 3; k++) { pk_fma_lo(acc[k], JJ[d], wq[blk & 1][3 * h + k]); pk_fma_hi(acc[k], JJ[d + 1], wq[blk & 1][3 * h + k]); }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int i = NMOT + 3 * cb + k;
      const real b0 = (lane == i ? (real)1 : (real)0) - c0.di * pk_lo(acc[k]), b1 = (64 + lane == i ? (real)1 : (real)0) - c1.di * pk_hi(acc[k]);
      Bg[(size_t)(i - KREG) * 128] = b0; Bg[(size_t)(i - KREG) * 128 + 1] = b1;
      if (k == 0) { const real l = sh.r_lam[3 * cb]; wv0 += b0 * l; wv1 += b1 * l; }   // (while the column is in registers: reading it back cost a round trip per contact)
    }
  };
  {
    const int nl = nc < CL ? nc : CL;
#pragma unroll 1
    for (int cb = 0; cb < nl; cb++) {
      const real* wr = sh.b.Wp[3 * cb];
      column(cb, [&](int o) __attribute__((always_inline)) { return pk_pack(wr[o], wr[o + 1]); });
    }
    typedef const real __attribute__((address_space(1)))* grp;
#pragma unroll 1
    for (int cb = CL; cb < nc; cb++) {
      const grp wr = (grp)(ov.base + (size_t)(3 * (cb - CL)) * WPS);
      column(cb, [&](int o) __attribute__((always_inline)) { return pk_pack(wr[o], wr[o + 1]); });
    }
  }
#pragma unroll
  for (int q = NMOT; q < KREG; q++) if (q >= NMOT + 3 * nc) BB[q] = 0;
  unsigned angmask = 0;
  for (int c = 0; c < nc; c++) { const real* R = crec_of(sh, ov, c); if (R[CR_MU] < 0) angmask |= 1u << c; }
  angmask = (unsigned)__builtin_amdgcn_readfirstlane((int)angmask);
  if (lane < 9) sh.lrec[lane][LR_JWDINV] = sh.lrec[lane][LR_JW] * sh.mrec[lane][MR_DINV];          // (J W) dinv of the arm joint (1 up to rounding)
  __threadfence_block();                                     // the streamed columns: written above, read back by the same lane
  w.sync();
  // ---- solve (every limit row in place)
  // (the arm joints' three multipliers -- motor, lower, upper limit -- are wave-uniform values in registers and the joint block is
  //  arm_joint_rows, as in pgs_rows: the register budget is set by pgs_rows, and three v_readlane + three lane commits per joint and
  //  iteration were the price of lanes)
  real lam0 = c0.lam0, lam1 = c1.lam0, z0, z1;
  real lam_a[9], lam_lo[9], lam_hi[9];
#pragma unroll
  for (int j = 0; j < 9; j++) { lam_a[j] = 0; lam_lo[j] = 0; lam_hi[j] = 0; }
  z0 = c0.rhs + wv0; z1 = c1.rhs + wv1;                      // warm start: z = lambda + rhs - dinv (J du) (see pgs_rows)
  // WELD: the env has attach / weld rows (scripted mode, states 4-6), whose friction rows run whatever the normal multiplier is; without
  // them (always in action mode) the per-contact test is a scalar compare of s0's bit pattern alone.  (Round 4: one instantiation per
  // case; the combined test had come out as five instructions -- v_and, v_max_i32, v_cmp, s_and, s_cbranch -- per contact.)
  auto iterate = [&](auto CHECKTAG, auto WELDTAG) __attribute__((always_inline)) -> bool {
    constexpr bool CHECK = decltype(CHECKTAG)::value;
    constexpr bool WELD = decltype(WELDTAG)::value;
    unsigned long long busy = 0;
    __asm__ volatile("" ::: "memory");
    // ring of streamed columns: the first D are requested before the motor rows
    typedef const char __attribute__((address_space(1)))* gcp;
    typedef const pk2 __attribute__((address_space(1)))* gpp;
    gcp colp = (gcp)(ov.base + OVF_B_OFF);
    __asm__ volatile("" : "+s"(colp));
    auto ldcol = [&](int sidx) __attribute__((always_inline)) -> pk2 { return *(gpp)(colp + (size_t)sidx * 512 + l8); };
    pk2 rr[D];
#pragma unroll
    for (int s = 0; s < D; s++) rr[s] = ldcol(s);
    constexpr int PF = 2;
    real4 pa4[PF], pl4[PF];
#pragma unroll
    for (int k = 0; k < PF; k++) { pa4[k] = *reinterpret_cast<const real4*>(sh.mrec[k]); pl4[k] = *reinterpret_cast<const real4*>(sh.lrec[k]); }
    real za = z0; pk2 zp1 = pk_pack(z0, z1);               // arm chain; (pipe chain, register set 1)
#pragma unroll
    for (int j = 0; j < PIH_OBJ_NJ; j++) {
      if (j < 9) {
        const real4 ca = pa4[j % PF], cl = pl4[j % PF];
        if (j + PF < 9) { pa4[j % PF] = *reinterpret_cast<const real4*>(sh.mrec[j + PF]); pl4[j % PF] = *reinterpret_cast<const real4*>(sh.lrec[j + PF]); }
        real d2, d3;
        const real dl = arm_joint_rows<CHECK, true>(ca, cl, -rdlane(za, j), lam_a[j], lam_lo[j], lam_hi[j], busy, d2, d3);
        const real tot = dl + d2 - d3;
        za += pk_lo(BB[j]) * tot; zp1 = pk_pack(pk_lo(zp1), pk_hi(zp1) + pk_hi(BB[j]) * tot);
      }
      const int g = 9 + j;
      real dlv;
      gs_row2_bounded(zp1, pk_lo(zp1), BB[g], c0.ub, lam0, g, dlv);
      if (CHECK) busy |= __ballot(absr(dlv) > c0.thr) & (1ull << g);
    }
    pk2 zz = pk_pack((za + pk_lo(zp1)) - z0, pk_hi(zp1));
    // one row (gs_row_normal / gs_row_friction): clamp the lane's own z, take the row's step from its lane, move every z
    // (nc and angmask through scalars that are opaque at every contact: the 2 x 32 loop-invariant exit / friction conditions would
    //  otherwise be precomputed as 64-bit lane masks outside the iteration loop and spilled, or the loop given a run-time trip count
    //  and not unrolled.  One copy per iteration, modified "in place" by the empty asm: no instruction per contact)
    int ncl = nc; unsigned am = angmask;
    unsigned l8c = l8;
    gcp colq = colp + D * 512;                               // column 3 c + D: what contact c requests
    __asm__ volatile("" : "+s"(colq));
#pragma unroll
    for (int c = 0; c < HC; c++) {
      __asm__ volatile("" : "+s"(ncl), "+s"(am), "+v"(l8c));   // (l8c: its zero extension must be visible in the contact's own basic block
                                                               //  for the scalar-base + 32-bit-lane-offset form of global_load)
      if (c >= ncl) break;
      const int g0 = NMOT + 3 * c;
      pk2 bb[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int sc = g0 + k - KREG;                        // (KREG = NMOT: every contact column is streamed)
        bb[k] = rr[sc % D];
        rr[sc % D] = *(gpp)(colq + ((c & 1) * 3 + k) * 512 + l8c);   // request the column a ring ahead (immediate offsets 0 .. 2 560)
      }
      if (c & 1) {
        colq += 6 * 512;
        __asm__ volatile("" : "+s"(colq));                 // (the running pointer stays in an SGPR pair: s_add_u32 / s_addc_u32 per PAIR of contacts)
      }
      real dl, s0;
      if (g0 < 64) { gs_row2_normal(zz, pk_lo(zz), bb[0], c0.lb, lam0, g0, dl, s0); if (CHECK) busy |= __ballot(absr(dl) > c0.thr) & (1ull << g0); }
      else { gs_row2_normal(zz, pk_hi(zz), bb[0], c1.lb, lam1, g0 - 64, dl, s0); if (CHECK) busy |= __ballot(absr(dl) > c1.thr) & (1ull << (g0 - 64)); }
      // Bullet leaves the friction rows of an unloaded contact alone: wave-uniform branch on  s0 > 0 || weld row  -- as integers, on
      // the scalar unit (the bit pattern of a positive float is a positive integer)
      const int s0i = __builtin_bit_cast(int, s0), weld = WELD ? (int)((am >> c) & 1u) : 0;
      if (WELD ? (s0i > weld ? s0i : weld) > 0 : s0i > 0) {
        auto friction = [&](int g, pk2 col) __attribute__((always_inline)) {      // (row g lives in register set g / 64)
          if (g < 64) { const real h0 = max_(c0.mu * s0, c0.fl); gs_row2_friction(zz, pk_lo(zz), col, h0, lam0, g, dl); if (CHECK) busy |= __ballot(absr(dl) > c0.thr) & (1ull << g); }
          else { const real h1 = max_(c1.mu * s0, c1.fl); gs_row2_friction(zz, pk_hi(zz), col, h1, lam1, g - 64, dl); if (CHECK) busy |= __ballot(absr(dl) > c1.thr) & (1ull << (g - 64)); }
        };
        friction(g0 + 1, bb[1]);
        friction(g0 + 2, bb[2]);
      }
    }
    z0 = pk_lo(zz); z1 = pk_hi(zz);
    return CHECK && busy == 0;
  };
  int it;
  if (angmask != 0) it = pgs_iteration_loop<false>(P.iters, P.checkstride, [&]() __attribute__((always_inline)) { return iterate(std::true_type{}, std::true_type{}); }, [&]() __attribute__((always_inline)) { return iterate(std::false_type{}, std::true_type{}); });
  else it = pgs_iteration_loop<false>(P.iters, P.checkstride, [&]() __attribute__((always_inline)) { return iterate(std::true_type{}, std::false_type{}); }, [&]() __attribute__((always_inline)) { return iterate(std::false_type{}, std::false_type{}); });
  if (lane == 0) sh.S[PIH_S_SOLVER] = 5;
  // ---- multipliers back to LDS, DOF velocities du = sum_i W_i lambda_i
  if (lane >= NMOT && lane < NMOT + 3 * nc) sh.r_lam[lane - NMOT] = lam0;
  if (32 + lane < 3 * nc) sh.r_lam[32 + lane] = lam1;
  if (lane >= 9 && lane < NMOT) sh.mrec[lane][MR_LAM] = lam0;
#pragma unroll
  for (int j = 0; j < 9; j++) if (lane == 0) sh.mrec[j][MR_LAM] = lam_a[j] + lam_lo[j] - lam_hi[j];
  w.sync();
  {
    const int d = lane, dw = d < ND ? d : ND;
    real du = 0;
#pragma unroll
    for (int j = 0; j < PIH_OBJ_NJ; j++) {
      du += Mg[j * 64] * (d < 9 ? (j < 9 ? sh.mrec[j][MR_LAM] : (real)0) : sh.mrec[9 + j][MR_LAM]);
    }
    // du += sum_r W_r[d] lambda_r: rows of contacts < CL from LDS, the others from the env's scratch -- two loops with known address
    // spaces, four reads in flight (one loop over the generic row pointer was a serialised round trip per row, flat loads to global
    // memory for the rows of contacts >= CL)
    {
      const int nl = 3 * (nc < CL ? nc : CL);
#pragma unroll 8
      for (int r = 0; r < nl; r++) du += sh.b.Wp[r][dw] * sh.r_lam[r];
      typedef const real __attribute__((address_space(1)))* grp;
      const grp wg = (grp)ov.base;
#pragma unroll 4
      for (int r = 3 * CL; r < 3 * nc; r++) du += wg[(size_t)(r - 3 * CL) * WPS + dw] * sh.r_lam[r];
    }
    if (d < ND) sh.u[d] += du;
  }
  w.sync();
  return it;
}

// Sequential impulse, Bullet resolveSingleConstraintRowGeneric form; row order: per arm joint (motor, lower limit, upper
// limit), the 23 pipe motors, then per contact (normal, dir1, dir2).  Returns iterations executed.
// GPU form: one lane per DOF holds its entry of the velocity change `du`; row multipliers live lane-distributed in
// registers (v_readlane to broadcast); motor response rows are preloaded into registers; the arm and pipe motor chains
// commute (disjoint DOFs) and are interleaved for ILP; each contact is solved as an exact 3x3 Gauss-Seidel block: three
// DPP row-reductions in flight at once, then the cross terms G bring dir1/dir2 up to date without touching `du`.
PIH_HD int pgs(Wave& w, Shared& sh, const Params& P, const Ovf& ov, const MotorW& mw) {
  const int nc = sh.nc;
  if (P.pgsmode == 0 && nc <= MERGED_CONTACTS) return pgs_rows(w, sh, P);   // all rows fit one wavefront: row-space solver
  if (P.pgsmode == 0 && nc <= HC) return pgs_rows2(w, sh, P, ov, mw);       // two rows per lane
  if (w.lane() == 0) sh.S[PIH_S_SOLVER] = 0;
  // early exit test without divisions: (dl / dinv)^2 <= resid  <=>  dl^2 - resid dinv^2 <= 0  for every row
  w.sync();
  const int d = w.lane();
  const DofGeom g = dof_geom(sh, d);
  const bool armlane = d < 9;
  const int dw = d < ND ? d : ND;   // response-row word of this lane (idle lanes read the zero pad)
  // motor / limit multipliers: wave-uniform values held in VGPRs (no readlane, no conditional write-back);
  // contact multipliers: lane-distributed, contact c in lane c
  real lam_p[PIH_OBJ_NJ], lam_a[9], lam_lo[9], lam_hi[9];
#pragma unroll
  for (int j = 0; j < PIH_OBJ_NJ; j++) lam_p[j] = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) { lam_a[j] = 0; lam_lo[j] = 0; lam_hi[j] = 0; }
  // per-lane sign of every contact's Jacobian column, 2 bits per contact (two's complement: 00 = 0, 01 = +1, 11 = -1, read
  // back with one v_bfe_i32): +1 if this lane's joint is an ancestor of linkA, -1 of linkB, 0 of both or neither
  unsigned sg0 = 0, sg1 = 0, sg2 = 0;
  // Jacobian column of this lane for a point p: cross(ae, p - g.o) + mp  (revolute-like: ae = axis, mp = 0; prismatic-like:
  // ae = 0, mp = axis; unused lane: both 0) -- no per-contact select
  const V3 ae = g.kind == 0 ? g.a : mk(0, 0, 0), mp = g.kind == 1 ? g.a : mk(0, 0, 0);
  real du = 0;
  int ang_c = -1;
  for (int c = 0; c < nc; c++) {
    int la = sh.c_la[c], lb = sh.c_lb[c];
    if (sh.c_mu[c] < (real)-1.5) ang_c = c;
    int sgn = g.kind != 2 ? (int)is_anc(g.L, la) - (int)is_anc(g.L, lb) : 0;
    unsigned code = (unsigned)sgn & 3u;
    if (c < 16) sg0 |= code << (2 * c); else if (c < 32) sg1 |= code << (2 * (c - 16)); else sg2 |= code << (2 * (c - 32));
    real l = sh.r_lam[3 * c];   // warm start (uniform LDS read)
    if (l != 0) {
      du += (c < CL ? sh.b.Wp[3 * c][dw] : ov.base[(size_t)(3 * (c - CL)) * WPS + dw]) * l;
    }
  }
  const int ang_cs = __builtin_amdgcn_readfirstlane(ang_c);
  // one PGS iteration; returns true when every row moved by less than its threshold
  auto iterate = [&](auto CHECKTAG) __attribute__((always_inline)) -> bool {
    constexpr bool CHECK = decltype(CHECKTAG)::value;     // evaluate the early-exit test in this iteration? (see pgs_iteration_loop)
    // Early exit (Bullet's least-squares residual test, max over rows of (d lambda / dinv)^2 <= resid) as |d lambda| >
    // sqrt(resid) dinv per row: one v_cmp into a wave mask + a scalar OR per row instead of an FMA and a max.  Bit 32 is read:
    // the motor chain is wave-uniform and the contact chain is valid in lanes 32..47.
    unsigned long long busy = 0;
    // the row constants are re-read from LDS every iteration ON PURPOSE: without this compiler barrier LICM hoists all
    // ~155 loop-invariant loads out of the iteration loop and spills them to scratch inside the hot loop
    __asm__ volatile("" ::: "memory");
    // row constants come from LDS as 16-byte broadcasts, explicitly prefetched PF records ahead: the dependent chain of one
    // motor step is ~6 VALU ops (~50 cycles) while an LDS round trip is >100, so a distance-1 prefetch stalls every step
    constexpr int PF = 6;
    real4 pm[PF], pa4[PF], pl4[PF];
#pragma unroll
    for (int k = 0; k < PF; k++) { pm[k] = *reinterpret_cast<const real4*>(sh.mrec[9 + k]); pa4[k] = *reinterpret_cast<const real4*>(sh.mrec[k]); pl4[k] = *reinterpret_cast<const real4*>(sh.lrec[k]); }
#pragma unroll
    for (int j = 0; j < PIH_OBJ_NJ; j++) {
      real tot_a = 0;
      const real4 cm = pm[j % PF];
      if (j + PF < PIH_OBJ_NJ) pm[j % PF] = *reinterpret_cast<const real4*>(sh.mrec[9 + j + PF]);
      if (j < 9) {   // arm joint block: motor, lower limit, upper limit (wave-uniform chain)
        const real4 ca = pa4[j % PF], cl = pl4[j % PF];
        if (j + PF < 9) { pa4[j % PF] = *reinterpret_cast<const real4*>(sh.mrec[j + PF]); pl4[j % PF] = *reinterpret_cast<const real4*>(sh.lrec[j + PF]); }
        const real di = rec4<MR_DINV>(&ca), rhs = rec4<MR_RHS>(&ca), thr = rec4<MR_THRESH>(&ca), lim = rec4<MR_IMP>(&ca);
        const real lor = rec4<LR_LO>(&cl), hir = rec4<LR_HI>(&cl), wjj = rec4<LR_JW>(&cl);
        real dj = rdlane(du, j);
        real sum = lam_a[j] + (rhs - dj * di);
        sum = med3_(sum, -lim, lim);
        real dl = sum - lam_a[j]; lam_a[j] = sum;
        if (CHECK) busy |= __ballot(absr(dl) > thr);
        dj += dl * wjj;
        real s2 = lam_lo[j] + (lor - dj * di); s2 = max_(s2, (real)0);
        real d2 = s2 - lam_lo[j]; lam_lo[j] = s2;
        if (CHECK) busy |= __ballot(absr(d2) > thr);
        dj += d2 * wjj;
        real s3 = lam_hi[j] + (hir + dj * di); s3 = max_(s3, (real)0);
        real d3 = s3 - lam_hi[j]; lam_hi[j] = s3;
        if (CHECK) busy |= __ballot(absr(d3) > thr);
        tot_a = dl + d2 - d3;
      }
      // pipe joint motor j (DOF 15 + j)
      const real di = rec4<MR_DINV>(&cm), rhs = rec4<MR_RHS>(&cm), thr = rec4<MR_THRESH>(&cm), lim = rec4<MR_IMP>(&cm);
      real dj = rdlane(du, 15 + j);
      real sum = lam_p[j] + (rhs - dj * di);
      sum = med3_(sum, -lim, lim);
      real dl = sum - lam_p[j]; lam_p[j] = sum;
      if (CHECK) busy |= __ballot(absr(dl) > thr);
      du += mw.w[j] * (armlane ? tot_a : dl);
    }
    // one exact 3x3 Gauss-Seidel block per contact.  The body is instantiated twice so that the LDS-resident contacts
    // (c < CL) compile to ds_read with immediate offsets and only the rare spilled ones (c >= CL) use global loads; a
    // single loop over "LDS or global" pointers degrades every access to flat_load + vmcnt(0)/lgkmcnt(0) waits.
    // Whole record (8 x 16 B) + the three response-row entries of this lane are fetched in ONE batch, and for the
    // LDS-resident contacts the next contact's batch is issued before the current block computes (software pipelining):
    // piecemeal loads cost four serial LDS round trips per contact, which two waves per SIMD cannot hide.
    struct CRec { real4 q[8]; real w0, w1, w2; };
    auto fetch = [&](const real* R, const real* wr) __attribute__((always_inline)) -> CRec {
      CRec r;
#pragma unroll
      for (int i = 0; i < 8; i++) r.q[i] = reinterpret_cast<const real4*>(R)[i];
      r.w0 = wr[dw]; r.w1 = wr[WPS + dw]; r.w2 = wr[2 * WPS + dw];
      return r;
    };
    auto block = [&](int c, unsigned sgw, const CRec& r, real* R, bool in_lds) __attribute__((always_inline)) {
      // (the angular rows of the attach weld -- at most one such contact, scripted mode only, index ang_c -- take the DOF's axis
      //  itself as Jacobian column instead of axis x lever arm: one scalar compare per contact)
      // (the record's words by name, rec4<CR_*>: pih_common.h; CR_LB = 0 / -BIG and CR_FLOOR = 0 / +BIG make the attach rows bilateral
      //  without a select)
      const real4* const q = r.q;
      const real w0 = r.w0, w1 = r.w1, w2 = r.w2;
      const V3 pr = mk(rec4<CR_P>(q) - g.o.x, rec4<CR_P + 1>(q) - g.o.y, rec4<CR_P + 2>(q) - g.o.z);
      const real mu = rec4<CR_MU>(q);
      const real sdu = (real)(int)__builtin_amdgcn_sbfe(sgw, 2u * (unsigned)(c & 15), 2u) * du;
      V3 cv = mk(__builtin_fmaf(ae.y, pr.z, __builtin_fmaf(-ae.z, pr.y, mp.x)), __builtin_fmaf(ae.z, pr.x, __builtin_fmaf(-ae.x, pr.z, mp.y)), __builtin_fmaf(ae.x, pr.y, __builtin_fmaf(-ae.y, pr.x, mp.z)));
      if (__builtin_expect(c == ang_cs, 0)) cv = ae;
      real jd0 = sdu * dot(rec4v<CR_DIR0>(q), cv), jd1 = sdu * dot(rec4v<CR_DIR0 + CR_KSTRIDE>(q), cv), jd2 = sdu * dot(rec4v<CR_DIR0 + CR_KSTRIDE * 2>(q), cv);
      // materialise the products: otherwise fast-math folds the multiply into the first reduction step as mul + mov_dpp + fmac
      // (3 instructions per value) instead of mul + v_add_f32_dpp (2)
      __asm__ volatile("" : "+v"(jd0), "+v"(jd1), "+v"(jd2));
      row16_sum3(jd0, jd1, jd2);
      rows012_total3(jd0, jd1, jd2);          // valid in lanes 32..47 from here; the scalar chain below runs in plain VGPRs
      const real l0 = rec4<CR_LAM>(q), l1 = rec4<CR_LAM + 1>(q), l2 = rec4<CR_LAM + 2>(q);
      const real di0 = rec4<CR_DINV0>(q), di1 = rec4<CR_DINV0 + CR_KSTRIDE>(q), di2 = rec4<CR_DINV0 + CR_KSTRIDE * 2>(q);
      real s0 = l0 + (rec4<CR_RHS>(q) - jd0 * di0);
      s0 = max_(s0, rec4<CR_LB>(q));
      real dl0 = s0 - l0;
      if (CHECK) busy |= __ballot(absr(dl0) > rec4<CR_THRESH>(q));
      real dl1 = 0, dl2 = 0, s1 = l1, s2 = l2;
      if (rdlane(s0, 32) > 0 || rdlane(mu, 32) < 0) {   // wave-uniform branch (Bullet skips the friction rows of an unloaded contact)
        real hi = max_(mu * s0, rec4<CR_FLOOR>(q));
        jd1 += rec4<CR_G>(q) * dl0;
        s1 = l1 + (rec4<CR_RHS + 1>(q) - jd1 * di1); s1 = med3_(s1, -hi, hi); dl1 = s1 - l1;
        if (CHECK) busy |= __ballot(absr(dl1) > rec4<CR_THRESH + 1>(q));
        jd2 += rec4<CR_G + 1>(q) * dl0 + rec4<CR_G + 2>(q) * dl1;
        s2 = l2 + (rec4<CR_RHS + 2>(q) - jd2 * di2); s2 = med3_(s2, -hi, hi); dl2 = s2 - l2;
        if (CHECK) busy |= __ballot(absr(dl2) > rec4<CR_THRESH + 2>(q));
      }
      if (d == 32) { R[CR_LAM] = s0; R[CR_LAM + 1] = s1; R[CR_LAM + 2] = s2; }
      if (!in_lds) __threadfence_block();     // spilled records live in global memory: make lane 32's store visible to the wave
      du += w0 * rdlane(dl0, 32) + w1 * rdlane(dl1, 32) + w2 * rdlane(dl2, 32);
    };
    const int ncl = nc < CL ? nc : CL;
    if (ncl > 0) {
      // two-deep ping-pong (ra / rb) instead of "cur = nxt": the rotation of a 27-register record costs 27 v_mov per contact
      CRec ra = fetch(sh.b.crec[0], &sh.b.Wp[0][0]);
      int c = 0;
      for (;;) {
        const int c1 = c + 1 < ncl ? c + 1 : c;
        CRec rb = fetch(sh.b.crec[c1], &sh.b.Wp[3 * c1][0]);
        block(c, c < 16 ? sg0 : sg1, ra, sh.b.crec[c], true);
        if (++c >= ncl) break;
        const int c2 = c + 1 < ncl ? c + 1 : c;
        ra = fetch(sh.b.crec[c2], &sh.b.Wp[3 * c2][0]);
        block(c, c < 16 ? sg0 : sg1, rb, sh.b.crec[c], true);
        if (++c >= ncl) break;
      }
    }
    if (nc > CL) {
      // the spilled contacts (global scratch) with the same one-ahead ping-pong: an env that gets here is one of the heaviest of
      // the launch, i.e. the one the launch ends up waiting for, and an unprefetched global load per contact is its latency
      auto row_of = [&](int c) { return ov.base + (size_t)(3 * (c - CL)) * WPS; };
      CRec ra = fetch(crec_spilled(ov, CL), row_of(CL));
      int c = CL;
      for (;;) {
        const int c1 = c + 1 < nc ? c + 1 : c;
        CRec rb = fetch(crec_spilled(ov, c1), row_of(c1));
        block(c, c < 32 ? sg1 : sg2, ra, crec_spilled(ov, c), false);
        if (++c >= nc) break;
        const int c2 = c + 1 < nc ? c + 1 : c;
        ra = fetch(crec_spilled(ov, c2), row_of(c2));
        block(c, c < 32 ? sg1 : sg2, rb, crec_spilled(ov, c), false);
        if (++c >= nc) break;
      }
    }
    return CHECK && !((busy >> 32) & 1ull);
  };
  const int it = pgs_iteration_loop(P.iters, P.checkstride, [&]() __attribute__((always_inline)) { return iterate(std::true_type{}); }, [&]() __attribute__((always_inline)) { return iterate(std::false_type{}); });
  w.sync();
  if (d < nc) { const real* R = crec_of(sh, ov, d); sh.r_lam[3 * d] = R[CR_LAM]; sh.r_lam[3 * d + 1] = R[CR_LAM + 1]; sh.r_lam[3 * d + 2] = R[CR_LAM + 2]; }
  if (d < ND) sh.u[d] += du;
  w.sync();
  return it;
}

}  // namespace pih
