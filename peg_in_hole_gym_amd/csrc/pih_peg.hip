// pih_peg.hip -- the kernels of the peg-in-hole task: dispatch-order sort and controller, the step, reset, stand-alone IK, wrist camera,
// grasp labels, state gather.  gfx950 only; one wavefront (64 threads, one workgroup) per env; per-env scratch in LDS (struct pih::Shared).
// The C ABI (pih_hip.hip) reaches them through the launch functions at the end (pih_launch.h).
// Why these kernels share a translation unit: a kernel's code can depend on its companions, and tools/isa_fingerprint.py is to show every
// kernel as it was when all of them lived in pih_hip.hip.  In this composition all do; pih_render_kernel alone in a translation unit does
// not (profiles/kernel_tu_split_fingerprint.txt).
#include <hip/hip_runtime.h>
#include <cstring>
#include "pih_device.h"
#include "pih_render.h"
#include "pih_fly_render.h"      // the tile walk of every camera kernel (fly::render_strip)
#include "pih_launch.h"

using namespace pih;

// ------------------------------------------------------------------------------------------------ kernels
// state: float[n][256] (env-major records: the 64 lanes of the env's wave read/write consecutive words, so every
// access is a fully coalesced 256 B segment).
// Longest-job-first dispatch order.  The cost of an env-step grows ~linearly with its contact count (each contact is one
// 3x3 PGS block per iteration), and at 4096 envs there are only two rounds of resident waves, so a heavy env that starts
// late leaves most of the chip idle at the tail.  This single-workgroup counting sort orders the envs by the contact count
// of their PREVIOUS step (descending); pih_step_kernel maps blockIdx through it.  Results do not depend on block order.
constexpr int PRE_THREADS = 256;
// the dispatch-order bin of an env with `ncontact` contacts in its previous step, of 64: bin 0 = most contacts (63 and more)
__device__ __forceinline__ int contact_bin(float ncontact) {
  const int k = (int)ncontact;
  return 63 - (k < 0 ? 0 : (k > 63 ? 63 : k));
}
__device__ __forceinline__ void pre_sort_block(float* __restrict__ state, int* __restrict__ order, int n) {
  const int t = threadIdx.x;
  if (!order) return;
  __shared__ int hist[64], base[64];
  if (t < 64) hist[t] = 0;
  __syncthreads();
  for (int e = t; e < n; e += PRE_THREADS) {
    atomicAdd(&hist[contact_bin(state[(size_t)e * PIH_STATE_WORDS + PIH_S_NCONTACT])], 1);
  }
  __syncthreads();
  if (t == 0) { int acc = 0; for (int b = 0; b < 64; b++) { base[b] = acc; acc += hist[b]; } }
  __syncthreads();
  for (int e = t; e < n; e += PRE_THREADS) {
    const int r = atomicAdd(&base[contact_bin(state[(size_t)e * PIH_STATE_WORDS + PIH_S_NCONTACT])], 1);
    order[r] = e;
  }
}

// Launch 1 of the two-launch step of rounds 1-3, kept as the reference of the fused launch (pih_config.schedule + 8; the only step a
// hipGraph can capture).  Block 0: the dispatch order above.  Blocks 1..: the controller (action / state machine -> IK -> joint targets)
// one env per LANE, 64 envs per block on the block's first wavefront (controller_targets: ik_chain).
__global__ void __launch_bounds__(PRE_THREADS) pih_pre_kernel(Params P, float* __restrict__ state, const float* __restrict__ actions,
                                                               int* __restrict__ order, int n) {
  const int t = threadIdx.x;
  if (blockIdx.x == 0) { pre_sort_block(state, order, n); return; }
  if (t >= 64) return;
  const int env = (blockIdx.x - 1) * 64 + t;
  if (env >= n) return;
  float* S = state + (size_t)env * PIH_STATE_WORDS;
  if (!P.autoreset && S[PIH_S_DONE] != 0) return;      // finished envs keep their last values (envs/base_env.py:62,66)
  float a[4] = {0, 0, 0, 0};
  if (actions) { a[0] = actions[env * 4]; a[1] = actions[env * 4 + 1]; a[2] = actions[env * 4 + 2]; a[3] = actions[env * 4 + 3]; }
  controller_targets(S, P, a);
}

// ---- the fused launch (round 4): ONE launch per step.
// Rounds 1-3 ran two launches per step: pih_pre_kernel (dispatch-order sort + controller, 33 us of which ~10 us are the gap between two
// dependent launches, on 64 of the chip's 1 024 SIMDs) and then pih_step_kernel (313 us at 4 096 envs).  Here the step kernel's grid is
// G = ceil(n / 64) CONTROLLER wavefronts (blocks 0 .. G - 1, dispatched first) followed by the n env wavefronts:
//   * a controller wavefront runs controller_compute for 64 envs, one per lane, from the envs' state records as the previous launch left
//     them, writes each env's 13 controller words into its mailbox record and publishes the group with the launch's epoch
//     (pih_mailbox.h); it never waits for anything;
//   * an env wavefront does forward kinematics, collision detection and the articulated-body sweep (~22 us), then waits -- bounded,
//     s_sleep between polls -- for its group's flag and takes the controller words from the mailbox (Wave::await_controller); the
//     controller needs ~25 us, so the first round of env waves waits a few us and the second round not at all;
//   * the dispatch order for the NEXT launch is built by the env wavefronts themselves: at its end an env takes a slot in the bin of its
//     contact count (atomicAdd; bin 0 = most contacts) of the "next" bin buffer; at its start block b finds "its" env by a prefix sum
//     over the 64 bin counts of the "current" buffer.  Three buffers rotate (current / next / being zeroed), so no launch ever reads a
//     count another wave of the same launch is still changing.  Results do not depend on the order (tests/test_gpu_api.py).
struct FusedArgs {
  int G, n, epoch;               // G = 0: two-launch path (no controller role, no mailbox)
  const int* bcur; int* bnext; int* bzero;   // bin buffers: [64 counts][64 x n slots]; nullptr: block b = env b (schedule 0) or `order`
  float* mail; int* flags; int* err;
};
__device__ __forceinline__ int fused_lookup_env(const int* __restrict__ bcur, int b, int n, int lane) {
  int p = bcur[lane];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(p, d); if (lane >= d) p += t; }
  const unsigned long long m = __ballot(p > b);
  if (m == 0) return b;                                      // (inconsistent bins cannot happen; stay in range if they do)
  const int k = __ffsll((long long)m) - 1;
  const int base = k > 0 ? __shfl(p, k - 1) : 0;
  const int e = bcur[64 + (size_t)k * n + (b - base)];
  return e >= 0 && e < n ? e : b;
}

__global__ void __launch_bounds__(64, 2) pih_step_kernel(Params P, float* __restrict__ state, const float* __restrict__ actions,
                                                      float* __restrict__ obs, float* __restrict__ reward,
                                                      unsigned char* __restrict__ done, float* __restrict__ dbg,
                                                      float* __restrict__ ovf, const int* __restrict__ order, FusedArgs F) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x < F.G) {
    // ---- controller role: 64 envs, one per lane (controller_compute: the strictly sequential IK)
    __builtin_amdgcn_s_setprio(3);                             // it shares its SIMD with an env wavefront that will be waiting for it
    if (blockIdx.x == 0 && F.bzero) F.bzero[lane] = 0;
    const int env = blockIdx.x * 64 + lane;
    if (env < F.n) {
      const float* S = state + (size_t)env * PIH_STATE_WORDS;
      if (P.autoreset || S[PIH_S_DONE] == 0) {               // finished envs keep their last values (envs/base_env.py:62,66): their waves do not read the mailbox
        float a[4] = {0, 0, 0, 0};
        if (actions) { a[0] = actions[env * 4]; a[1] = actions[env * 4 + 1]; a[2] = actions[env * 4 + 2]; a[3] = actions[env * 4 + 3]; }
        const CtrlOut o = controller_compute(S, P, a);
        float* m = F.mail + (size_t)env * CTRL_WORDS;
        const float ov[13] = {o.target[0], o.target[1], o.target[2], o.target[3], o.target[4], o.target[5], o.target[6], o.target[7], o.target[8], o.fsm, o.fsmt, o.grasp_angle, o.attach_qz};
#pragma unroll
        for (int i = 0; i < 13; i++) mail_store(m + i, ov[i]);
      }
    }
    mailbox_publish(F.flags, F.epoch);
    return;
  }
  __shared__ Shared sh;
  const int b = blockIdx.x - F.G;
  const int env = __builtin_amdgcn_readfirstlane(F.bcur ? fused_lookup_env(F.bcur, b, F.n, lane) : (order ? order[b] : b));   // (wave-uniform by construction; the scalar makes it so for the compiler)
  Wave w; w.l = lane; w.counter = 0;
  float* rec = state + (size_t)env * PIH_STATE_WORDS;
#pragma unroll
  for (int i = 0; i < PIH_STATE_WORDS / 64; i++) sh.S[lane + 64 * i] = rec[lane + 64 * i];
  __syncthreads();
  float o[5], r; unsigned char d;
  Ovf ov; ov.base = ovf + (size_t)env * OVF_WORDS;
  w.dbg = dbg ? dbg + (size_t)env * PIH_DEBUG_WORDS : nullptr; w.dbgmode = P.debug; w.prio_on = !P.noprio;
  if (F.G > 0) { w.cflags = F.flags; w.cmail = F.mail; w.cerr = F.err; w.cepoch = F.epoch; w.cenv = env; }
  step_env(w, sh, P, ov, env, nullptr, o, &r, &d, dbg ? dbg + (size_t)env * PIH_DEBUG_WORDS : nullptr);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PIH_STATE_WORDS / 64; i++) rec[lane + 64 * i] = sh.S[lane + 64 * i];
  if (lane < 5 && obs) obs[env * 5 + lane] = o[0] * (lane == 0) + o[1] * (lane == 1) + o[2] * (lane == 2) + o[3] * (lane == 3) + o[4] * (lane == 4);
  if (lane == 0) {
    if (reward) reward[env] = r; if (done) done[env] = d;
    if (F.bnext) {                                           // a slot in the next launch's dispatch order
      const int bin = contact_bin(sh.S[PIH_S_NCONTACT]);
      const int rnk = atomicAdd(F.bnext + bin, 1);
      if (rnk < F.n) F.bnext[64 + (size_t)bin * F.n + rnk] = env;
    }
  }
}

// first fill of a bin buffer (pih_create): the same counting sort, from the state records
__global__ void __launch_bounds__(256) pih_bins_init_kernel(const float* __restrict__ state, int* __restrict__ bins, int n) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int bin = contact_bin(state[(size_t)e * PIH_STATE_WORDS + PIH_S_NCONTACT]);
    const int rnk = atomicAdd(bins + bin, 1);
    bins[64 + (size_t)bin * n + rnk] = e;
  }
}

// hard (resetSimulation, envs/base_env.py:85-86): a NEW scene like every reset (the reference keeps drawing from the global `random`); it
// also clears the non-finite-reset count.  rewind (explicit replay, pih_reset(seed != 0) / pih_reseed): the env's draw counter restarts.
__global__ void __launch_bounds__(64) pih_reset_kernel(Params P, float* __restrict__ state, const unsigned char* __restrict__ mask, int hard, int rewind) {
  __shared__ Shared sh;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (mask && !mask[env]) return;
  Wave w; w.l = lane; w.counter = 0;
  float* rec = state + (size_t)env * PIH_STATE_WORDS;
  for (int i = 0; i < PIH_STATE_WORDS / 64; i++) sh.S[lane + 64 * i] = rec[lane + 64 * i];
  __syncthreads();
  if (hard) sh.S[PIH_S_SPARE] = 0;
  if (rewind) { sh.S[PIH_S_RNG] = 0; sh.S[PIH_S_RNG_HI] = 0; }
  __syncthreads();
  reset_state(sh.S, P, P.env0 + env);
  __syncthreads();
  fk_all(w, sh);
  float tip[7]; tip_pose(sh, tip);
  for (int i = 0; i < 7; i++) sh.S[PIH_S_TIP + i] = tip[i];
  V3 ee; M3 eR; ee_pose(sh, ee, eR);
  sh.S[PIH_S_EE] = ee.x + sh.S[PIH_S_OFFSET]; sh.S[PIH_S_EE + 1] = ee.y + sh.S[PIH_S_OFFSET + 1]; sh.S[PIH_S_EE + 2] = ee.z + sh.S[PIH_S_OFFSET + 2];
  __syncthreads();
  for (int i = 0; i < PIH_STATE_WORDS / 64; i++) rec[lane + 64 * i] = sh.S[lane + 64 * i];
}

__global__ void __launch_bounds__(64) pih_init_offsets_kernel(float* __restrict__ state, const float* __restrict__ offsets, int n) {
  int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n) return;
  float* rec = state + (size_t)e * PIH_STATE_WORDS;
  for (int k = 0; k < 3; k++) rec[PIH_S_OFFSET + k] = offsets ? offsets[3 * e + k] : 0.f;
}

// stand-alone batched IK (envs/utils.py:67,79): one problem per QUAD of lanes (pih_ikq.h), 16 problems per wavefront
template <class C> __device__ __forceinline__ void ik_quad_problem(const Params& P, int n, int stride, const float* q0, const float* tpos, const float* tquat, float* qout) {
  const int i = blockIdx.x * 16 + (threadIdx.x >> 2);
  if (i >= n) return;
  QuadDpp qd; qd.l = threadIdx.x & 3;
  const int j0 = 2 * qd.l, j1 = 2 * qd.l + 1;
  const QuadSlots sl = ikq_slots<C>(qd);
  float a = j0 < C::N ? q0[i * stride + j0] : 0.0f, b = j1 < C::N ? q0[i * stride + j1] : 0.0f;
  Q4 tq; tq.x = tquat[4 * i]; tq.y = tquat[4 * i + 1]; tq.z = tquat[4 * i + 2]; tq.w = tquat[4 * i + 3];
  ikq_solve(qd, sl, P, mk(tpos[3 * i], tpos[3 * i + 1], tpos[3 * i + 2]), tq, a, b);
  if (j0 < C::N) qout[i * stride + j0] = a;
  if (j1 < C::N) qout[i * stride + j1] = b;
  for (int k = C::N + qd.l; k < stride; k += 4) qout[i * stride + k] = q0[i * stride + k];      // (Panda: the finger entries pass through)
}
__global__ void __launch_bounds__(64) pih_ik_kernel(Params P, int n, const float* __restrict__ q0, const float* __restrict__ tpos,
                                                    const float* __restrict__ tquat, float* __restrict__ qout) {
  ik_quad_problem<PandaChain>(P, n, 9, q0, tpos, tquat, qout);
}
// the same for the UR5 chain (envs/utils.py:79): q0 float[n,6] -> qout float[n,6]
__global__ void __launch_bounds__(64) pih_ik_ur5_kernel(Params P, int n, const float* __restrict__ q0, const float* __restrict__ tpos,
                                                        const float* __restrict__ tquat, float* __restrict__ qout) {
  ik_quad_problem<Ur5Chain>(P, n, 6, q0, tpos, tquat, qout);
}

// wrist camera (p12): grid = (strips, envs), 256 threads (4 waves); out float[count, H, W, 4] = depth, r, g, b.  The tile walk is the one
// of every camera kernel (fly::render_strip, pih_fly_render.h) on a grid with the wrist camera's constant tan(fov / 2).
__global__ void __launch_bounds__(RENDER_THREADS) pih_render_kernel(const float* __restrict__ state, float* __restrict__ out,
                                                                    int env_begin, int W, int H, int rows_per_strip, int flags) {
  __shared__ Shared sh;
  __shared__ Scene sc;
  const int tid = threadIdx.x, e = blockIdx.y, env = env_begin + e;
  const int r0 = blockIdx.x * rows_per_strip, r1 = min(H, r0 + rows_per_strip);
  Wave w; w.l = tid; w.counter = 0;
  const float* rec = state + (size_t)env * PIH_STATE_WORDS;
  for (int i = tid; i < PIH_STATE_WORDS; i += RENDER_THREADS) sh.S[i] = rec[i];
  __syncthreads();
  scene_setup(w, sh, sc, tid);
  static_assert(fly::TILE_ROWS == 16 && fly::TILE_COLS == 64, "the tile of pih_render.h's mapping: 16 rows x 64 columns, one row of a tile per wave instruction");
  fly::render_strip<unsigned>(sc, fly::FlyGrid(PIH_CAM_TANH2, PIH_CAM_TANH2, W, H), reinterpret_cast<float4*>(out), (size_t)e * H, W, r0, r1, tid,
                              [&](unsigned prims, real xc, real yc) { return fly::to_float4(shade(sc, prims, xc, yc, flags)); });
}

// label images: grid = (ceil(S*S/256), envs); out[e][k][y][x], image index [cc][rr] of the reference = [x-like c][r]
__global__ void __launch_bounds__(256) pih_labels_kernel(const float* __restrict__ state, float* __restrict__ out, float* __restrict__ meta,
                                                         int env_begin, int S) {
  const int e = blockIdx.y, env = env_begin + e;
  const float angle = state[(size_t)env * PIH_STATE_WORDS + PIH_S_GRASP_ANGLE];
  const LabelRect L = label_rect(angle, S);
  // each thread owns 4 consecutive pixels and writes one 16-byte store per label plane (the kernel is pure HBM writes)
  const int SS = S * S, i4 = (blockIdx.x * 256 + threadIdx.x) * 4;
  float* o = out + (size_t)e * 4 * SS;
  if (i4 < SS) {
    float v[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int idx = i4 + k < SS ? i4 + k : SS - 1;
      const int c = idx / S, r = idx - c * S;            // element [c][r] of the image
      const bool in = label_inside(L, (float)c, (float)r);
      v[0][k] = in ? 50.0f : 0.0f; v[1][k] = in ? L.s2 : 0.0f; v[2][k] = in ? L.c2 : 1.0f; v[3][k] = in ? L.wpx : 0.0f;
    }
    const bool vec = (i4 + 3 < SS) && ((SS & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
#pragma unroll
    for (int pl = 0; pl < 4; pl++) {
      if (vec) *reinterpret_cast<float4*>(o + (size_t)pl * SS + i4) = make_float4(v[pl][0], v[pl][1], v[pl][2], v[pl][3]);
      else for (int k = 0; k < 4 && i4 + k < SS; k++) o[(size_t)pl * SS + i4 + k] = v[pl][k];
    }
  }
  if (meta && blockIdx.x == 0 && threadIdx.x == 0) {
    float* m = meta + (size_t)e * 5;
    m[0] = 0; m[1] = 0; m[2] = angle * (180.0f / 3.14159265358979f); m[3] = L.wpx; m[4] = L.lpx;
  }
}

__global__ void pih_gather_kernel(const float* __restrict__ state, float* __restrict__ out, int n, int word0, int nwords) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * nwords) return;
  int e = idx / nwords, k = idx - e * nwords;
  out[idx] = state[(size_t)e * PIH_STATE_WORDS + word0 + k];
}

// ------------------------------------------------------------------------------------------------ launches (pih_launch.h)
namespace pih {
size_t peg_mail_words(int n) { return (size_t)n * CTRL_WORDS; }
size_t peg_bin_ints(int n) { return 64 + (size_t)64 * n; }      // [64 counts][64 x n slots]

void peg_init_offsets_launch(hipStream_t stream, float* state, const float* offsets, int n) {
  hipLaunchKernelGGL(pih_init_offsets_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, state, offsets, n);
}
void peg_reset_launch(hipStream_t stream, const Params& P, float* state, const unsigned char* mask, int hard, int rewind, int n) {
  hipLaunchKernelGGL(pih_reset_kernel, dim3(n), dim3(64), 0, stream, P, state, mask, hard, rewind);
}
void peg_bins_init_launch(hipStream_t stream, const float* state, int* bins, int n) {
  hipLaunchKernelGGL(pih_bins_init_kernel, dim3(64), dim3(256), 0, stream, state, bins, n);
}
void peg_pre_launch(hipStream_t stream, const Params& P, float* state, const float* actions, int* order, int n) {
  hipLaunchKernelGGL(pih_pre_kernel, dim3(1 + (n + 63) / 64), dim3(PRE_THREADS), 0, stream, P, state, actions, order, n);
}
void peg_step_launch(hipStream_t stream, const Params& P, const StepIO& io, float* ovf, const int* order, int n) {
  FusedArgs F; memset(&F, 0, sizeof F);
  hipLaunchKernelGGL(pih_step_kernel, dim3(n), dim3(64), 0, stream, P, io.state, io.actions, io.obs, io.reward, io.done, io.dbg, ovf, order, F);
}
// one launch: controller wavefronts first, then the env wavefronts
void peg_step_fused_launch(hipStream_t stream, const Params& P, const StepIO& io, float* ovf, int n, const Mailbox& mb, const Bins& bins) {
  FusedArgs F; memset(&F, 0, sizeof F);
  F.G = (n + 63) / 64; F.n = n; F.epoch = mb.epoch; F.mail = mb.mail; F.flags = mb.flags; F.err = mb.err;
  F.bcur = bins.cur; F.bnext = bins.next; F.bzero = bins.zero;
  hipLaunchKernelGGL(pih_step_kernel, dim3(F.G + n), dim3(64), 0, stream, P, io.state, io.actions, io.obs, io.reward, io.done, io.dbg, ovf, (const int*)nullptr, F);
}
void peg_gather_launch(hipStream_t stream, const float* state, float* out, int n, int word0, int nwords) {
  hipLaunchKernelGGL(pih_gather_kernel, dim3((n * nwords + 255) / 256), dim3(256), 0, stream, state, out, n, word0, nwords);
}
void ik_launch(bool ur5, hipStream_t stream, const Params& P, int n, const float* q0, const float* tpos, const float* tquat, float* qout) {
  hipLaunchKernelGGL(ur5 ? pih_ik_ur5_kernel : pih_ik_kernel, dim3((n + 15) / 16), dim3(64), 0, stream, P, n, q0, tpos, tquat, qout);
}
void render_launch(dim3 grid, hipStream_t stream, const float* state, float* out, int env_begin, int W, int H, int rows_per_strip, int flags) {
  hipLaunchKernelGGL(pih_render_kernel, grid, dim3(RENDER_THREADS), 0, stream, state, out, env_begin, W, H, rows_per_strip, flags);
}
void labels_launch(hipStream_t stream, const float* state, float* out, float* meta, int env_begin, int env_count, int S) {
  hipLaunchKernelGGL(pih_labels_kernel, dim3((S * S + 1023) / 1024, env_count), dim3(256), 0, stream, state, out, meta, env_begin, S);
}
}  // namespace pih
