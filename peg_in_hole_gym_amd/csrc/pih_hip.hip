// pih_hip.hip -- kernels + C ABI (include/pih.h) of the MI355X-native peg-in-hole environment.
// gfx950 only; one wavefront (64 threads, one workgroup) per env; per-env scratch in LDS (struct pih::Shared).
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o libpih_hip.so pih_hip.hip   (see build.py)
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pih_device.h"
#include "pih_render.h"
#include "pih_fly.h"
#include "pih_fly_render.h"

using namespace pih;

// pih_fly_image.hip: the kernels of the packed output formats and of the per-env cameras in device memory
namespace pih {
void fly_image_launch(int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                      int n, int object, int env_begin, int W, int H, int rows_per_strip, int flags);
// pih_view.hip: the free camera of the peg-in-hole task
void view_launch(int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                 int env_begin, int W, int H, int rows_per_strip, int flags);
// pih_lit.hip: both cameras under a caller-given light, with a specular term and cast shadows
int lit_light_check(const float* words, const char** what);
void lit_launch(bool fly_task, int fmt, dim3 grid, hipStream_t stream, const float* state, void* out, const fly::FlyCam& cam, const float* cam_dev,
                const float* light, const float* light_dev, int n, int object, int env_begin, int W, int H, int rows_per_strip, int flags);
// pih_robot.hip: the batched robot-model queries of include/pih_robot.h
void robot_fk_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, const float* qd, float* out);
void robot_jacobian_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, int frame, const float* local_pos, float* out);
void robot_mass_launch(int robot, bool staged, hipStream_t stream, int n, const float* q, float* out);
void robot_invdyn_launch(int robot, hipStream_t stream, int n, const float* q, const float* qd, const float* qdd, float* tau);
void link_states_launch(bool fly_task, hipStream_t stream, const float* state, float* out, int n_envs, int env_begin, int env_count);
int robot_dims(int robot, int* ndof, int* nframes);
int link_states_frames(int task_id);
}

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

// free camera of the random-fly task (pih_fly_render.h): grid = (strips, envs), 256 threads (4 waves); out float[count, H, W, 4] = depth,
// r, g, b.  state is structure-of-arrays: the 13 words the scene needs are wave-uniform (scalar) loads (load_fly_pose).  One host camera,
// validated by pih_render_cam: no camera test here (pih_fly_image_kernel has it); the tile walk is render_strip.
__global__ void __launch_bounds__(RENDER_THREADS) pih_fly_render_kernel(const float* __restrict__ state, float* __restrict__ out, fly::FlyCam cam,
                                                                        int n, int object, int env_begin, int W, int H, int rows_per_strip, int flags) {
  using namespace fly;
  __shared__ FlyScene sc;
  const int tid = threadIdx.x, e = blockIdx.y, env = env_begin + e;
  const int r0 = blockIdx.x * rows_per_strip, r1 = min(H, r0 + rows_per_strip);
  if (tid < 16) scene_setup_poses(sc, load_fly_pose(state, env, n), cam, object, flags, tid);
  __syncthreads();
  scene_setup_bounds(sc, object, tid);
  __syncthreads();
  render_strip<unsigned>(sc, FlyGrid(sc, W, H), reinterpret_cast<float4*>(out), (size_t)e * H, W, r0, r1, tid,
                         [&](unsigned prims, real xc, real yc) { return to_float4(shade(sc, prims, xc, yc, flags)); });
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

// ------------------------------------------------------------------------------------------------ 'random-fly' task kernels
// One env per LANE or per QUAD of lanes (pih_fly.h).  state: float[PIH_FLY_STATE_WORDS][n] (structure-of-arrays: word w of the envs of a
// wave is one coalesced segment).  LDS: the per-lane contact rows, [word][lane]: 120 KB per wave in the lane layout (one wave per CU), 38 KB
// in the quad layout (four per CU; the kernel needs 450 registers, i.e. one wave per SIMD, anyway).
// (Round 3, profiles/r03_fly_envs_per_wave.txt: packing FEWER envs into a wave of the lane layout did not shorten the launch, and with 120 KB
//  of LDS per wave it cost rounds.  The quad layout does not idle the other lanes: it gives them a share of the PGS sweep.)
//
// The fused random-fly launch (round 4, as the peg-in-hole one): the first G = ceil(n / 64) blocks are CONTROLLER wavefronts (the IK of 64
// envs, one per lane, straight into a mailbox [group][word][lane], then the epoch into the block's flag), the following blocks the step
// wavefronts (ceil(n / 16) in the quad layout, G in the lane layout), whose lanes read their targets from the mailbox right before the PGS
// loop -- after forward kinematics, the articulated-body sweeps, collision detection and all response rows.  Every workgroup of the launch
// carries the step's dynamic LDS, and a step wavefront spins on its controller's flag, so the layout is used only while ALL workgroups are
// resident at once (pih_create: quad layout 4 per CU, lane layout 1 per CU); bigger batches run the IK inside the step wavefront
// (FUSED = false).
struct FlyFused { int G, epoch; float* mail; int* flags; int* err; };
struct MailboxIk {
  const int* flag; const float* mail; int* err; int epoch, env, n;
  __device__ __forceinline__ void operator()(const float*, const float*, const float*, const Params&, float* qs) const {
    mailbox_await(flag, epoch, err, true);
#pragma unroll
    for (int i = 0; i < fly::NJ; i++) qs[i] = mail_load(mail + ((size_t)(env >> 6) * fly::NJ + i) * 64 + (env & 63));
  }
};
// QUAD: one env per quad of lanes (pih_fly.h): a step wavefront holds 16 envs, the PGS sweep is split over the quad; the controller
// wavefronts stay one env per lane, so one flag covers four step wavefronts.
struct FlyWave {           // what fly::step_env asks of the wavefront, as scalars over its active lanes
  __device__ __forceinline__ int wave_or(int x) const {     // OR of a 6-bit mask
    int m = 0;
#pragma unroll
    for (int k = 0; k < fly::NJ; k++) if (__builtin_amdgcn_ballot_w64((x >> k) & 1) != 0) m |= 1 << k;
    return __builtin_amdgcn_readfirstlane(m);
  }
  __device__ __forceinline__ bool wave_any(bool x) const { return __builtin_amdgcn_ballot_w64(x) != 0; }
};
struct FlyLane : FlyWave { static constexpr bool QUAD = false; __device__ __forceinline__ explicit FlyLane(int) {} };
struct FlyQuad : QuadDpp, FlyWave {
  static constexpr bool QUAD = true;
  __device__ __forceinline__ explicit FlyQuad(int lane) { l = lane & 3; }
  __device__ __forceinline__ int wave_max(int x) const {     // the largest x (0 <= x <= fly::NC)
    int m = 0;
#pragma unroll
    for (int k = 1; k <= fly::NC; k++) if (__builtin_amdgcn_ballot_w64(x >= k) != 0) m = k;
    return __builtin_amdgcn_readfirstlane(m);
  }
};
template <bool FUSED, bool QUAD>
__global__ void __launch_bounds__(64, 1) pih_fly_step_kernel(Params P, float* __restrict__ state, const float* __restrict__ actions,
                                                             float* __restrict__ obs, float* __restrict__ reward,
                                                             unsigned char* __restrict__ done, float* __restrict__ dbg, int n, FlyFused F) {
  extern __shared__ float lanemem[];
  if (FUSED && (int)blockIdx.x < F.G) {
    // ---- controller role
    __builtin_amdgcn_s_setprio(3);
    const int env = blockIdx.x * 64 + threadIdx.x;
    if (env < n && (P.autoreset || state[(size_t)PIH_F_DONE * n + env] == 0)) {
      float q[fly::NJ], S3[PIH_F_OFFSET + 3], a[PIH_FLY_ACTION_DIM], qs[fly::NJ];
#pragma unroll
      for (int i = 0; i < fly::NJ; i++) q[i] = state[(size_t)(PIH_F_Q + i) * n + env];
#pragma unroll
      for (int k = 0; k < 3; k++) S3[PIH_F_OFFSET + k] = state[(size_t)(PIH_F_OFFSET + k) * n + env];
#pragma unroll
      for (int k = 0; k < PIH_FLY_ACTION_DIM; k++) a[k] = actions[(size_t)env * PIH_FLY_ACTION_DIM + k];
      fly::InlineIk()(q, S3, a, P, qs);
#pragma unroll
      for (int i = 0; i < fly::NJ; i++) mail_store(F.mail + ((size_t)blockIdx.x * fly::NJ + i) * 64 + threadIdx.x, qs[i]);
    }
    mailbox_publish(F.flags, F.epoch);
    return;
  }
  const int blk = FUSED ? blockIdx.x - F.G : blockIdx.x;
  const int env = QUAD ? blk * 16 + (int)(threadIdx.x >> 2) : blk * 64 + (int)threadIdx.x;
  if (env >= n) return;
  const bool writer = !QUAD || (threadIdx.x & 3) == 0;      // (the four lanes of a quad hold identical results)
  // config.debug = 2: start / end of the wavefront on the chip-wide 100 MHz clock and where it ran (debug words PIH_DBG_T_START .. of the
  // wave's first env; tools/fly_trace.py) -- never read by the kernel
  const bool stamp = dbg && P.debug == 2 && threadIdx.x == 0;
  long long ts0 = 0;
  if (stamp) ts0 = (long long)__builtin_amdgcn_s_memrealtime();
  float S[fly::SW];
#pragma unroll
  for (int w = 0; w < fly::SW; w++) S[w] = state[(size_t)w * n + env];
  float a[PIH_FLY_ACTION_DIM] = {0, 0, 0, 0, 0, 0};
  if (actions) {
#pragma unroll
    for (int k = 0; k < PIH_FLY_ACTION_DIM; k++) a[k] = actions[(size_t)env * PIH_FLY_ACTION_DIM + k];
  }
  float o[PIH_FLY_OBS_DIM], r; unsigned char d;
  fly::LaneMem mem; mem.p = lanemem + threadIdx.x; mem.stride = 64;
  float* dbge = dbg ? dbg + (size_t)env * PIH_DEBUG_WORDS : nullptr;
  // the IK targets from the controller wavefront's mailbox (FUSED) or computed here
  std::conditional_t<FUSED, MailboxIk, fly::InlineIk> ctl;
  if constexpr (FUSED) { ctl.flag = F.flags + (env >> 6); ctl.mail = F.mail; ctl.err = F.err; ctl.epoch = F.epoch; ctl.env = env; ctl.n = n; }
  fly::step_env(S, P, P.env0 + env, a, o, &r, &d, mem, dbge, ctl, std::conditional_t<QUAD, FlyQuad, FlyLane>((int)threadIdx.x));
  if (writer) {
#pragma unroll
    for (int w = 0; w < fly::SW; w++) state[(size_t)w * n + env] = S[w];
    if (obs) {
#pragma unroll
      for (int k = 0; k < PIH_FLY_OBS_DIM; k++) obs[(size_t)env * PIH_FLY_OBS_DIM + k] = o[k];
    }
    if (reward) reward[env] = r;
    if (done) done[env] = d;
  }
  if (stamp) {
    const long long ts1 = (long long)__builtin_amdgcn_s_memrealtime();
    float* o2 = dbg + (size_t)env * PIH_DEBUG_WORDS;
    debug_store_time(o2, PIH_DBG_T_START, ts0); debug_store_time(o2, PIH_DBG_T_END, ts1); debug_store_hw_id(o2);
  }
}

__global__ void __launch_bounds__(64) pih_fly_reset_kernel(Params P, float* __restrict__ state, const unsigned char* __restrict__ mask, int hard, int rewind, int n) {
  const int env = blockIdx.x * 64 + threadIdx.x;
  if (env >= n || (mask && !mask[env])) return;
  float S[fly::SW];
#pragma unroll
  for (int w = 0; w < fly::SW; w++) S[w] = state[(size_t)w * n + env];
  if (hard) S[PIH_F_SPARE] = 0;
  if (rewind) { S[PIH_F_RNG] = 0; S[PIH_F_RNG_HI] = 0; }
  fly::reset_state(S, P, P.env0 + env);
#pragma unroll
  for (int w = 0; w < fly::SW; w++) state[(size_t)w * n + env] = S[w];
}

// env-major float[n, W]  <->  structure-of-arrays float[W][n]
__global__ void pih_soa_to_aos_kernel(const float* __restrict__ soa, float* __restrict__ aos, int n, int W, int word0, int nwords) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * nwords) return;
  const int e = idx / nwords, k = idx - e * nwords;
  aos[idx] = soa[(size_t)(word0 + k) * n + e];
  (void)W;
}
__global__ void pih_aos_to_soa_kernel(const float* __restrict__ aos, float* __restrict__ soa, int n, int W) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * W) return;
  const int w = idx / n, e = idx - w * n;
  soa[idx] = aos[(size_t)e * W + w];
}
__global__ void pih_fly_init_offsets_kernel(float* __restrict__ state, const float* __restrict__ offsets, int n) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n) return;
  for (int k = 0; k < 3; k++) state[(size_t)(PIH_F_OFFSET + k) * n + e] = offsets ? offsets[3 * e + k] : 0.f;
}

// ------------------------------------------------------------------------------------------------ host side
// roctx ranges around the step / reset launches (tracing): only with pih_config.debug != 0, and through dlopen so
// that the library has no link-time dependency on the profiler SDK -- without the roctx library the ranges are silently absent.
struct Roctx {
  int (*push)(const char*) = nullptr; int (*pop)() = nullptr; bool tried = false;
  void load() {
    if (tried) return;
    tried = true;
    for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      void* l = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (!l) continue;
      push = reinterpret_cast<int (*)(const char*)>(dlsym(l, "roctxRangePushA")); pop = reinterpret_cast<int (*)()>(dlsym(l, "roctxRangePop"));
      if (push && pop) return;
      push = nullptr; pop = nullptr;
    }
  }
};
static Roctx g_roctx;
struct RoctxRange {      // RAII: pushes when tracing is on for this handle and the library was found
  bool on = false;
  RoctxRange(bool enabled, const char* name) { if (enabled) { g_roctx.load(); if (g_roctx.push) { g_roctx.push(name); on = true; } } }
  ~RoctxRange() { if (on) g_roctx.pop(); }
};
constexpr size_t EV_POOL = 1024;   // timing event triples kept before they are folded into the running sums
struct EvTriple { hipEvent_t a, b, c; };
struct pih_handle {
  pih_config cfg;
  Params P;
  int device = 0;
  bool fly = false;         // PIH_TASK_RANDOM_FLY: structure-of-arrays state, one env per lane
  bool rewind_pending = false;   // pih_reseed: the envs reset by the next pih_reset restart their draw sequence
  int words = PIH_STATE_WORDS;
  float* state = nullptr;
  float* dbg = nullptr;
  float* ovf = nullptr;     // spill area for contacts beyond the LDS-resident CL (rarely touched)
  int* order = nullptr;     // longest-job-first block -> env map (block 0 of pih_pre_kernel; two-launch path)
  // fused launch (default for the peg-in-hole task): controller mailbox + group flags + error word, three rotating bin buffers of the
  // in-kernel dispatch order, the launch counter
  bool fused = false, flyquad = false;     // flyquad: random-fly step wavefronts hold one env per quad of lanes
  float* mail = nullptr; int* flags = nullptr; int* errw = nullptr; volatile int* errw_host = nullptr; int* bins = nullptr; size_t bin_ints = 0; int epoch = 0;
  std::string err;
  int timing = 0;           // 0 off; k >= 1: every k-th step launch is bracketed by events (pih_set_timing)
  unsigned timing_tick = 0;
  std::vector<EvTriple> ev;   // (before pre-kernel, between, after step kernel) of each timed step launch
  size_t ev_used = 0;
  double acc_pre_ms = 0, acc_step_ms = 0; int64_t acc_n = 0;
};

static thread_local std::string g_err;
static const char* const CTRL_TIMEOUT_MSG = "pih_step: an env wavefront timed out waiting for its controller wavefront (fused launch); the results of that step are invalid";

static int fail(pih_handle* h, const char* what, hipError_t e) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  if (h) h->err = m;
  g_err = m;
  return -1;
}
#define HIPCHK(h, x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(h, #x, _e); } while (0)

// Every entry point runs on the handle's own device ("one handle per device, handles independent"): the caller's current
// device is switched for the duration of the call and restored afterwards.
struct DevGuard {
  int prev = -1; bool switched = false; hipError_t err = hipSuccess;
  explicit DevGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; }
  }
  ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define PIH_ENTER(h) DevGuard _guard((h)->device); if (_guard.err != hipSuccess) return fail(h, "select the handle's device", _guard.err)

// fold finished event triples into the running sums (called when the pool is full and by pih_timing)
static int drain_events(pih_handle* h) {
  for (size_t i = 0; i < h->ev_used; i++) {
    HIPCHK(h, hipEventSynchronize(h->ev[i].c));
    float m1 = 0, m2 = 0;
    HIPCHK(h, hipEventElapsedTime(&m1, h->ev[i].a, h->ev[i].b));
    HIPCHK(h, hipEventElapsedTime(&m2, h->ev[i].b, h->ev[i].c));
    h->acc_pre_ms += m1; h->acc_step_ms += m2; h->acc_n++;
  }
  h->ev_used = 0;
  return 0;
}

extern "C" {

void pih_default_config(pih_config* c) { config_defaults(c); }
int pih_abi_version(void) { return PIH_ABI_VERSION; }
int pih_task_dims(int task_id, int32_t out[3]) {
  if (!out) return -2;
  if (task_id == PIH_TASK_PEG_IN_HOLE) { out[0] = PIH_ACTION_DIM; out[1] = PIH_OBS_DIM; out[2] = PIH_STATE_WORDS; return 0; }
  if (task_id == PIH_TASK_RANDOM_FLY) { out[0] = PIH_FLY_ACTION_DIM; out[1] = PIH_FLY_OBS_DIM; out[2] = PIH_FLY_STATE_WORDS; return 0; }
  return -2;
}

const char* pih_object_name(int task_id, int object_id) {
  static const char* const names[PIH_FLY_NOBJ] = PIH_FLY_OBJ_NAMES;
  return task_id == PIH_TASK_RANDOM_FLY && object_id >= 0 && object_id < PIH_FLY_NOBJ ? names[object_id] : nullptr;
}

int pih_destroy(pih_handle* h) {
  if (!h) return 0;
  DevGuard guard(h->device);
  for (auto& p : h->ev) { hipEventDestroy(p.a); hipEventDestroy(p.b); hipEventDestroy(p.c); }
  if (h->state) hipFree(h->state);
  if (h->dbg) hipFree(h->dbg);
  if (h->ovf) hipFree(h->ovf);
  if (h->order) hipFree(h->order);
  if (h->mail) hipFree(h->mail);
  if (h->flags) hipFree(h->flags);
  if (h->errw_host) hipHostFree(const_cast<int*>(h->errw_host));
  if (h->bins) hipFree(h->bins);
  delete h;
  return 0;
}

// Fused launch, both tasks (pih_mailbox.h): a zeroed mailbox of `mail_words` floats, one flag per group of 64 envs, and the error word.
// The error word lives in pinned, device-mapped HOST memory: an env wavefront that gives up waiting stores 1 there (system scope), and the
// next pih_step / pih_timing2 on the handle sees it without synchronising anything.
static int mailbox_alloc(pih_handle* h, size_t mail_words) {
  const size_t G = ((size_t)h->cfg.n_envs + 63) / 64;
  HIPCHK(h, hipMalloc(&h->mail, mail_words * sizeof(float)));
  HIPCHK(h, hipMemset(h->mail, 0, mail_words * sizeof(float)));
  HIPCHK(h, hipMalloc(&h->flags, G * sizeof(int)));
  HIPCHK(h, hipMemset(h->flags, 0, G * sizeof(int)));
  HIPCHK(h, hipHostMalloc((void**)&h->errw_host, sizeof(int), hipHostMallocMapped));
  *h->errw_host = 0;
  HIPCHK(h, hipHostGetDevicePointer((void**)&h->errw, const_cast<int*>(h->errw_host), 0));
  return 0;
}
// the epoch of the next fused launch, or -5 once an env wavefront of an EARLIER launch of this handle timed out (from then on every step
// fails loudly)
static int next_epoch(pih_handle* h) {
  if (*h->errw_host) { h->err = CTRL_TIMEOUT_MSG; return -5; }
  return ++h->epoch;
}

// The random-fly step launch of a handle in its layout (h->flyquad), fused or not: the instantiation of pih_fly_step_kernel, the grid (G
// controller workgroups in front of the step workgroups when fused), the dynamic LDS of every workgroup, and how many of them a CU holds
struct FlyLaunch { decltype(&pih_fly_step_kernel<false, false>) kernel; int G, grid, per_cu; size_t lds; };
static_assert((size_t)fly::LANE_WORDS * 64 * sizeof(float) <= 160 * 1024 && (size_t)fly::LANE_WORDS_Q * 64 * sizeof(float) * 4 <= 160 * 1024, "the random-fly kernel's per-wave LDS exceeds its share of a CU's 160 KB");
static FlyLaunch fly_launch(const pih_handle* h, bool fused) {
  const int n = h->cfg.n_envs;
  FlyLaunch L;
  L.G = (n + 63) / 64;
  if (h->flyquad) { L.kernel = fused ? pih_fly_step_kernel<true, true> : pih_fly_step_kernel<false, true>; L.grid = (n + 15) / 16; L.per_cu = 4; L.lds = (size_t)fly::LANE_WORDS_Q * 64 * sizeof(float); }
  else { L.kernel = fused ? pih_fly_step_kernel<true, false> : pih_fly_step_kernel<false, false>; L.grid = L.G; L.per_cu = 1; L.lds = (size_t)fly::LANE_WORDS * 64 * sizeof(float); }
  if (fused) L.grid += L.G;
  return L;
}

// allocation + first reset; on any failure the caller (pih_create) destroys the half-built handle
static int create_impl(pih_handle* h, const float* offsets_host, float** offd) {
  const pih_config* cfg = &h->cfg;
  size_t nb = (size_t)cfg->n_envs * h->words * sizeof(float);
  HIPCHK(h, hipMalloc(&h->state, nb));
  HIPCHK(h, hipMemset(h->state, 0, nb));
  if (cfg->debug) { HIPCHK(h, hipMalloc(&h->dbg, (size_t)cfg->n_envs * PIH_DEBUG_WORDS * sizeof(float))); HIPCHK(h, hipMemset(h->dbg, 0, (size_t)cfg->n_envs * PIH_DEBUG_WORDS * sizeof(float))); }
  if (offsets_host) {
    HIPCHK(h, hipMalloc(offd, (size_t)cfg->n_envs * 3 * sizeof(float)));
    HIPCHK(h, hipMemcpy(*offd, offsets_host, (size_t)cfg->n_envs * 3 * sizeof(float), hipMemcpyHostToDevice));
  }
  if (h->fly) {
    // One env per QUAD of lanes in the step wavefronts unless schedule + 32.  The fused launch (controller wavefronts + step wavefronts in
    // one grid; schedule + 8: IK inside the step wavefront) is used while ALL its workgroups -- each with the step's dynamic LDS -- are
    // resident at once: 4 per CU in the quad layout (n <= 13 104 on 256 CUs), 1 per CU in the lane layout; bigger batches run the IK inside
    // the step wavefront.
    h->flyquad = (cfg->schedule & 32) == 0;
    int cus = 0; HIPCHK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    const FlyLaunch fused = fly_launch(h, true);
    h->fused = (cfg->schedule & 8) == 0 && fused.grid <= fused.per_cu * cus;
    // (dynamic LDS beyond the default 64 KB limit: the per-lane contact rows and candidate staging of 64 lanes)
    for (const FlyLaunch& L : {fly_launch(h, false), fused})
      HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(L.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    // mailbox [group][word][64 lanes]: the two 128-byte lines of a (group, word) hold no other group's targets
    if (h->fused) { int rc = mailbox_alloc(h, (size_t)fused.G * 64 * fly::NJ); if (rc) return rc; }
    const int nb64 = (cfg->n_envs + 63) / 64;
    hipLaunchKernelGGL(pih_fly_init_offsets_kernel, dim3(nb64), dim3(64), 0, 0, h->state, *offd, cfg->n_envs);
    hipLaunchKernelGGL(pih_fly_reset_kernel, dim3(nb64), dim3(64), 0, 0, h->P, h->state, (const unsigned char*)nullptr, 0, 0, cfg->n_envs);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipDeviceSynchronize());
    return 0;
  }
  HIPCHK(h, hipMalloc(&h->ovf, ((size_t)cfg->n_envs * OVF_WORDS + OVF_PAD_WORDS) * sizeof(float)));
  HIPCHK(h, hipMemset(h->ovf, 0, ((size_t)cfg->n_envs * OVF_WORDS + OVF_PAD_WORDS) * sizeof(float)));
  // fused launch unless schedule + 8 asks for the two-launch step; the longest-job-first order (schedule & 1) is built by the env
  // wavefronts in the bin buffers (fused) or by block 0 of pih_pre_kernel in `order` (two launches)
  h->fused = (cfg->schedule & 8) == 0;
  if (h->fused) {
    int rc = mailbox_alloc(h, (size_t)cfg->n_envs * CTRL_WORDS);
    if (rc) return rc;
    if (cfg->schedule & 1) {
      h->bin_ints = 64 + (size_t)64 * cfg->n_envs;
      HIPCHK(h, hipMalloc(&h->bins, 3 * h->bin_ints * sizeof(int)));
      HIPCHK(h, hipMemset(h->bins, 0, 3 * h->bin_ints * sizeof(int)));
    }
  } else if (cfg->schedule & 1) HIPCHK(h, hipMalloc(&h->order, (size_t)cfg->n_envs * sizeof(int)));
  hipLaunchKernelGGL(pih_init_offsets_kernel, dim3((cfg->n_envs + 63) / 64), dim3(64), 0, 0, h->state, *offd, cfg->n_envs);
  hipLaunchKernelGGL(pih_reset_kernel, dim3(cfg->n_envs), dim3(64), 0, 0, h->P, h->state, (const unsigned char*)nullptr, 0, 0);
  // the first launch (epoch 1) reads bin buffer 1: every env once, ordered by the contact counts of the reset state
  if (h->bins) hipLaunchKernelGGL(pih_bins_init_kernel, dim3(64), dim3(256), 0, 0, h->state, h->bins + h->bin_ints, cfg->n_envs);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipDeviceSynchronize());
  return 0;
}

int pih_create(const pih_config* cfg, const float* offsets_host, pih_handle** out) {
  if (!cfg || !out || cfg->n_envs <= 0) { g_err = "pih_create: bad arguments"; return -2; }
  if (cfg->task_id != PIH_TASK_PEG_IN_HOLE && cfg->task_id != PIH_TASK_RANDOM_FLY) { g_err = "pih_create: unknown task_id"; return -2; }
  if (cfg->task_id == PIH_TASK_RANDOM_FLY && (cfg->object_id < 0 || cfg->object_id >= PIH_FLY_NOBJ)) { g_err = "pih_create: unknown object_id for the random-fly task"; return -2; }
  // the switches of include/pih.h: order 0 / 1 plus the bits 4, 8, 32, 64; every other value selects a retired path or nothing
  if ((cfg->schedule & 3) >= 2 || (cfg->schedule & ~(3 | 4 | 8 | 32 | 64)) != 0) {
    g_err = "pih_create: schedule = " + std::to_string(cfg->schedule) + " is not supported (0 or 1, plus any of 4, 8, 32, 64)";
    return -2;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) { g_err = "pih_create: no HIP device (this library has no CPU path)"; return -3; }
  pih_handle* h = new pih_handle;
  h->cfg = *cfg; h->P = params_from_config(cfg);
  h->fly = cfg->task_id == PIH_TASK_RANDOM_FLY; h->words = h->fly ? PIH_FLY_STATE_WORDS : PIH_STATE_WORDS;
  float* offd = nullptr;
  int rc = -1;
  if (hipGetDevice(&h->device) == hipSuccess) rc = create_impl(h, offsets_host, &offd);
  else g_err = "pih_create: hipGetDevice failed";
  if (offd) hipFree(offd);
  if (rc != 0) { pih_destroy(h); return rc; }   // nothing leaks on the error path (g_err keeps the message)
  *out = h;
  return 0;
}

int pih_reset(pih_handle* h, const uint8_t* mask_dev, int hard, uint64_t seed, void* stream) {
  if (!h) return -2;
  // a new seed rewinds the draw sequences, and that must reach EVERY env of the handle: with a mask the unmasked envs would keep
  // their draw counter on a different seed stream (neither a replay nor a continuation; round-3 review) -- rejected
  if (mask_dev && (seed != 0 || h->rewind_pending)) {
    h->err = "pih_reset: a new seed (seed != 0, or a pending pih_reseed) needs a reset of all envs (mask_dev = NULL)";
    return -2;
  }
  PIH_ENTER(h);
  RoctxRange range(h->cfg.debug != 0, hard ? "pih_reset(hard)" : "pih_reset");
  if (seed != 0) { h->cfg.seed = seed; h->P.seed = seed; h->rewind_pending = true; }
  const int rewind = h->rewind_pending ? 1 : 0;
  h->rewind_pending = false;
  if (h->fly) hipLaunchKernelGGL(pih_fly_reset_kernel, dim3((h->cfg.n_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->P, h->state, mask_dev, hard != 0, rewind, h->cfg.n_envs);
  else hipLaunchKernelGGL(pih_reset_kernel, dim3(h->cfg.n_envs), dim3(64), 0, (hipStream_t)stream, h->P, h->state, mask_dev, hard != 0, rewind);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_reseed(pih_handle* h, uint64_t seed) {
  if (!h) return -2;
  h->cfg.seed = seed; h->P.seed = seed; h->rewind_pending = true;
  return 0;
}

static int launch_step(pih_handle* h, const float* actions, float* obs, float* reward, uint8_t* done, hipStream_t s) {
  RoctxRange range(h->cfg.debug != 0, h->fly ? "pih_step(random-fly)" : "pih_step(peg-in-hole)");
  EvTriple* t = nullptr;
  if (h->timing > 0 && (h->timing_tick++ % (unsigned)h->timing) == 0) {
    if (h->ev_used == EV_POOL) { int r = drain_events(h); if (r) return r; }
    if (h->ev_used == h->ev.size()) {
      EvTriple n;
      HIPCHK(h, hipEventCreate(&n.a)); HIPCHK(h, hipEventCreate(&n.b)); HIPCHK(h, hipEventCreate(&n.c));
      h->ev.push_back(n);
    }
    t = &h->ev[h->ev_used++];
    HIPCHK(h, hipEventRecord(t->a, s));
  }
  // random-fly: the fused launch (IK in controller wavefronts of the same grid) while all its workgroups fit the chip at once, else (and
  // with schedule + 8) the IK inside the step wavefront.  peg-in-hole: the fused launch, or with schedule + 8 the two-launch step.
  if (h->fly) {
    const FlyLaunch L = fly_launch(h, h->fused);
    FlyFused FF; memset(&FF, 0, sizeof FF);
    if (h->fused) {
      const int e = next_epoch(h);
      if (e < 0) return e;
      FF.G = L.G; FF.epoch = e; FF.mail = h->mail; FF.flags = h->flags; FF.err = h->errw;
    }
    if (t) HIPCHK(h, hipEventRecord(t->b, s));
    hipLaunchKernelGGL(L.kernel, dim3(L.grid), dim3(64), L.lds, s, h->P, h->state, actions, obs, reward, done, h->dbg, h->cfg.n_envs, FF);
    if (t) HIPCHK(h, hipEventRecord(t->c, s));
    HIPCHK(h, hipGetLastError());
    return 0;
  }
  FusedArgs F; memset(&F, 0, sizeof F);
  if (h->fused) {
    // one launch: controller wavefronts first, then the env wavefronts
    const int e = next_epoch(h);
    if (e < 0) return e;
    F.G = (h->cfg.n_envs + 63) / 64; F.n = h->cfg.n_envs; F.epoch = e; F.mail = h->mail; F.flags = h->flags; F.err = h->errw;
    if (h->bins) { F.bcur = h->bins + (size_t)(e % 3) * h->bin_ints; F.bnext = h->bins + (size_t)((e + 1) % 3) * h->bin_ints; F.bzero = h->bins + (size_t)((e + 2) % 3) * h->bin_ints; }
    if (t) HIPCHK(h, hipEventRecord(t->b, s));
    hipLaunchKernelGGL(pih_step_kernel, dim3(F.G + h->cfg.n_envs), dim3(64), 0, s, h->P, h->state, actions, obs, reward, done, h->dbg, h->ovf, (const int*)nullptr, F);
  } else {
    hipLaunchKernelGGL(pih_pre_kernel, dim3(1 + (h->cfg.n_envs + 63) / 64), dim3(PRE_THREADS), 0, s, h->P, h->state, actions, h->order, h->cfg.n_envs);
    if (t) HIPCHK(h, hipEventRecord(t->b, s));
    hipLaunchKernelGGL(pih_step_kernel, dim3(h->cfg.n_envs), dim3(64), 0, s, h->P, h->state, actions, obs, reward, done, h->dbg, h->ovf, (const int*)h->order, F);
  }
  if (t) HIPCHK(h, hipEventRecord(t->c, s));
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_step(pih_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream) {
  if (!h) return -2;
  if ((h->cfg.mode == 0 || h->fly) && !actions_dev) { h->err = "pih_step: actions_dev is NULL in action mode"; return -2; }
  PIH_ENTER(h);
  return launch_step(h, actions_dev, obs_dev, reward_dev, done_dev, (hipStream_t)stream);
}

int pih_step_n(pih_handle* h, int k, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream) {
  if (!h || k < 0) return -2;
  if ((h->cfg.mode == 0 || h->fly) && !actions_dev) { h->err = "pih_step_n: actions_dev is NULL in action mode"; return -2; }
  PIH_ENTER(h);
  for (int i = 0; i < k; i++) { int r = launch_step(h, actions_dev, obs_dev, reward_dev, done_dev, (hipStream_t)stream); if (r) return r; }
  return 0;
}

int pih_get_state(pih_handle* h, int field, void* out_dev, void* stream) {
  if (!h || !out_dev) return -2;
  PIH_ENTER(h);
  hipStream_t s = (hipStream_t)stream;
  const int n = h->cfg.n_envs;
  if (field == PIH_FIELD_DEBUG) {                              // both tasks: env-major, layout PIH_DBG_* of include/pih.h
    if (!h->dbg) { h->err = "pih_get_state: debug buffer not enabled (config.debug = 0)"; return -4; }
    HIPCHK(h, hipMemcpyAsync(out_dev, h->dbg, (size_t)n * PIH_DEBUG_WORDS * sizeof(float), hipMemcpyDeviceToDevice, s)); return 0;
  }
  if (h->fly) {
    int w0 = 0, nw = 0;
    switch (field) {
      case PIH_FIELD_STATE: w0 = 0; nw = PIH_FLY_STATE_WORDS; break;
      case PIH_FIELD_CONTACT_FORCE: w0 = PIH_F_CFORCE; nw = 1; break;
      case PIH_FIELD_EE_POS: w0 = PIH_F_EE; nw = 3; break;
      default: h->err = "pih_get_state: field not available for the random-fly task"; return -2;
    }
    hipLaunchKernelGGL(pih_soa_to_aos_kernel, dim3((n * nw + 255) / 256), dim3(256), 0, s, h->state, (float*)out_dev, n, PIH_FLY_STATE_WORDS, w0, nw);
    HIPCHK(h, hipGetLastError());
    return 0;
  }
  switch (field) {
    case PIH_FIELD_STATE: HIPCHK(h, hipMemcpyAsync(out_dev, h->state, (size_t)n * PIH_STATE_WORDS * sizeof(float), hipMemcpyDeviceToDevice, s)); return 0;
    case PIH_FIELD_TIP_POSE: hipLaunchKernelGGL(pih_gather_kernel, dim3((n * 7 + 255) / 256), dim3(256), 0, s, h->state, (float*)out_dev, n, (int)PIH_S_TIP, 7); break;
    case PIH_FIELD_CONTACT_FORCE: hipLaunchKernelGGL(pih_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, h->state, (float*)out_dev, n, (int)PIH_S_CFORCE, 1); break;
    case PIH_FIELD_EE_POS: hipLaunchKernelGGL(pih_gather_kernel, dim3((n * 3 + 255) / 256), dim3(256), 0, s, h->state, (float*)out_dev, n, (int)PIH_S_EE, 3); break;
    default: h->err = "pih_get_state: unknown field"; return -2;
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_set_state(pih_handle* h, int field, const void* in_dev, void* stream) {
  if (!h || !in_dev) return -2;
  if (field != PIH_FIELD_STATE) { h->err = "pih_set_state: only PIH_FIELD_STATE is writable"; return -2; }
  PIH_ENTER(h);
  if (h->fly) {
    const int n = h->cfg.n_envs;
    hipLaunchKernelGGL(pih_aos_to_soa_kernel, dim3((n * PIH_FLY_STATE_WORDS + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)in_dev, h->state, n, PIH_FLY_STATE_WORDS);
    HIPCHK(h, hipGetLastError());
    return 0;
  }
  HIPCHK(h, hipMemcpyAsync(h->state, in_dev, (size_t)h->cfg.n_envs * PIH_STATE_WORDS * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int pih_ik(pih_handle* h, int n, const float* q0_dev, const float* tpos_dev, const float* tquat_dev, float* qout_dev, void* stream) {
  if (!h || n <= 0 || !q0_dev || !tpos_dev || !tquat_dev || !qout_dev) return -2;
  PIH_ENTER(h);
  hipLaunchKernelGGL(pih_ik_kernel, dim3((n + 15) / 16), dim3(64), 0, (hipStream_t)stream, h->P, n, q0_dev, tpos_dev, tquat_dev, qout_dev);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_ik_ur5(pih_handle* h, int n, const float* q0_dev, const float* tpos_dev, const float* tquat_dev, float* qout_dev, void* stream) {
  if (!h || n <= 0 || !q0_dev || !tpos_dev || !tquat_dev || !qout_dev) return -2;
  PIH_ENTER(h);
  hipLaunchKernelGGL(pih_ik_ur5_kernel, dim3((n + 15) / 16), dim3(64), 0, (hipStream_t)stream, h->P, n, q0_dev, tpos_dev, tquat_dev, qout_dev);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// rows per workgroup of the two cameras.  Every workgroup sets its env's scene up once (forward kinematics): few strips per env when the
// batch alone gives the chip several rounds of workgroups (>= 8192: images differ ~3x in cost, the tail matters), more strips for small
// batches.  Returns the number of strips; *rows = rows per strip, a multiple of the 16-row tile.
static int render_strips(int height, int env_count, int* rows) {
  int strips = (8192 + env_count - 1) / env_count;
  const int max_strips = (height + 31) / 32;
  strips = strips < 1 ? 1 : (strips > max_strips ? max_strips : strips);
  *rows = ((height + strips - 1) / strips + 15) / 16 * 16;
  return (height + *rows - 1) / *rows;
}

int pih_render(pih_handle* h, float* out_dev, int width, int height, int env_begin, int env_count, void* stream) {
  return pih_render_ex(h, out_dev, width, height, env_begin, env_count, 0, stream);
}

// ---- what the camera entry points check, each piece once; an entry point calls them in ITS order (which of two simultaneous faults is
// reported is part of its behaviour: tests/test_gpu_render_errors.py).  Each returns 0, or -2 with the handle's error text set.
struct RenderCall {      // the arguments every camera entry point takes
  pih_handle* h; const char* name; const void* out; int width, height, env_begin, env_count;
  int fail(const std::string& what) const { h->err = std::string(name) + ": " + what; return -2; }
  // handle, out, sizes, env range (`also`: what else an entry point files under "bad arguments")
  int bad_arguments(bool also = false) const {
    if (h && out && width > 0 && height > 0 && env_begin >= 0 && env_count > 0 && env_begin + env_count <= h->cfg.n_envs && !also) return 0;
    return h ? fail("bad arguments") : -2;
  }
  int misaligned() const { return (reinterpret_cast<uintptr_t>(out) & 15) != 0 ? fail("out_dev must be 16-byte aligned") : 0; }
  int too_many() const { return env_count > 65535 ? fail("env_count > 65535 per call") : 0; }
  // unknown bits, both output formats, both camera frames, a device flag without its array (`preset`: what NULL would have meant)
  int bad_flags(int flags, int known, const char* preset, const void* cam_ptr, const void* light_ptr = nullptr) const {
    if ((flags & ~known) != 0) return fail("unknown flag");
    if ((flags & PIH_RENDER_OUT_RGBA8) && (flags & PIH_RENDER_OUT_DEPTH)) return fail("PIH_RENDER_OUT_RGBA8 and PIH_RENDER_OUT_DEPTH exclude each other");
    if ((flags & PIH_RENDER_CAM_EE) && (flags & PIH_RENDER_CAM_EE_POS)) return fail("PIH_RENDER_CAM_EE and PIH_RENDER_CAM_EE_POS exclude each other");
    if ((flags & PIH_RENDER_CAM_DEVICE) && !cam_ptr) return fail(std::string("PIH_RENDER_CAM_DEVICE needs a camera array (NULL = ") + preset + " is for a host camera)");
    if ((flags & PIH_RENDER_LIGHT_DEVICE) && !light_ptr) return fail("PIH_RENDER_LIGHT_DEVICE needs a light array (NULL = PIH_LIGHT_DEFAULT is for a host light)");
    return 0;
  }
  // The camera the kernel gets by value: the caller's host camera, tested here, or `cam` as it comes in (the task's preset) for NULL and
  // for per-env cameras in device memory, which the kernel tests.  name_word: say which word is not finite (pih_render_cam does not).
  // wrist_flags != nullptr: NULL means the peg-in-hole wrist preset, which is in the PIH_RENDER_CAM_EE_POS frame whatever flag was passed.
  int host_camera(fly::FlyCam& cam, const float* cam_ptr, int flags, bool name_word, int* wrist_flags) const {
    if (flags & PIH_RENDER_CAM_DEVICE) return 0;
    if (cam_ptr) memcpy(cam.w, cam_ptr, sizeof cam.w);
    else if (wrist_flags) *wrist_flags = (flags & ~PIH_RENDER_CAM_EE) | PIH_RENDER_CAM_EE_POS;
    static const char* const what[] = {nullptr, "eye == target (or not finite)", "up is zero or parallel to the view axis target - eye", "fov outside (0, 180) degrees",
                                       "aspect <= 0", "near <= 0", "far <= near"};
    if (name_word) {
      // (a NaN or an infinity is looked for in the words' bits, as integers: the library's floating-point code is built with -ffast-math)
      static const char* const word[] = {"eye", "eye", "eye", "target", "target", "target", "up", "up", "up", "fov", "aspect", "near", "far"};
      uint32_t bits[PIH_CAM_WORDS]; memcpy(bits, cam.w, sizeof bits);
      for (int i = 0; i < PIH_CAM_WORDS; i++)
        if ((bits[i] & 0x7f800000u) == 0x7f800000u) return fail(std::string("degenerate camera: ") + word[i] + " is not finite");
    }
    const int code = fly::cam_degenerate(cam.w);
    return code != fly::CAM_OK ? fail(std::string("degenerate camera: ") + what[code]) : 0;
  }
};
#define PIH_RENDER_CHECK(x) do { if (const int _rc = (x)) return _rc; } while (0)
static const int RENDER_FMT = PIH_RENDER_OUT_RGBA8 | PIH_RENDER_OUT_DEPTH;
static const int RENDER_CAM_FLAGS = PIH_RENDER_SHADED | PIH_RENDER_CAM_EE | RENDER_FMT | PIH_RENDER_CAM_DEVICE;      // what pih_render_cam knows

int pih_render_ex(pih_handle* h, float* out_dev, int width, int height, int env_begin, int env_count, int flags, void* stream) {
  const RenderCall c = {h, "pih_render", out_dev, width, height, env_begin, env_count};
  PIH_RENDER_CHECK(c.bad_arguments());
  if (h->fly) return c.fail("the wrist camera belongs to the peg-in-hole task");
  PIH_RENDER_CHECK(c.misaligned());
  // (the output formats and the device cameras of pih_render_cam do not exist here: out_dev is float[count, H, W, 4] whatever the flags say)
  if ((flags & ~PIH_RENDER_SHADED) != 0) { h->err = "pih_render_ex: unknown flag (the wrist camera takes PIH_RENDER_SHADED only)"; return -2; }
  PIH_ENTER(h);
  int rows; const int strips = render_strips(height, env_count, &rows);
  PIH_RENDER_CHECK(c.too_many());
  hipLaunchKernelGGL(pih_render_kernel, dim3(strips, env_count), dim3(RENDER_THREADS), 0, (hipStream_t)stream, h->state, out_dev, env_begin, width, height, rows, flags);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_render_cam(pih_handle* h, float* out_dev, const float* cam_ptr, int width, int height, int env_begin, int env_count, int flags, void* stream) {
  const RenderCall c = {h, "pih_render_cam", out_dev, width, height, env_begin, env_count};
  PIH_RENDER_CHECK(c.bad_arguments((flags & ~RENDER_CAM_FLAGS) != 0));      // (an unknown flag is "bad arguments" here)
  if (!h->fly) return c.fail("the free camera belongs to the random-fly task (peg-in-hole: pih_render / pih_render_ex)");
  PIH_RENDER_CHECK(c.bad_flags(flags, RENDER_CAM_FLAGS, "default", cam_ptr));
  PIH_RENDER_CHECK(c.misaligned());
  PIH_RENDER_CHECK(c.too_many());
  fly::FlyCam cam = {PIH_FLY_CAM_DEFAULT};
  PIH_RENDER_CHECK(c.host_camera(cam, cam_ptr, flags, false, nullptr));
  PIH_ENTER(h);
  const int fmt = flags & RENDER_FMT;
  const bool cam_on_device = (flags & PIH_RENDER_CAM_DEVICE) != 0;
  int rows; const int strips = render_strips(height, env_count, &rows);
  if (fmt || cam_on_device)
    fly_image_launch(fmt, dim3(strips, env_count), (hipStream_t)stream, h->state, out_dev, cam, cam_on_device ? cam_ptr : nullptr, h->cfg.n_envs, h->P.object, env_begin, width, height, rows, flags);
  else      // the float4 image of one host camera: the kernel it has always been
    hipLaunchKernelGGL(pih_fly_render_kernel, dim3(strips, env_count), dim3(RENDER_THREADS), 0, (hipStream_t)stream, h->state, out_dev, cam,
                       h->cfg.n_envs, h->P.object, env_begin, width, height, rows, flags);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_render_view(pih_handle* h, void* out_dev, const float* cam_ptr, int width, int height, int env_begin, int env_count, int flags, void* stream) {
  const RenderCall c = {h, "pih_render_view", out_dev, width, height, env_begin, env_count};
  PIH_RENDER_CHECK(c.bad_arguments());
  if (h->fly) return c.fail("this camera belongs to the peg-in-hole task (random-fly: pih_render_cam)");
  PIH_RENDER_CHECK(c.bad_flags(flags, RENDER_CAM_FLAGS | PIH_RENDER_CAM_EE_POS, "the wrist preset", cam_ptr));
  PIH_RENDER_CHECK(c.misaligned());
  PIH_RENDER_CHECK(c.too_many());
  fly::FlyCam cam = {PIH_VIEW_CAM_WRIST};
  PIH_RENDER_CHECK(c.host_camera(cam, cam_ptr, flags, true, &flags));
  PIH_ENTER(h);
  int rows; const int strips = render_strips(height, env_count, &rows);
  view_launch(flags & RENDER_FMT, dim3(strips, env_count), (hipStream_t)stream, h->state, out_dev, cam, (flags & PIH_RENDER_CAM_DEVICE) ? cam_ptr : nullptr, env_begin, width, height, rows, flags);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_render_lit(pih_handle* h, void* out_dev, const float* cam_ptr, const float* light_ptr, int width, int height, int env_begin, int env_count, int flags, void* stream) {
  const RenderCall c = {h, "pih_render_lit", out_dev, width, height, env_begin, env_count};
  PIH_RENDER_CHECK(c.bad_arguments());
  // the flags of the handle's free camera (pih_render_cam / pih_render_view), plus the device light
  PIH_RENDER_CHECK(c.bad_flags(flags, RENDER_CAM_FLAGS | PIH_RENDER_LIGHT_DEVICE | (h->fly ? 0 : PIH_RENDER_CAM_EE_POS), "the preset", cam_ptr, light_ptr));
  PIH_RENDER_CHECK(c.misaligned());
  PIH_RENDER_CHECK(c.too_many());
  fly::FlyCam cam = {PIH_FLY_CAM_DEFAULT};
  if (!h->fly) cam = fly::FlyCam{PIH_VIEW_CAM_WRIST};
  PIH_RENDER_CHECK(c.host_camera(cam, cam_ptr, flags, true, h->fly ? nullptr : &flags));
  const bool light_on_device = (flags & PIH_RENDER_LIGHT_DEVICE) != 0;
  float light[PIH_LIGHT_WORDS] = PIH_LIGHT_DEFAULT;
  if (!light_on_device) {
    if (light_ptr) memcpy(light, light_ptr, sizeof light);
    const char* what = nullptr;
    if (lit_light_check(light, &what) != 0) return c.fail(std::string("degenerate light: ") + what);
  }
  PIH_ENTER(h);
  int rows; const int strips = render_strips(height, env_count, &rows);
  lit_launch(h->fly, flags & RENDER_FMT, dim3(strips, env_count), (hipStream_t)stream, h->state, out_dev, cam, (flags & PIH_RENDER_CAM_DEVICE) ? cam_ptr : nullptr, light,
             light_on_device ? light_ptr : nullptr, h->cfg.n_envs, h->P.object, env_begin, width, height, rows, flags);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_grasp_labels(pih_handle* h, float* out_dev, float* meta_dev, int size, int env_begin, int env_count, void* stream) {
  if (!h || !out_dev || size <= 0 || env_begin < 0 || env_count <= 0 || env_count > 65535 || env_begin + env_count > h->cfg.n_envs) {
    if (h) h->err = "pih_grasp_labels: bad arguments";
    return -2;
  }
  if (h->fly) { h->err = "pih_grasp_labels: the grasp labels belong to the peg-in-hole task"; return -2; }
  PIH_ENTER(h);
  hipLaunchKernelGGL(pih_labels_kernel, dim3((size * size + 1023) / 1024, env_count), dim3(256), 0, (hipStream_t)stream, h->state, out_dev, meta_dev, env_begin, size);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_set_timing(pih_handle* h, int enable) { if (!h) return -2; h->timing = enable > 0 ? enable : 0; h->timing_tick = 0; return 0; }

int pih_timing2(pih_handle* h, int reset, double* pre_ms_out, double* step_ms_out, int64_t* launches_out) {
  if (!h) return -2;
  PIH_ENTER(h);
  int r = drain_events(h);
  if (r) return r;
  if (h->errw_host && *h->errw_host) { h->err = CTRL_TIMEOUT_MSG; return -5; }
  if (pre_ms_out) *pre_ms_out = h->acc_n ? h->acc_pre_ms / (double)h->acc_n : 0.0;
  if (step_ms_out) *step_ms_out = h->acc_n ? h->acc_step_ms / (double)h->acc_n : 0.0;
  if (launches_out) *launches_out = h->acc_n;
  if (reset) { h->acc_pre_ms = h->acc_step_ms = 0; h->acc_n = 0; }
  return 0;
}

int pih_timing(pih_handle* h, int reset, double* avg_ms_out, int64_t* launches_out) {
  double a = 0, b = 0;
  int r = pih_timing2(h, reset, &a, &b, launches_out);
  if (r == 0 && avg_ms_out) *avg_ms_out = a + b;
  return r;
}

// ---- batched robot-model queries (include/pih_robot.h; kernels in pih_robot.hip).  Every argument is checked before the device is touched.
static int robot_bad(pih_handle* h, const char* call, const char* arg, const char* why) {
  const std::string m = std::string(call) + ": " + arg + " " + why;
  if (h) h->err = m;
  g_err = m;
  return -2;
}
// the checks the four queries share; *ndof / *nframes of the robot.  -> 0, -2, or 1 for n == 0 (nothing to do)
static int robot_check(pih_handle* h, const char* call, int robot, int n, int* ndof, int* nframes) {
  if (!h) return robot_bad(h, call, "h", "is NULL");
  if (robot_dims(robot, ndof, nframes) != 0) return robot_bad(h, call, "robot", "is neither PIH_ROBOT_PANDA nor PIH_ROBOT_UR5");
  if (n < 0) return robot_bad(h, call, "n", "is negative");
  if (n > (1 << 30)) return robot_bad(h, call, "n", "is larger than 2^30");
  return n == 0 ? 1 : 0;
}
// Which store variant of pih_robot.hip a call of n problems uses: every lane stores its own rows below `threshold` problems, the wavefront's
// rows go through LDS from there on.  The thresholds are where the staged variant became the faster one on the MI355X (DESIGN.md 6.6:
// below them a call is launch-bound and the barrier and the copy loop only add latency; inverse dynamics, 6 .. 9 words per problem, never
// gains).  PIH_ROBOT_STORE = direct | staged in the environment overrides the rule: the measurement switch of tools/robot_query_bench.py,
// not part of the ABI.  Same values either way.
constexpr int ROBOT_FK_STAGED_FROM = 32768, ROBOT_JACOBIAN_STAGED_FROM = 16384, ROBOT_MASS_STAGED_FROM = 24576;
static bool robot_staged(int n, int threshold) {
  const char* e = getenv("PIH_ROBOT_STORE");
  if (e && !strcmp(e, "direct")) return false;
  if (e && !strcmp(e, "staged")) return true;
  return n >= threshold;
}

int pih_robot_dims(int robot, int32_t out[2]) {
  int nd, nf;
  if (!out) return robot_bad(nullptr, "pih_robot_dims", "out", "is NULL");
  if (robot_dims(robot, &nd, &nf) != 0) return robot_bad(nullptr, "pih_robot_dims", "robot", "is neither PIH_ROBOT_PANDA nor PIH_ROBOT_UR5");
  out[0] = nd; out[1] = nf;
  return 0;
}
int pih_link_states_frames(int task_id) { return link_states_frames(task_id); }

int pih_robot_fk(pih_handle* h, int robot, int n, const float* q_dev, const float* qd_dev, float* out_dev, void* stream) {
  int nd, nf;
  const int c = robot_check(h, "pih_robot_fk", robot, n, &nd, &nf);
  if (c) return c < 0 ? c : 0;
  if (!q_dev) return robot_bad(h, "pih_robot_fk", "q_dev", "is NULL");
  if (!out_dev) return robot_bad(h, "pih_robot_fk", "out_dev", "is NULL");
  PIH_ENTER(h);
  robot_fk_launch(robot, robot_staged(n, ROBOT_FK_STAGED_FROM), (hipStream_t)stream, n, q_dev, qd_dev, out_dev);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_robot_jacobian(pih_handle* h, int robot, int n, const float* q_dev, int frame, const float* local_pos_dev, float* out_dev, void* stream) {
  int nd, nf;
  const int c = robot_check(h, "pih_robot_jacobian", robot, n, &nd, &nf);
  if (c < 0) return c;
  if (frame < 0 || frame >= nf) return robot_bad(h, "pih_robot_jacobian", "frame", "is outside the robot's frames");
  if (c) return 0;
  if (!q_dev) return robot_bad(h, "pih_robot_jacobian", "q_dev", "is NULL");
  if (!out_dev) return robot_bad(h, "pih_robot_jacobian", "out_dev", "is NULL");
  PIH_ENTER(h);
  robot_jacobian_launch(robot, robot_staged(n, ROBOT_JACOBIAN_STAGED_FROM), (hipStream_t)stream, n, q_dev, frame, local_pos_dev, out_dev);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_robot_mass_matrix(pih_handle* h, int robot, int n, const float* q_dev, float* out_dev, void* stream) {
  int nd, nf;
  const int c = robot_check(h, "pih_robot_mass_matrix", robot, n, &nd, &nf);
  if (c) return c < 0 ? c : 0;
  if (!q_dev) return robot_bad(h, "pih_robot_mass_matrix", "q_dev", "is NULL");
  if (!out_dev) return robot_bad(h, "pih_robot_mass_matrix", "out_dev", "is NULL");
  PIH_ENTER(h);
  robot_mass_launch(robot, robot_staged(n, ROBOT_MASS_STAGED_FROM), (hipStream_t)stream, n, q_dev, out_dev);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_robot_inverse_dynamics(pih_handle* h, int robot, int n, const float* q_dev, const float* qd_dev, const float* qdd_dev, float* tau_dev, void* stream) {
  int nd, nf;
  const int c = robot_check(h, "pih_robot_inverse_dynamics", robot, n, &nd, &nf);
  if (c) return c < 0 ? c : 0;
  if (!q_dev) return robot_bad(h, "pih_robot_inverse_dynamics", "q_dev", "is NULL");
  if (!qd_dev) return robot_bad(h, "pih_robot_inverse_dynamics", "qd_dev", "is NULL");
  if (!qdd_dev) return robot_bad(h, "pih_robot_inverse_dynamics", "qdd_dev", "is NULL");
  if (!tau_dev) return robot_bad(h, "pih_robot_inverse_dynamics", "tau_dev", "is NULL");
  PIH_ENTER(h);
  robot_invdyn_launch(robot, (hipStream_t)stream, n, q_dev, qd_dev, qdd_dev, tau_dev);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_link_states(pih_handle* h, float* out_dev, int env_begin, int env_count, void* stream) {
  if (!h) return robot_bad(h, "pih_link_states", "h", "is NULL");
  if (!out_dev) return robot_bad(h, "pih_link_states", "out_dev", "is NULL");
  if (env_begin < 0 || env_count <= 0 || env_begin > h->cfg.n_envs || env_count > h->cfg.n_envs - env_begin)
    return robot_bad(h, "pih_link_states", "env_begin / env_count", "is outside the handle's envs");
  PIH_ENTER(h);
  link_states_launch(h->fly, (hipStream_t)stream, h->state, out_dev, h->cfg.n_envs, env_begin, env_count);
  HIPCHK(h, hipGetLastError());
  return 0;
}

const char* pih_last_error(pih_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

}  // extern "C"
