// pih_fly.hip -- the kernels of the random-fly task: step, reset, state layout (its cameras: pih_fly_image.hip, pih_lit.hip).  gfx950 only.
// The C ABI (pih_hip.hip) reaches them through the launch functions at the end (pih_launch.h), which own the choice of instantiation, the
// grid, the dynamic LDS and whether the fused grid fits the chip.
#include <hip/hip_runtime.h>
#include <cstring>
#include <type_traits>
#include "pih_device.h"      // (QuadDpp of pih_ikq.h, the mailbox, the debug stamps of pih_wave.h)
#include "pih_fly.h"
#include "pih_launch.h"

using namespace pih;

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

// ------------------------------------------------------------------------------------------------ launches (pih_launch.h)
// The random-fly step launch of n envs in a layout (quad: one env per quad of lanes), fused or not: the instantiation of pih_fly_step_kernel,
// the grid (G controller workgroups in front of the step workgroups when fused), the dynamic LDS of every workgroup, and how many of them a
// CU holds
struct FlyLaunch { decltype(&pih_fly_step_kernel<false, false>) kernel; int G, grid, per_cu; size_t lds; };
static_assert((size_t)fly::LANE_WORDS * 64 * sizeof(float) <= 160 * 1024 && (size_t)fly::LANE_WORDS_Q * 64 * sizeof(float) * 4 <= 160 * 1024, "the random-fly kernel's per-wave LDS exceeds its share of a CU's 160 KB");
static FlyLaunch fly_launch(int n, bool quad, bool fused) {
  FlyLaunch L;
  L.G = (n + 63) / 64;
  if (quad) { L.kernel = fused ? pih_fly_step_kernel<true, true> : pih_fly_step_kernel<false, true>; L.grid = (n + 15) / 16; L.per_cu = 4; L.lds = (size_t)fly::LANE_WORDS_Q * 64 * sizeof(float); }
  else { L.kernel = fused ? pih_fly_step_kernel<true, false> : pih_fly_step_kernel<false, false>; L.grid = L.G; L.per_cu = 1; L.lds = (size_t)fly::LANE_WORDS * 64 * sizeof(float); }
  if (fused) L.grid += L.G;
  return L;
}

namespace pih {
// mailbox [group][word][64 lanes]: the two 128-byte lines of a (group, word) hold no other group's targets
size_t fly_mail_words(int n) { return (size_t)((n + 63) / 64) * 64 * fly::NJ; }
// The fused launch is used while ALL its workgroups -- each with the step's dynamic LDS -- are resident at once: 4 per CU in the quad layout
// (n <= 13 104 on 256 CUs), 1 per CU in the lane layout
bool fly_fused_fits(int n, bool quad, int cus) {
  const FlyLaunch L = fly_launch(n, quad, true);
  return L.grid <= L.per_cu * cus;
}
// (dynamic LDS beyond the default 64 KB limit: the per-lane contact rows and candidate staging of 64 lanes)
hipError_t fly_step_prepare(bool quad) {
  for (const bool fused : {false, true}) {
    const FlyLaunch L = fly_launch(1, quad, fused);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(L.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
void fly_step_launch(hipStream_t stream, const Params& P, const StepIO& io, int n, bool quad, const Mailbox* mb) {
  const FlyLaunch L = fly_launch(n, quad, mb != nullptr);
  FlyFused FF; memset(&FF, 0, sizeof FF);
  if (mb) { FF.G = L.G; FF.epoch = mb->epoch; FF.mail = mb->mail; FF.flags = mb->flags; FF.err = mb->err; }
  hipLaunchKernelGGL(L.kernel, dim3(L.grid), dim3(64), L.lds, stream, P, io.state, io.actions, io.obs, io.reward, io.done, io.dbg, n, FF);
}
void fly_init_offsets_launch(hipStream_t stream, float* state, const float* offsets, int n) {
  hipLaunchKernelGGL(pih_fly_init_offsets_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, state, offsets, n);
}
void fly_reset_launch(hipStream_t stream, const Params& P, float* state, const unsigned char* mask, int hard, int rewind, int n) {
  hipLaunchKernelGGL(pih_fly_reset_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, P, state, mask, hard, rewind, n);
}
void fly_get_words_launch(hipStream_t stream, const float* soa, float* aos, int n, int word0, int nwords) {
  hipLaunchKernelGGL(pih_soa_to_aos_kernel, dim3((n * nwords + 255) / 256), dim3(256), 0, stream, soa, aos, n, PIH_FLY_STATE_WORDS, word0, nwords);
}
void fly_set_state_launch(hipStream_t stream, const float* aos, float* soa, int n) {
  hipLaunchKernelGGL(pih_aos_to_soa_kernel, dim3((n * PIH_FLY_STATE_WORDS + 255) / 256), dim3(256), 0, stream, aos, soa, n, PIH_FLY_STATE_WORDS);
}
}  // namespace pih
