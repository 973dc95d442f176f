// pih_hip.hip -- the C ABI (include/pih.h, include/pih_robot.h) of the MI355X-native peg-in-hole environment, and nothing else: the handle,
// its allocations, the fused-launch state, timing, roctx ranges, and every entry point with its argument checks.  Host code only: every
// kernel lives in a translation unit of its own kind (pih_peg.hip, pih_fly.hip, pih_fly_image.hip, pih_view.hip, pih_lit.hip,
// pih_robot.hip) and is reached through the launch functions of pih_launch.h, so an edit here cannot appear in a kernel's code.
// Build: build.py (one hipcc call over all translation units)
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pih_common.h"            // Params, config_defaults, params_from_config, the overflow area's size
#include "pih_fly_render.h"        // fly::FlyCam, fly::cam_degenerate
#include "pih_launch.h"

using namespace pih;

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
    // resident at once (fly_fused_fits, pih_fly.hip); bigger batches run the IK inside the step wavefront.
    h->flyquad = (cfg->schedule & 32) == 0;
    int cus = 0; HIPCHK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    h->fused = (cfg->schedule & 8) == 0 && fly_fused_fits(cfg->n_envs, h->flyquad, cus);
    HIPCHK(h, fly_step_prepare(h->flyquad));
    if (h->fused) { int rc = mailbox_alloc(h, fly_mail_words(cfg->n_envs)); if (rc) return rc; }
    fly_init_offsets_launch(0, h->state, *offd, cfg->n_envs);
    fly_reset_launch(0, h->P, h->state, nullptr, 0, 0, cfg->n_envs);
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
    int rc = mailbox_alloc(h, peg_mail_words(cfg->n_envs));
    if (rc) return rc;
    if (cfg->schedule & 1) {
      h->bin_ints = peg_bin_ints(cfg->n_envs);
      HIPCHK(h, hipMalloc(&h->bins, 3 * h->bin_ints * sizeof(int)));
      HIPCHK(h, hipMemset(h->bins, 0, 3 * h->bin_ints * sizeof(int)));
    }
  } else if (cfg->schedule & 1) HIPCHK(h, hipMalloc(&h->order, (size_t)cfg->n_envs * sizeof(int)));
  peg_init_offsets_launch(0, h->state, *offd, cfg->n_envs);
  peg_reset_launch(0, h->P, h->state, nullptr, 0, 0, cfg->n_envs);
  // the first launch (epoch 1) reads bin buffer 1: every env once, ordered by the contact counts of the reset state
  if (h->bins) peg_bins_init_launch(0, h->state, h->bins + h->bin_ints, cfg->n_envs);
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
  (h->fly ? fly_reset_launch : peg_reset_launch)((hipStream_t)stream, h->P, h->state, mask_dev, hard != 0, rewind, h->cfg.n_envs);
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
  const int n = h->cfg.n_envs;
  const StepIO io = {h->state, actions, obs, reward, done, h->dbg};
  Mailbox mb = {h->mail, h->flags, h->errw, 0};
  if (h->fused) {
    mb.epoch = next_epoch(h);
    if (mb.epoch < 0) return mb.epoch;
  }
  if (h->fly) {
    if (t) HIPCHK(h, hipEventRecord(t->b, s));
    fly_step_launch(s, h->P, io, n, h->flyquad, h->fused ? &mb : nullptr);
  } else if (h->fused) {
    // one launch: controller wavefronts first, then the env wavefronts; the three bin buffers rotate (current / next / being zeroed)
    Bins bins = {nullptr, nullptr, nullptr};
    const int e = mb.epoch;
    if (h->bins) bins = {h->bins + (size_t)(e % 3) * h->bin_ints, h->bins + (size_t)((e + 1) % 3) * h->bin_ints, h->bins + (size_t)((e + 2) % 3) * h->bin_ints};
    if (t) HIPCHK(h, hipEventRecord(t->b, s));
    peg_step_fused_launch(s, h->P, io, h->ovf, n, mb, bins);
  } else {
    peg_pre_launch(s, h->P, h->state, actions, h->order, n);
    if (t) HIPCHK(h, hipEventRecord(t->b, s));
    peg_step_launch(s, h->P, io, h->ovf, h->order, n);
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
    fly_get_words_launch(s, h->state, (float*)out_dev, n, w0, nw);
    HIPCHK(h, hipGetLastError());
    return 0;
  }
  switch (field) {
    case PIH_FIELD_STATE: HIPCHK(h, hipMemcpyAsync(out_dev, h->state, (size_t)n * PIH_STATE_WORDS * sizeof(float), hipMemcpyDeviceToDevice, s)); return 0;
    case PIH_FIELD_TIP_POSE: peg_gather_launch(s, h->state, (float*)out_dev, n, (int)PIH_S_TIP, 7); break;
    case PIH_FIELD_CONTACT_FORCE: peg_gather_launch(s, h->state, (float*)out_dev, n, (int)PIH_S_CFORCE, 1); break;
    case PIH_FIELD_EE_POS: peg_gather_launch(s, h->state, (float*)out_dev, n, (int)PIH_S_EE, 3); break;
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
    fly_set_state_launch((hipStream_t)stream, (const float*)in_dev, h->state, h->cfg.n_envs);
    HIPCHK(h, hipGetLastError());
    return 0;
  }
  HIPCHK(h, hipMemcpyAsync(h->state, in_dev, (size_t)h->cfg.n_envs * PIH_STATE_WORDS * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int pih_ik(pih_handle* h, int n, const float* q0_dev, const float* tpos_dev, const float* tquat_dev, float* qout_dev, void* stream) {
  if (!h || n <= 0 || !q0_dev || !tpos_dev || !tquat_dev || !qout_dev) return -2;
  PIH_ENTER(h);
  ik_launch(false, (hipStream_t)stream, h->P, n, q0_dev, tpos_dev, tquat_dev, qout_dev);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int pih_ik_ur5(pih_handle* h, int n, const float* q0_dev, const float* tpos_dev, const float* tquat_dev, float* qout_dev, void* stream) {
  if (!h || n <= 0 || !q0_dev || !tpos_dev || !tquat_dev || !qout_dev) return -2;
  PIH_ENTER(h);
  ik_launch(true, (hipStream_t)stream, h->P, n, q0_dev, tpos_dev, tquat_dev, qout_dev);
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
  render_launch(dim3(strips, env_count), (hipStream_t)stream, h->state, out_dev, env_begin, width, height, rows, flags);
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
  fly_image_launch(fmt, dim3(strips, env_count), (hipStream_t)stream, h->state, out_dev, cam, cam_on_device ? cam_ptr : nullptr, h->cfg.n_envs, h->P.object, env_begin, width, height, rows, flags);
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
  labels_launch((hipStream_t)stream, h->state, out_dev, meta_dev, env_begin, env_count, size);
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

// ---- batched ray tests (include/pih_robot.h; kernels in pih_rays.hip)
int pih_ray_test(pih_handle* h, float* out_dev, const float* rays_dev, int rays_per_env, int env_begin, int env_count, int flags, void* stream) {
  if (!h) return robot_bad(h, "pih_ray_test", "h", "is NULL");
  if (!out_dev) return robot_bad(h, "pih_ray_test", "out_dev", "is NULL");
  if (!rays_dev) return robot_bad(h, "pih_ray_test", "rays_dev", "is NULL");
  if (rays_per_env < 1) return robot_bad(h, "pih_ray_test", "rays_per_env", "is smaller than 1");
  if (rays_per_env > (1 << 20)) return robot_bad(h, "pih_ray_test", "rays_per_env", "is larger than 2^20");
  if (env_begin < 0 || env_count <= 0 || env_begin > h->cfg.n_envs || env_count > h->cfg.n_envs - env_begin)
    return robot_bad(h, "pih_ray_test", "env_begin / env_count", "is outside the handle's envs");
  if (env_count > 65535) return robot_bad(h, "pih_ray_test", "env_count", "is larger than 65535 per call");
  if ((flags & ~(PIH_RAY_FRAME_EE | PIH_RAY_SHARED | PIH_RAY_IGNORE_ROBOT)) != 0) return robot_bad(h, "pih_ray_test", "flags", "has an unknown bit");
  if ((reinterpret_cast<uintptr_t>(out_dev) & 15) != 0) return robot_bad(h, "pih_ray_test", "out_dev", "must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(rays_dev) & 15) != 0) return robot_bad(h, "pih_ray_test", "rays_dev", "must be 16-byte aligned");
  PIH_ENTER(h);
  ray_test_launch(h->fly, (hipStream_t)stream, h->state, out_dev, rays_dev, rays_per_env, h->cfg.n_envs, h->P.object, env_begin, env_count, flags);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// ---- batched closest-point queries (include/pih_robot.h; kernels in pih_dist.hip)
int pih_closest_points(pih_handle* h, float* out_dev, const float* points_dev, int points_per_env, int groups, int env_begin, int env_count, int flags, void* stream) {
  if (!h) return robot_bad(h, "pih_closest_points", "h", "is NULL");
  if (!out_dev) return robot_bad(h, "pih_closest_points", "out_dev", "is NULL");
  if (!points_dev) return robot_bad(h, "pih_closest_points", "points_dev", "is NULL");
  if (points_per_env < 1) return robot_bad(h, "pih_closest_points", "points_per_env", "is smaller than 1");
  if (points_per_env > (1 << 20)) return robot_bad(h, "pih_closest_points", "points_per_env", "is larger than 2^20");
  if (env_begin < 0 || env_count <= 0 || env_begin > h->cfg.n_envs || env_count > h->cfg.n_envs - env_begin)
    return robot_bad(h, "pih_closest_points", "env_begin / env_count", "is outside the handle's envs");
  if (env_count > 65535) return robot_bad(h, "pih_closest_points", "env_count", "is larger than 65535 per call");
  if ((groups & ~PIH_GROUP_ALL) != 0) return robot_bad(h, "pih_closest_points", "groups", "has a bit outside PIH_GROUP_ALL");
  if ((groups & (h->fly ? (PIH_GROUP_ARM | PIH_GROUP_OBJECT | PIH_GROUP_TABLE) : PIH_GROUP_ALL)) == 0)
    return robot_bad(h, "pih_closest_points", "groups", "selects nothing in this task");
  if ((flags & ~(PIH_RAY_FRAME_EE | PIH_RAY_SHARED)) != 0) return robot_bad(h, "pih_closest_points", "flags", "has an unknown bit");
  if ((reinterpret_cast<uintptr_t>(out_dev) & 15) != 0) return robot_bad(h, "pih_closest_points", "out_dev", "must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(points_dev) & 15) != 0) return robot_bad(h, "pih_closest_points", "points_dev", "must be 16-byte aligned");
  PIH_ENTER(h);
  closest_points_launch(h->fly, (hipStream_t)stream, h->state, out_dev, points_dev, points_per_env, groups, h->cfg.n_envs, h->P.object, env_begin, env_count, flags);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// ---- robot clearance for many joint configurations (include/pih_robot.h; kernels in pih_clear.hip)
int pih_robot_clearance_probes(int task_id) { return robot_clearance_probes(task_id); }
int pih_robot_clearance(pih_handle* h, float* out_dev, const float* q_dev, int configs_per_env, float reach, int groups, int env_begin, int env_count, int flags, void* stream) {
  if (!h) return robot_bad(h, "pih_robot_clearance", "h", "is NULL");
  if (!out_dev) return robot_bad(h, "pih_robot_clearance", "out_dev", "is NULL");
  if (configs_per_env < 1) return robot_bad(h, "pih_robot_clearance", "configs_per_env", "is smaller than 1");
  if (configs_per_env > (1 << 20)) return robot_bad(h, "pih_robot_clearance", "configs_per_env", "is larger than 2^20");
  if (!q_dev && configs_per_env != 1) return robot_bad(h, "pih_robot_clearance", "q_dev", "is NULL with configs_per_env != 1 (NULL = each env's current joint state)");
  unsigned reach_bits; memcpy(&reach_bits, &reach, sizeof reach_bits);      // (the library is built with -ffast-math: the exponent says it)
  if ((reach_bits & 0x7f800000u) == 0x7f800000u || (reach_bits >> 31) != 0 || (reach_bits & 0x7fffffffu) == 0)
    return robot_bad(h, "pih_robot_clearance", "reach", "is not finite or not larger than 0");
  if (env_begin < 0 || env_count <= 0 || env_begin > h->cfg.n_envs || env_count > h->cfg.n_envs - env_begin)
    return robot_bad(h, "pih_robot_clearance", "env_begin / env_count", "is outside the handle's envs");
  if (env_count > 65535) return robot_bad(h, "pih_robot_clearance", "env_count", "is larger than 65535 per call");
  if ((flags & ~PIH_RAY_SHARED) != 0) return robot_bad(h, "pih_robot_clearance", "flags", "has an unknown bit (only PIH_RAY_SHARED is known)");
  if ((groups & ~(PIH_GROUP_OBJECT | PIH_GROUP_TABLE)) != 0)
    return robot_bad(h, "pih_robot_clearance", "groups", "has a bit outside PIH_GROUP_OBJECT | PIH_GROUP_TABLE (fingers, hole and the arm itself are not measured)");
  if (groups == 0) return robot_bad(h, "pih_robot_clearance", "groups", "selects nothing");
  if ((reinterpret_cast<uintptr_t>(out_dev) & 15) != 0) return robot_bad(h, "pih_robot_clearance", "out_dev", "must be 16-byte aligned");
  PIH_ENTER(h);
  robot_clearance_launch(h->fly, (hipStream_t)stream, h->state, out_dev, q_dev, configs_per_env, reach, groups, h->cfg.n_envs, h->P.object, env_begin, env_count, flags);
  HIPCHK(h, hipGetLastError());
  return 0;
}

const char* pih_last_error(pih_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

}  // extern "C"
