// pih_mailbox.h -- the handshake of the fused launch (round 4): the controller wavefronts and the step wavefronts of ONE grid meet
// through a mailbox in HBM.  Used by both tasks: pih_step_kernel (reader: Wave::await_controller, pih_wave.h) and pih_fly_step_kernel
// (reader: MailboxIk, pih_fly.hip); the host side (allocation, per-launch epoch and error check) is mailbox_alloc / next_epoch of pih_hip.hip.
//
// A controller wavefront computes the outputs of its group of 64 envs, stores them into the mailbox (mail_store) and publishes the group
// with mailbox_publish: the launch's epoch goes into the group's flag.  A step wavefront waits for that flag (mailbox_await), then reads
// its env's words (mail_load).  Every launch has a new epoch, so no flag is ever cleared.
//
// Memory model.  Flag and mailbox words are RELAXED agent-scope atomics: stores and loads that are coherent across the chip's eight L2s
// by themselves (sc1).  An agent-scope acquire would invalidate, and an agent-scope release write back, the whole L2 of the XCD --
// measured: + 50 us per launch with 4 096 acquires -- which write-through stores do not need.  What orders the
// two sides:
//   * publish: the mailbox stores of all 64 lanes are acknowledged before the flag store -- an explicit  s_waitcnt vmcnt(0), then the
//     barrier, then lane 0 stores the flag.  The workgroup-scope release fence alone compiles to NO wait (the waves of a workgroup share
//     their CU's L1, so the memory model needs none for that scope), and the flag store then overtook mailbox stores still in flight:
//     with 640+ workgroups in a random-fly launch a step wavefront read one stale target word in ~ 1 of 200 groups (tests/test_gpu_fly.py,
//     12 000 envs);
//   * await: the wave reads the mailbox only after it has seen the flag.  The wait is wave-uniform and bounded (s_sleep between polls):
//     on time-out the error word -- pinned host memory mapped into the device -- is set and the step goes on with the values it has, so
//     a launch never hangs on this; the next pih_step on the handle returns -5.
// gfx950 only (the host harness of tests/emul has no fused launch).
#pragma once

namespace pih {

__device__ __forceinline__ void mail_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float mail_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// controller workgroup, all lanes, after their mail_store: publish the group of workgroup blockIdx.x
__device__ __forceinline__ void mailbox_publish(int* flags, int epoch) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flags + blockIdx.x, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// step wavefront: wait until the group's flag holds this launch's epoch; on time-out the lanes with `report` set the error word
__device__ __forceinline__ void mailbox_await(const int* flag, int epoch, int* err, bool report) {
  int tries = 0;
  while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < epoch) {
    __builtin_amdgcn_s_sleep(4);
    if (++tries > (1 << 21)) { if (report) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace pih
