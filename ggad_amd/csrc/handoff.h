// In-launch hand-offs: every workgroup (or wave) of a launch stores partial results and draws a ticket on a counter in device memory;
// the one whose ticket is last -- whichever it is -- reads all the partials and finishes the job in a fixed order.  Nobody waits, so
// the launch needs no co-residency and replays in a hipGraph.  What can go wrong is SILENT: a partial read from a stale cache line is
// a slightly wrong number, not a fault.  The three forms below follow cdna_hip_programming §6 Guideline 16 (counter form) and are the
// only ones the library uses: a new kernel calls one of them, it does not write a fourth.
//
// The ticket word, all forms: int32 in device memory, ZERO before the first call; the winner puts it back to zero (the fence forms
// with an atomic store; the fence-free form with a plain one, see its body).  Launches that share a word are ordered on
// one stream or in one captured chain.  `count` = number of arrivals, the same in all of them; `flag` = one __shared__ int.
//
// ggad_last_of: workgroup form, plain stores and loads, release / acquire fences.
//   producer  EVERY wave waits for its stores (s_waitcnt vmcnt(0); the barrier waits for no memory counter: without the wait a
//             wave's stores can be in flight when thread 0 fences -- stale under uneven load), the barrier, then ONE thread: the
//             agent-scope release (an L2 write-back: once per workgroup, not per wave), an asm wait BEHIND the fence (the compiler
//             can drop the fence's own: Pitfall 12, "rare stale WITH a release fence"), the ticket.
//   winner    the same thread: agent-scope acquire (drops this compute unit's L1), an asm wait for it, the reset, then the barrier:
//             the wait holds the barrier until the L1 is clean, so one lane's acquire covers the workgroup.  Behind it plain VECTOR
//             loads; the acquire does not clean the scalar cache (Pitfall 6): a word every lane reads alike is read with ld_agent.
// ggad_last_wave_of: the same protocol for kernels whose unit of work is a wave (no barrier, no LDS).  The whole wave fences -- a
//             write-back per wave, so only where few waves hand off.  Without the wait behind the release lane 0's ticket can pass
//             the write-back; without the one behind the acquire the winner's loads can pass the invalidate.
// ggad_last_of_sc1: workgroup form WITHOUT fences, for a kernel that streams out much other data (a release would write all of that
//             back too).  Valid only when (1) every handed-off byte was stored with st_agent* (write-through) and (2) EVERY load of
//             it in the winner is ld_agent* (served by L2 / memory, never by an L1 line of an earlier launch): ONE plain load of
//             such a byte reads stale data, and a test with a cold L1 does not show it.  Every storing wave still waits for its
//             stores before the barrier (Pitfall 14: draining thread 0's wave alone is stale under load).  Measured on hipMalloc
//             memory, not an architectural guarantee; a kernel that cannot keep (1) and (2) uses ggad_last_of.
//
// A ticket that hands over NO data (k_adam_multi: it counts arrivals) needs none of this.  step_xcd.hip (tagged slots between
// resident workgroups) and exchange.cpp (granules between processes) are other protocols, described where they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// agent-scope relaxed accesses (sc1): the store is written through to memory, the load is not served from this compute unit's L1
__device__ __forceinline__ float ld_agent(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent16(float4 *p, float4 v) {
  unsigned long long *q = reinterpret_cast<unsigned long long *>(p);
  __hip_atomic_store(q, ((unsigned long long)__float_as_uint(v.y) << 32) | __float_as_uint(v.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q + 1, ((unsigned long long)__float_as_uint(v.w) << 32) | __float_as_uint(v.z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float4 ld_agent16(const float4 *p) {
  const unsigned long long *q = reinterpret_cast<const unsigned long long *>(p);
  const unsigned long long a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long b = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_float4(__uint_as_float((unsigned)a), __uint_as_float((unsigned)(a >> 32)), __uint_as_float((unsigned)b), __uint_as_float((unsigned)(b >> 32)));
}

// true in the last of `count` workgroups to arrive at `ticket`, after its acquire; called by every thread of the workgroup
__device__ __forceinline__ bool ggad_last_of(int32_t *ticket, int count, int *flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = (t == count - 1) ? 1 : 0;
    if (*flag) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  return *flag != 0;
}

// true in the last of `count` WAVES to arrive at `ticket`, after its acquire; called by every lane of a full wave
__device__ __forceinline__ bool ggad_last_wave_of(int32_t *ticket, int count) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int t = 0;
  if ((threadIdx.x & 63) == 0) t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  t = __shfl(t, 0, 64);
  if (t != count - 1) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// true in the last of `count` workgroups to arrive at `ticket`; NO fence: see the conditions above
__device__ __forceinline__ bool ggad_last_of_sc1(int32_t *ticket, int count, int *flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's write-through stores are acknowledged ...
  __syncthreads();                                   // ... every wave's are: the ticket may be drawn
  if (threadIdx.x == 0) *flag = (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == count - 1) ? 1 : 0;
  __syncthreads();
  if (*flag == 0) return false;
  // a PLAIN reset, as k_prelu_bwd_one always had: nobody adds to this word again before the launch ends, and the end of the launch
  // writes it back.  An atomic (write-through) store here is waited for by the winner's first ld_agent* loads (one vmcnt counter):
  // the TAM epoch at Amazon size, two such launches, went from 0.9069 [0.9066, 0.9075] to 0.9087 [0.9075, 0.9097] ms with it.
  if (threadIdx.x == 0) *ticket = 0;
  return true;
}
