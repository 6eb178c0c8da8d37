// Shared helpers for the gfx950 kernels of libggad_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include "../../include/ggad_hip.h"

#define GGAD_WAVE 64
#define GGAD_MAX_D 64    // embedding width handled by one wave (lane = channel)
#define GGAD_MAX_F 1024  // feature width limit of the gather kernels

void ggad_set_error(hipError_t e, const char *where);

#define GGAD_CHECK_LAUNCH(where)                 \
  do {                                           \
    hipError_t _e = hipGetLastError();           \
    if (_e != hipSuccess) {                      \
      ggad_set_error(_e, where);                 \
      return GGAD_E_LAUNCH;                      \
    }                                            \
  } while (0)

#define GGAD_REQUIRE(cond) \
  do {                     \
    if (!(cond)) return GGAD_E_INVALID; \
  } while (0)

static inline hipStream_t as_stream(ggad_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// More than 64 KB of dynamic LDS is a per-DEVICE attribute of a kernel: set -- and its result checked -- once per device of the
// process, under the mutex of the site (one static ggad_lds_optin per site).  `kernels` all get `bytes`.  1 = ready, -1 = this device
// refused (remembered), 0 = no usable current device; each site reacts in its own way.
struct ggad_lds_optin {
  std::mutex mu;
  int state[64] = {};
};
template <typename... K>
static inline int ggad_lds_opt_in(ggad_lds_optin &S, int bytes, K... kernels) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  std::lock_guard<std::mutex> lock(S.mu);
  if (S.state[dev] == 0) {
    const bool ok = ((hipFuncSetAttribute((const void *)kernels, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) && ...);
    (void)hipGetLastError();
    S.state[dev] = ok ? 1 : -1;
  }
  return S.state[dev];
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (GGAD_WAVE - 1); }

// Sum over the 64 lanes of a wave; every lane gets the result.  Fixed butterfly order,
// so the value is deterministic for given inputs.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, GGAD_WAVE);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, GGAD_WAVE);
  return v;
}

// k_adam_multi's update of one element (fullgraph.hip), expression for expression: torch's Adam with L2 weight decay, betas .9 / .999,
// eps 1e-8; sc0 = lr / (1 - .9^t) and sc1 = sqrt(1 - .999^t) are formed in double by the caller.  Shared by the kernels that apply
// Adam inside a fused step (recon_mb.hip, sage.hip).
__device__ __forceinline__ void ggad_adam_elem(float &pi, float &mi, float &vi, float g, float wd, float sc0, float sc1) {
  float gi = fmaf(wd, pi, g);
  mi = fmaf(gi - mi, 0.1f, mi);
  vi = fmaf(0.001f * gi, gi, vi * 0.999f);
  const float denom = sqrtf(vi) / sc1 + 1e-8f;
  pi = pi - sc0 * (mi / denom);
}

// first index in sorted a[lo,hi) with a[idx] >= key
__device__ __forceinline__ int lower_bound_i32(const int32_t *__restrict__ a, int lo, int hi, int key) {
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- plan launches that leave one XCD alone.  The dispatcher deals the workgroups of a launch to the eight XCDs in strict rotation
// (block b runs on XCD (first + b) % 8, `first` a constant of the stream: scripts/xcd_block_map.hip).  While the XCD-resident chunk
// kernel (step_xcd.hip) owns an XCD, the plan kernels of the next chunk run on the other seven: launched with ggad_skip_grid(n)
// workgroups, every eighth one -- blockIdx.x % 8 == skip, the ones the dispatcher would put on that XCD -- returns at once and the
// others number themselves 0 .. n' - 1 (n' >= n: every kernel bounds-checks what it derives from the number).  Which blocks are
// skipped is decided by INDEX, so the results never depend on the placement; only the speed does.  skip < 0: plain launch.
__device__ __forceinline__ bool ggad_vblock(int skip, unsigned &vb, unsigned &vg) {
  const unsigned b = blockIdx.x, n = gridDim.x;
  if (skip < 0) { vb = b; vg = n; return true; }
  const unsigned sk = (unsigned)skip;
  if ((b & 7u) == sk) return false;
  vb = b - ((b >> 3) + ((b & 7u) > sk ? 1u : 0u));
  vg = n - ((n >> 3) + ((n & 7u) > sk ? 1u : 0u));
  return true;
}
static inline unsigned ggad_skip_grid(unsigned want, int skip) { return skip < 0 ? want : (unsigned)(((uint64_t)(want + 1) * 8 + 6) / 7); }

// ---- internal (C++ linkage) pieces of ggad_mb_plan_build, shared between plan_build.cpp, plan.hip and hop2_ldsw.hip
// counters[] of a plan: every counter on a 64-byte line of its own.  A device-scope atomic on ONE address (or line) completes every
// ~7 ns whoever issues it (measured: 43 K wave-level atomics = 313 us of k_build_groups), so the plan kernels reserve storage
// once per WORKGROUP (wg_reserve below), not once per wave, and the work-item cursor of the 2-hop gather is bumped by big grabs.
constexpr int GGAD_CTR_STRIDE = 16;
constexpr int GGAD_CTR_GROUPS = 0 * GGAD_CTR_STRIDE, GGAD_CTR_ITEMS = 1 * GGAD_CTR_STRIDE, GGAD_CTR_PART = 2 * GGAD_CTR_STRIDE,
              GGAD_CTR_CURSOR = 3 * GGAD_CTR_STRIDE, GGAD_CTR_PC = 4 * GGAD_CTR_STRIDE,
              GGAD_CTR_BIG = 5 * GGAD_CTR_STRIDE,          // groups of range-partitioned owners (hop2_ldsw.hip)
              GGAD_CTR_RANGE0 = 6 * GGAD_CTR_STRIDE,       // .. 13: the work cursor of each of the eight id ranges
              GGAD_CTR_PROF = 14 * GGAD_CTR_STRIDE;        // 14, 15: phase clocks of a -DGGAD_G2_PROF build (16 x 64 bits)
constexpr int GGAD_RANGES = 8;            // id ranges of the 2-hop gather: one per XCD, so that each L2 keeps an eighth of the hot rows
constexpr int GGAD_RANGE_DEG = 256;       // owners with more neighbours than this are gathered range by range
constexpr int GGAD_PLAN_COUNTERS = 16 * GGAD_CTR_STRIDE;      // ints of ggad_mb_plan::counters

struct ggad_plan_view {      // device views into the staging block of ONE build + its exact sizes (known on the host)
  const int32_t *batch_ptr, *batch_ent_ptr, *nodes, *row_slot, *ent_ptr, *row_ck_ptr, *ck_rc, *ck_e0;
  int32_t n_batches, n_rows, n_ents, n_chunks;
  int32_t seg_stride;        // entries per tile row of seg_t (n_ents rounded up to 64)
  int64_t pair_bound;        // host bound on the (owner, neighbour) pairs of THIS build (the capacities may be far larger)
};
int ggad_int_hop1(const ggad_mb_plan *P, const ggad_plan_view &V, int ldsw, int reset_now, hipStream_t st);
int ggad_int_global_hop2(const ggad_mb_plan *P, const ggad_plan_view &V, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
int ggad_int_ldsw_hop2(const ggad_mb_plan *P, const ggad_plan_view &V, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
int ggad_int_range_deg();      // owners above this degree are gathered by id range (INT32_MAX: the partition is off)

// ---- gemm_slab.hip: the slab-resident tall product; 1 = launched, 0 = not this kernel's shape, < 0 = launch error
int ggad_int_gemm_slab(const float *A, const float *B, float *C, int M, int N, int K, int64_t lda, int64_t sbk, int64_t sbn, int64_t ldc,
                       const float *bias, int relu, hipStream_t st, const float *prelu_a = nullptr, float *C2 = nullptr, int64_t ldc2 = 0);

// ---- mlp.hip: D (m x n) = P^T Q over R rows as row-range partials + ordered reduction (the weight gradients); 1 = launched, 0 = not taken
int64_t ggad_int_wgrad_tn_ws(int R, int m, int n);
int ggad_int_wgrad_tn(const float *P, int64_t ldp, const float *Q, int64_t ldq, int R, int m, int n, float *D, float *ws, hipStream_t st,
                      int *vpq = nullptr);      // vpq: GGAD_GEMM_VARIANT_TN(vp, vq) of the launch, for ggad_gemm_last_route

// ---- step_wide.hip: the layered step chain for 64 < D <= 256 (and chain 3 at any D <= 256); arguments and buffer contracts of the
// ggad_mb_* entry points of the same names (step.hip forwards to these)
constexpr int GGAD_MB_BWD_PARTS = 256;           // partial dW blocks of bwd_flat (both variants: ggad_mb_bwd_parts())
struct ggad_xchg_view;
bool ggad_int_wide_ok(int D, int F);
int ggad_int_wide_project(const float *params, int32_t D, int32_t F, const float *x2, const int32_t *ent_own, int32_t ent0,
                          int32_t n_ents, float *h2, ggad_stream_t stream);
int ggad_int_wide_fwd_rows(const float *params, int32_t D, int32_t F, const float *x1, const float *h2, const int32_t *ent_ptr,
                           const int32_t *ent_own, const int32_t *labels, int32_t row0, int32_t n_rows, int32_t ent0, float *h1,
                           float *nbar, float *gen, ggad_stream_t stream);
int ggad_int_wide_loss(const float *params, int32_t D, int32_t F, const float *h1, const float *nbar, const float *gen,
                       const int32_t *labels, const int32_t *pos_meta, const int32_t *row_pos, const int32_t *ent_ptr,
                       int32_t row0, int32_t n_rows, float *loss_ws, float *losses8, float *d_h1, float *d_gen, float *d_nbar,
                       float *dz, float *coef_a, float *coef_g, int32_t *step_counter, ggad_stream_t stream);
int ggad_int_wide_row_coefs(const float *params, int32_t D, int32_t F, const int32_t *labels, const int32_t *ent_ptr,
                            int32_t row0, int32_t n_rows, const float *h1, const float *gen, const float *d_h1,
                            const float *d_gen, const float *d_nbar, float *dz, float *coef_a, float *coef_g,
                            ggad_stream_t stream);
int ggad_int_wide_bwd_flat(int32_t D, int32_t F, const float *x1, const float *x2, const float *h2, const int32_t *ent_own,
                           const int32_t *ent_row, int32_t row0, int32_t n_rows, int32_t ent0, int32_t n_ents,
                           const float *coef_a, const float *coef_g, float *dw_part, ggad_stream_t stream);
int ggad_int_wide_grad_reduce(int32_t D, int32_t F, const int32_t *pos_meta, int32_t row0, int32_t n_rows, const float *losses8,
                              const float *nbar, const float *dw_part, const float *dz, const float *loss_ws, float *grads,
                              int mode, float *params, float *m, float *v, float lr, float wd, const int32_t *step_counter,
                              const ggad_xchg_view *xv, uint32_t xstep, float grad_scale, ggad_stream_t stream);
int ggad_int_wide_rows(const float *params, int32_t D, int32_t F, const float *x1, int32_t n_rows, float *out, int score,
                       ggad_stream_t stream);

// ---- one-shot gradient exchange (exchange.cpp owns the handle, step.hip the kernel)
constexpr int GGAD_XCHG_MAX_WORLD = 16;
struct ggad_xchg_view {                          // what the kernel needs, passed by value
  float *peer[GGAD_XCHG_MAX_WORLD];             // peer[q] = rank q's buffer as mapped into THIS process (peer[rank] = own)
  int32_t rank, world;
  int64_t n;                                     // floats per slot
  int32_t *err;                                  // device word: set when a wait timed out
  unsigned long long timeout_ticks;              // bound of a wait in 100 MHz wall-clock ticks (GGAD_XCHG_TIMEOUT_S, default 20 s)
};
struct ggad_xchg {
  ggad_xchg_view view;
  void *local;                                   // own buffer (fine-grained device memory)
  size_t bytes;
  uint32_t step;                                 // exchanges done so far (all ranks call in lockstep)
  bool opened[GGAD_XCHG_MAX_WORLD];
};
static inline size_t ggad_xchg_granules(int world, int64_t n) { return (size_t)2 * world * (size_t)n; }   // 8 bytes each: {value, step}
