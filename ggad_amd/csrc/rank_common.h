// The device pieces that the two ranking files share, each exactly once: rank_metrics.hip sorts the 32-bit keys of the positives,
// topk.hip the 64-bit (key, position) words of the candidates, and both do it the same way -- runs of RK_RUN words sorted by one
// workgroup each with the bitonic network in LDS, then merged in pairs by rank, ping-pong between two buffers.  (The merge pass itself
// is NOT shared: k_rw_merge needs a lower bound from the left run and an upper bound from the right one, k_tkw_merge's words are
// distinct and one bound serves both sides; one template for both cost ggad_topk_wide_f32 9 to 12 us of 778 at k = 4,194,304 in three
// measurements, profiles/rank_one_chain_time_line.json.)  The two choices behind that are measured (kernel trace at n = 1,736,598):
//   * sorted runs of 2,048 words, not of 8,192: the bitonic network over 8,192 keys is 91 barrier steps of four exchanges per thread,
//     67 us in one workgroup; over 2,048 keys it is 66 steps of one exchange, 23 us, and the two merge passes more cost 5 us each at
//     8,313 positives (13 us each at 2^20, where there are nine passes instead of seven)
//   * the merge is by rank, not by merge path (fixed output spans staged in LDS): a pass is one independent binary search per word in
//     words that stay in L2 -- those 5 and 13 us -- and has no diagonal search and no staging to get wrong
// Everything is in the anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int RK_T = 1024;                // threads of every workgroup of the ranking kernels
constexpr int RK_RUN = 2048;              // words one workgroup sorts: one exchange per thread and step of the network

// order-preserving image of a float (not NaN): a < b <=> key(a) < key(b), and -0.0 ties with +0.0.  The key of a real score is
// never 0 (-inf maps to 0x007FFFFF) and never 0xFFFFFFFF (that is the image of a NaN).
__device__ __forceinline__ uint32_t rk_key(float s) {
  const uint32_t b = s == 0.0f ? 0u : __float_as_uint(s);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

// first index in sorted a[lo, hi) with a[idx] >= key / > key
template <typename W>
__device__ __forceinline__ int rk_lower(const W *a, int lo, int hi, W key) {
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
template <typename W>
__device__ __forceinline__ int rk_upper(const W *a, int lo, int hi, W key) {
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] <= key) lo = mid + 1; else hi = mid; }
  return lo;
}

// The M words (a power of two >= 64) of w[] in LDS sorted ascending by the bitonic network; whole workgroup, the caller's stores to
// w[] need no barrier before it and the sorted words none after it.
template <typename W>
__device__ __forceinline__ void rk_bitonic(W *w, int M) {
  __syncthreads();
  for (int size = 2; size <= M; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < (M >> 1); i += RK_T) {
        const int a = 2 * i - (i & (stride - 1)), b = a + stride;
        const bool up = (a & size) == 0;
        const W x = w[a], y = w[b];
        if ((x > y) == up) { w[a] = y; w[b] = x; }
      }
      __syncthreads();
    }
  }
}

struct RkScan {                            // LDS of the workgroup scans and sums
  int32_t wsum[RK_T / GGAD_WAVE];
  int32_t res[2];
};

// Inclusive scan of one int per thread over the workgroup (shuffles inside a wave, the 16 wave totals through LDS); returns the
// thread's inclusive value, *total the sum of all.
__device__ __forceinline__ int rk_block_scan(RkScan &S, int v, int *total) {
  const int lane = lane_id(), wave = threadIdx.x / GGAD_WAVE;
  int x = v;
#pragma unroll
  for (int d = 1; d < GGAD_WAVE; d <<= 1) {
    const int y = __shfl_up(x, d, GGAD_WAVE);
    if (lane >= d) x += y;
  }
  if (lane == GGAD_WAVE - 1) S.wsum[wave] = x;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < RK_T / GGAD_WAVE; ++w) {
    const int c = S.wsum[w];
    before += w < wave ? c : 0;
    tot += c;
  }
  if (total) *total = tot;
  __syncthreads();                                                             // (the table is free again)
  return x + before;
}

// the sum of one int per thread over the workgroup, for every thread (16 wave totals through LDS, added in wave order)
__device__ __forceinline__ int rk_block_sum(int32_t *s16, int v) {
  v = wave_sum_i(v);
  if (lane_id() == 0) s16[threadIdx.x / GGAD_WAVE] = v;
  __syncthreads();
  int tot = 0;
#pragma unroll
  for (int w = 0; w < RK_T / GGAD_WAVE; ++w) tot += s16[w];
  __syncthreads();
  return tot;
}

}  // namespace
