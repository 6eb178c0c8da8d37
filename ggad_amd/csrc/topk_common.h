// The select stage that topk.hip (ggad_topk_f32) and topk_wide.hip (ggad_topk_wide_f32) share: the workspace layout, the order-preserving
// key, the block scan, and the kernels k_tk_init, k_tk_hist<0..2> and k_tk_select, which find the exact key of rank m - 1 and write the
// m (key, position) candidates in any order (heads of those two files).  Nothing here depends on how many candidates one workgroup can
// sort: every count and slot is an int32 bounded by n <= INT32_MAX, the layout offsets are int64, and the tie table of k_tk_select is
// per chunk of 1,024 positions, not per candidate.  Everything is in the anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int TK_T = 1024;                // threads of every workgroup
constexpr int TK_G = 256;                 // workgroups (= contiguous ranges) of the passes over the scores at most
constexpr int TK_B01 = 2048, TK_B2 = 1024;                                     // bins of digits 0 and 1, of digit 2
constexpr int TK_O_H0 = 0, TK_O_H1 = TK_B01, TK_O_H2 = 2 * TK_B01;            // int32 offsets into the workspace
constexpr int TK_O_CTR = TK_O_H2 + TK_B2;                                      // flags, positives, slots reserved by k_tk_select
constexpr int TK_O_CAND = TK_O_CTR + 16;                                       // keys[k] then positions[k], then the range histograms

struct TkLayout {
  int g;
  int64_t per_block;
  int64_t o_key() const { return TK_O_CAND; }
  int64_t o_pos(int k) const { return o_key() + k; }
  int64_t o_range(int k) const { return o_pos(k) + k; }                        // g rows of TK_B2 ints
  int64_t total(int k) const { return o_range(k) + (int64_t)g * TK_B2; }
};

inline TkLayout tk_layout(int64_t n) {
  TkLayout L;
  int64_t g = (n + TK_T - 1) / TK_T;
  L.g = (int)(g < 1 ? 1 : (g > TK_G ? TK_G : g));
  L.per_block = (n + L.g - 1) / L.g;
  return L;
}

// order-preserving image of a float (not NaN): a < b <=> key(a) < key(b), and -0.0 ties with +0.0 (rm_key of rank_metrics.hip).
// The key of a real score is never 0 (-inf maps to 0x007FFFFF), so 0 pads the sort below everything.
__device__ __forceinline__ uint32_t tk_key(float s) {
  const uint32_t b = s == 0.0f ? 0u : __float_as_uint(s);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

struct TkScan {                            // LDS of the block scans
  int32_t wsum[TK_T / GGAD_WAVE];
  int32_t res[2];
};

// Inclusive scan of one int per thread over the workgroup (shuffles inside a wave, the 16 wave totals through LDS); returns the
// thread's inclusive value, *total the sum of all.
__device__ __forceinline__ int tk_block_scan(TkScan &S, int v, int *total) {
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
  for (int w = 0; w < TK_T / GGAD_WAVE; ++w) {
    const int c = S.wsum[w];
    before += w < wave ? c : 0;
    tot += c;
  }
  if (total) *total = tot;
  __syncthreads();                                                             // (the table is free again)
  return x + before;
}

// The bin that holds the r-th largest element (r = 1 .. sum of hist) of a histogram of nb bins, bins counted from the top, and the
// number of elements in the bins above it.  Whole workgroup; every thread gets both.
__device__ __forceinline__ void tk_pick(TkScan &S, const int32_t *__restrict__ hist, int nb, int r, int &bin, int &above) {
  const int t = threadIdx.x;
  const int per = nb / TK_T;                                                   // 2 or 1 bins per thread, descending
  if (t == 0) { S.res[0] = 0; S.res[1] = 0; }
  int s = 0;
  for (int j = 0; j < per; ++j) s += hist[nb - 1 - (t * per + j)];
  const int incl = tk_block_scan(S, s, nullptr);
  int a = incl - s;
  if (a < r && r <= incl) {                                                    // exactly one thread
    for (int j = 0; j < per; ++j) {
      const int b = nb - 1 - (t * per + j);
      const int c = hist[b];
      if (r <= a + c) { S.res[0] = b; S.res[1] = a; break; }
      a += c;
    }
  }
  __syncthreads();
  bin = S.res[0];
  above = S.res[1];
  __syncthreads();
}

__global__ void __launch_bounds__(TK_T) k_tk_init(int32_t *__restrict__ ws) {
  for (int i = threadIdx.x; i < TK_O_CAND; i += TK_T) ws[i] = 0;
}

template <int PASS>
__global__ void __launch_bounds__(TK_T) k_tk_hist(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n, int m,
                                                  int64_t per_block, int32_t *__restrict__ ws, int32_t *__restrict__ range_hist) {
  constexpr int NB = PASS == 2 ? TK_B2 : TK_B01;
  __shared__ int32_t h[NB];
  __shared__ TkScan S;
  __shared__ int32_t s_cnt[2];
  if (m == 0) return;
  const int t = threadIdx.x;
  for (int i = t; i < NB; i += TK_T) h[i] = 0;
  if (t < 2) s_cnt[t] = 0;
  uint32_t want = 0;                                                           // the digits above this pass's of rank m - 1
  if (PASS >= 1) {
    int d0, a0;
    tk_pick(S, ws + TK_O_H0, TK_B01, m, d0, a0);
    want = (uint32_t)d0;
    if (PASS == 2) {
      int d1, a1;
      tk_pick(S, ws + TK_O_H1, TK_B01, m - a0, d1, a1);
      want = ((uint32_t)d0 << 11) | (uint32_t)d1;
    }
  }
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * per_block;
  const int64_t hi = lo + per_block < n ? lo + per_block : n;
  int flags = 0, pos = 0;
  for (int64_t i = lo + t; i < hi; i += TK_T) {
    const float s = score[i];
    const uint32_t key = tk_key(s);
    if (PASS == 0) {
      if (s != s) flags |= 1;
      if (label) {
        const int y = label[i];
        if (y > 1) flags |= 2;
        pos += y == 1;
      }
      atomicAdd(&h[key >> 21], 1);
    } else if (PASS == 1) {
      if ((key >> 21) == want) atomicAdd(&h[(key >> 10) & 2047u], 1);
    } else {
      if ((key >> 10) == want) atomicAdd(&h[key & 1023u], 1);
    }
  }
  if (PASS == 0) {
    pos = wave_sum_i(pos);
    if (lane_id() == 0 && pos) atomicAdd(&s_cnt[1], pos);
    if (flags) atomicOr(&s_cnt[0], flags);
  }
  __syncthreads();
  int32_t *gh = ws + (PASS == 0 ? TK_O_H0 : PASS == 1 ? TK_O_H1 : TK_O_H2);
  for (int i = t; i < NB; i += TK_T) {
    const int c = h[i];
    if (c) atomicAdd(&gh[i], c);
    if (PASS == 2) range_hist[(int64_t)blockIdx.x * TK_B2 + i] = c;
  }
  if (PASS == 0) {                                                             // one atomic per workgroup and word
    if (t == 0 && s_cnt[0]) atomicOr(&ws[TK_O_CTR + 0], s_cnt[0]);
    if (t == 1 && s_cnt[1]) atomicAdd(&ws[TK_O_CTR + 1], s_cnt[1]);
  }
}

__global__ void __launch_bounds__(TK_T) k_tk_select(const float *__restrict__ score, int64_t n, int m, int64_t per_block,
                                                    int32_t *__restrict__ ws, const int32_t *__restrict__ range_hist,
                                                    uint32_t *__restrict__ ckey, int32_t *__restrict__ cpos) {
  __shared__ TkScan S;
  __shared__ int32_t s_i[4];                                                   // ties before this range, keys above T here, slot base, slots given out
  __shared__ int32_t s_wc[TK_T / GGAD_WAVE];
  if (m == 0) return;
  const int t = threadIdx.x, lane = lane_id(), wave = t / GGAD_WAVE;
  if (t < 4) s_i[t] = 0;
  int d0, a0, d1, a1, d2, a2;
  tk_pick(S, ws + TK_O_H0, TK_B01, m, d0, a0);
  tk_pick(S, ws + TK_O_H1, TK_B01, m - a0, d1, a1);
  tk_pick(S, ws + TK_O_H2, TK_B2, m - a0 - a1, d2, a2);
  const uint32_t T = ((uint32_t)d0 << 21) | ((uint32_t)d1 << 10) | (uint32_t)d2;
  const int G = a0 + a1 + a2;                                                  // keys above T among all n (< m)
  const int need = m - G;                                                      // ties of T to take, lowest positions first (>= 1)
  const int64_t lo = (int64_t)blockIdx.x * per_block;
  const int64_t hi = lo + per_block < n ? lo + per_block : n;
  // ties in the ranges before this one (at most 255 words), keys above T in this range
  if (t < (int)blockIdx.x) { const int c = range_hist[(int64_t)t * TK_B2 + d2]; if (c) atomicAdd(&s_i[0], c); }
  int gt = 0;
  for (int64_t i = lo + t; i < hi; i += TK_T) gt += tk_key(score[i]) > T;
  gt = wave_sum_i(gt);
  if (lane == 0 && gt) atomicAdd(&s_i[1], gt);
  __syncthreads();
  if (t == 0 && s_i[1]) s_i[2] = atomicAdd(&ws[TK_O_CTR + 2], s_i[1]);
  __syncthreads();
  const int before = s_i[0], gbase = s_i[2];
  const bool ties_here = before < need && range_hist[(int64_t)blockIdx.x * TK_B2 + d2] > 0;       // (uniform)
  if (s_i[1] == 0 && !ties_here) return;
  int run = before;
  for (int64_t base = lo; base < hi; base += TK_T) {                           // whole workgroup, chunks in position order
    const int64_t i = base + t;
    uint32_t key = 0;
    if (i < hi) key = tk_key(score[i]);
    const bool is_gt = i < hi && key > T;
    const unsigned long long mg = __ballot(is_gt);
    if (mg) {                                                                  // one LDS atomic per wave that holds any
      const int leader = __ffsll(mg) - 1;
      int slot0 = 0;
      if (lane == leader) slot0 = atomicAdd(&s_i[3], __popcll(mg));
      slot0 = __shfl(slot0, leader, GGAD_WAVE);
      const int slot = gbase + slot0 + __popcll(mg & ((1ull << lane) - 1ull));
      if (is_gt && slot < G) { ckey[slot] = key; cpos[slot] = (int32_t)i; }
    }
    if (ties_here) {
      const bool is_tie = i < hi && key == T;
      const unsigned long long mt = __ballot(is_tie);
      if (lane == 0) s_wc[wave] = __popcll(mt);
      __syncthreads();
      int off = run, tot = 0;
      for (int w = 0; w < TK_T / GGAD_WAVE; ++w) { const int c = s_wc[w]; if (w < wave) off += c; tot += c; }
      if (is_tie) {
        const int r = off + __popcll(mt & ((1ull << lane) - 1ull));            // rank of this element among ALL ties of T
        if (r < need) { ckey[G + r] = key; cpos[G + r] = (int32_t)i; }
      }
      run += tot;
      __syncthreads();
    }
  }
}

}  // namespace
