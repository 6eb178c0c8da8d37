// Exact, deterministic top-k of float32 scores: the k highest scores of n, ranked by score descending and, among equal scores, by
// ascending position in the input (-0.0 ties with +0.0, +-inf are ordinary values, a NaN anywhere is reported in the status word);
// beside them the running count of label-1 elements along the ranking (precision / recall @ j), the positives among all n, and how
// many elements tie with the last rank but were left out.  No host synchronisation, integer atomics only, nothing that waits on
// another workgroup; equal inputs give equal bits in every output.  Two entry points share the select stage: ggad_topk_f32
// (k <= TK_CAP = 16,384) sorts the candidates in one workgroup, ggad_topk_wide_f32 (k <= TKW_CAP = 4,194,304) in runs that are merged;
// where both serve, every output holds the same bits.
//
// The 32-bit order-preserving key of a score is cut into three digits (11 + 11 + 10 bits, most significant first).  With m = min(k, n)
// and R = ceil(m / 2,048) the launches on one stream are
//   k_tk_init     one workgroup: clears the three global histograms and the counters
//   k_tk_hist<0>  TK_G workgroups over contiguous ranges: histogram of digit 0 in LDS, flushed with integer atomics; NaN / label flags
//                 and the positives among all n
//   k_tk_hist<1>  every workgroup re-derives from histogram 0 the digit 0 of rank m - 1 (a block scan over 2,048 bins), then
//                 histogram of digit 1 over the elements that share it
//   k_tk_hist<2>  the same one level down: histogram of digit 2 over the elements that share digits 0 and 1; every workgroup also
//                 stores the histogram of ITS range (plain stores), which is what orders the ties later
//   k_tk_select   the three digits give the exact key T of rank m - 1, the count G of keys above T and need = m - G ties to take.
//                 Keys above T are appended in any order (one global atomic per workgroup reserves its slots); the keys equal to T
//                 are taken by lowest position: the per-range counts of bin T give each range its offset, and a range writes its
//                 ties in position order (chunks of 1,024 consecutive elements, ballots and a 16-entry table per chunk).  Nothing
//                 up to here depends on m: every count and slot is an int32 bounded by n <= INT32_MAX, the layout offsets are int64
// then for ggad_topk_f32, six launches in all,
//   k_tk_sort     one workgroup: the m (key, position) pairs as 64-bit words in LDS, bitonic network (a total order, so the append
//                 order above cannot show; up to three strides per pass over LDS), scores and labels gathered, labels prefix-summed,
//                 out_meta
// and for ggad_topk_wide_f32
//   k_tkw_runs    R workgroups.  Run r packs candidates [2,048 r, ...) into 64-bit words (~key << 32) | position, whose ASCENDING
//                 unsigned order is "key descending, position ascending" = the ranking (a total order, so the append order above
//                 cannot show), pads with ~0 (above every word: a key is never 0), and sorts them with the bitonic network of
//                 rank_common.h in 16 KB of static LDS
//   k_tkw_merge   ceil(log2(R)) passes, ping-pong between two word buffers, one thread per word: a word's place in the merged pair of
//                 runs is its index in its own run plus its rank in the partner run.  Positions are distinct, so the words are, and
//                 one lower bound serves both sides.  An unpaired last run is copied through, so the ranking always ends in the
//                 buffer the pass count names
//   k_tkw_emit    one thread per output slot: out_pos, out_score = score[pos], the padding beyond m; with out_cumpos the 0/1 label of
//                 the rank is parked in out_cumpos and the label-1 ranks of each block of 1,024 are stored with plain stores
//   k_tkw_cum     workgroup b sums the block counts before it (at most 4,096 ints, a fixed order), scans its own 1,024 parked labels
//                 and writes out_cumpos, padding included; workgroup 0 writes out_meta
// 5 + 1 + ceil(log2(R)) + 2 launches: 19 at the wide cap.  Every word a launch reads was written by the host or by an earlier launch
// of the same call: a workspace of arbitrary bits needs no preparation, and either call is captured and replayed as one linear chain.
//
// Workspace, in int32 elements: the select stage's tk_layout(n).total(k); the wide call adds, with W = max(m, 1), 2 buffers x 2 W
// (the 64-bit words) + ceil(W / 1,024) block counts.  At n >= k = 2^22 that is 32 MB of candidates + 64 MB of words + 16 KB of counts.
//
// Why k_tk_sort stays although the runs are twice as fast at k = 16,384: up to k = 1,000 the public call through it is 12 us (a tenth)
// shorter, two launches fewer (profiles/rank_one_chain_time_line.json).
#include "rank_common.h"

namespace {

constexpr int TK_T = RK_T;                // threads of every workgroup
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

// The bin that holds the r-th largest element (r = 1 .. sum of hist) of a histogram of nb bins, bins counted from the top, and the
// number of elements in the bins above it.  Whole workgroup; every thread gets both.
__device__ __forceinline__ void tk_pick(RkScan &S, const int32_t *__restrict__ hist, int nb, int r, int &bin, int &above) {
  const int t = threadIdx.x;
  const int per = nb / TK_T;                                                   // 2 or 1 bins per thread, descending
  if (t == 0) { S.res[0] = 0; S.res[1] = 0; }
  int s = 0;
  for (int j = 0; j < per; ++j) s += hist[nb - 1 - (t * per + j)];
  const int incl = rk_block_scan(S, s, nullptr);
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
  __shared__ RkScan S;
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
    const uint32_t key = rk_key(s);
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
  __shared__ RkScan S;
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
  for (int64_t i = lo + t; i < hi; i += TK_T) gt += rk_key(score[i]) > T;
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
    if (i < hi) key = rk_key(score[i]);
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

// out_meta = {m, status, positives among all n, elements that tie with rank m - 1 and were left out}, from the select stage's words.
// Whole workgroup.
__device__ __forceinline__ void tk_write_meta(RkScan &S, const int32_t *__restrict__ ws, int m, int64_t *__restrict__ out_meta) {
  int left_out = 0;
  if (m > 0) {
    int d0, a0, d1, a1, d2, a2;
    tk_pick(S, ws + TK_O_H0, TK_B01, m, d0, a0);
    tk_pick(S, ws + TK_O_H1, TK_B01, m - a0, d1, a1);
    tk_pick(S, ws + TK_O_H2, TK_B2, m - a0 - a1, d2, a2);
    left_out = ws[TK_O_H2 + d2] - (m - a0 - a1 - a2);
  }
  if (threadIdx.x == 0) {
    const int flags = m > 0 ? ws[TK_O_CTR + 0] : 0;
    out_meta[0] = m;
    out_meta[1] = (flags & 2) ? 4 : (flags & 1) ? 3 : 0;
    out_meta[2] = m > 0 ? ws[TK_O_CTR + 1] : 0;
    out_meta[3] = left_out;
  }
}

// ---- ggad_topk_f32: the candidates sorted, emitted and prefix-summed by ONE workgroup
constexpr int TK_CAP = 16384;             // k at most: 16,384 (key, position) pairs of 8 bytes = 128 KB of the 160 KB LDS
constexpr int TK_SORT_LDS = TK_CAP * 8;

// C consecutive compare-exchange steps of the bitonic network (strides low << (C - 1) .. low of the stage `size`) in one pass over
// LDS: a thread takes the 2^C elements base + e * low, which those steps only pair among themselves, and runs the steps in
// registers.  The direction depends on the bit `size` of the index alone, which lies above every bit that varies inside a group.
template <int C>
__device__ __forceinline__ void tk_trip(unsigned long long *lds, int M, int size, int low) {
  constexpr int E = 1 << C;
  const int lg = __ffs(low) - 1;
  for (int g = threadIdx.x; g < (M >> C); g += TK_T) {
    const int base = ((g >> lg) << (lg + C)) | (g & (low - 1));
    const bool down = (base & size) == 0;
    unsigned long long v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = lds[base + e * low];
#pragma unroll
    for (int s = C - 1; s >= 0; --s) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if ((e >> s) & 1) continue;
        const unsigned long long x = v[e], y = v[e | (1 << s)];
        const bool sw = (x < y) == down;
        v[e] = sw ? y : x;
        v[e | (1 << s)] = sw ? x : y;
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) lds[base + e * low] = v[e];
  }
}

__global__ void __launch_bounds__(TK_T) k_tk_sort(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n, int k,
                                                  int m, int M, const int32_t *__restrict__ ws, const uint32_t *__restrict__ ckey,
                                                  const int32_t *__restrict__ cpos, int32_t *__restrict__ out_pos,
                                                  float *__restrict__ out_score, int32_t *__restrict__ out_cumpos,
                                                  int64_t *__restrict__ out_meta) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long tk_lds[];  // (key << 32) | ~position: descending = the ranking
  __shared__ RkScan S;
  const int t = threadIdx.x;
  int total = 0;
  if (m > 0) {
    for (int i = t; i < M; i += TK_T)
      tk_lds[i] = i < m ? ((unsigned long long)ckey[i] << 32) | (unsigned long long)(~(uint32_t)cpos[i]) : 0ull;
    __syncthreads();
    for (int size = 2; size <= M; size <<= 1) {                               // descending: up to three strides per pass over LDS
      int stride = size >> 1;
      while (stride > 0) {
        if (stride >= 4) { tk_trip<3>(tk_lds, M, size, stride >> 2); stride >>= 3; }
        else if (stride == 2) { tk_trip<2>(tk_lds, M, size, 1); stride = 0; }
        else { tk_trip<1>(tk_lds, M, size, 1); stride = 0; }
        __syncthreads();
      }
    }
    for (int idx = t; idx < m; idx += TK_T) {                                  // independent gathers; the label takes the entry's place
      const uint32_t p = ~(uint32_t)tk_lds[idx];
      const bool ok = (int64_t)p < n;                                          // (always; a guard for the gathers)
      out_pos[idx] = ok ? (int32_t)p : -1;
      out_score[idx] = ok ? score[p] : 0.0f;
      tk_lds[idx] = (ok && label) ? (unsigned long long)(label[p] == 1) : 0ull;
    }
    __syncthreads();
    const int ch = M > TK_T ? M / TK_T : 1;                                    // consecutive ranks of one thread
    int local = 0;
    for (int j = 0; j < ch; ++j) {
      const int idx = t * ch + j;
      if (idx < m) local += (int)tk_lds[idx];
    }
    int run = rk_block_scan(S, local, &total) - local;
    if (out_cumpos) {
      for (int j = 0; j < ch; ++j) {
        const int idx = t * ch + j;
        if (idx >= m) break;
        run += (int)tk_lds[idx];
        out_cumpos[idx] = run;
      }
    }
  }
  for (int j = m + t; j < k; j += TK_T) {
    out_pos[j] = -1;
    out_score[j] = 0.0f;
    if (out_cumpos) out_cumpos[j] = total;
  }
  tk_write_meta(S, ws, m, out_meta);
}

// ---- ggad_topk_wide_f32: the candidates sorted in runs and merged
constexpr int TKW_CAP = 1 << 22;          // k at most: one call ranks every node of DGraph-Fin (3,700,550); 2,048 runs, 11 merge passes
constexpr int TKW_RUN = RK_RUN;           // words one workgroup sorts: 16 KB of LDS

struct TkwLayout {                        // int32 offsets behind the select stage's words; o_buf is even, so the words are 8-byte aligned
  TkLayout sel;
  int m, runs, passes, blocks;
  int64_t words, o_buf0, o_buf1, o_cnt, total;
};

static_assert(TK_O_CAND % 2 == 0 && TK_B2 % 2 == 0, "the word buffers start on an even int32 offset");

TkwLayout tkw_layout(int64_t n, int k) {
  TkwLayout L;
  L.sel = tk_layout(n);
  L.m = (int)(n < k ? n : k);
  L.runs = (L.m + TKW_RUN - 1) / TKW_RUN;
  L.passes = 0;
  while ((1 << L.passes) < L.runs) ++L.passes;
  L.words = L.m > 1 ? L.m : 1;
  L.blocks = (int)((L.words + TK_T - 1) / TK_T);
  L.o_buf0 = L.sel.total(k);
  L.o_buf1 = L.o_buf0 + 2 * L.words;
  L.o_cnt = L.o_buf1 + 2 * L.words;
  L.total = L.o_cnt + L.blocks;
  return L;
}

bool tkw_args_ok(int64_t n, int64_t k) { return n >= 0 && n <= INT32_MAX && k >= 1 && k <= TKW_CAP; }

__global__ void __launch_bounds__(TK_T) k_tkw_runs(const uint32_t *__restrict__ ckey, const int32_t *__restrict__ cpos, int m,
                                                   unsigned long long *__restrict__ out) {
  __shared__ unsigned long long w[TKW_RUN];
  const int t = threadIdx.x;
  const int base = blockIdx.x * TKW_RUN;                                       // (< m: the grid is ceil(m / TKW_RUN))
  const int len = m - base < TKW_RUN ? m - base : TKW_RUN;
  int M = 64;
  while (M < len) M <<= 1;
  for (int i = t; i < M; i += TK_T)
    w[i] = i < len ? ((unsigned long long)(~ckey[base + i]) << 32) | (unsigned long long)(uint32_t)cpos[base + i] : ~0ull;
  rk_bitonic(w, M);
  for (int i = t; i < len; i += TK_T) out[base + i] = w[i];
}

// one pass: runs of `width` words of src[0, m) merged in pairs into dst[0, m)
__global__ void __launch_bounds__(TK_T) k_tkw_merge(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst,
                                                    int m, int width) {
  const int i = blockIdx.x * TK_T + threadIdx.x;
  if (i >= m) return;
  const unsigned long long word = src[i];
  const int base = (i / (2 * width)) * (2 * width);                            // (2 * width <= 2^22)
  const int mid = base + width;
  if (mid >= m) { dst[i] = word; return; }                                     // an unpaired run: carried through
  const int end = mid + width < m ? mid + width : m;
  int lo = i < mid ? mid : base, hi = i < mid ? end : mid;                      // the partner run; first index there with src[idx] > word
  const int first = lo;
  while (lo < hi) { const int c = (lo + hi) >> 1; if (src[c] < word) lo = c + 1; else hi = c; }
  dst[base + (i < mid ? i - base : i - mid) + (lo - first)] = word;
}

__global__ void __launch_bounds__(TK_T) k_tkw_emit(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n, int k,
                                                   int m, const unsigned long long *__restrict__ ranked, int32_t *__restrict__ out_pos,
                                                   float *__restrict__ out_score, int32_t *__restrict__ out_cumpos,
                                                   int32_t *__restrict__ cnt) {
  __shared__ int32_t s16[TK_T / GGAD_WAVE];
  const int j = blockIdx.x * TK_T + threadIdx.x;                               // (k <= 2^22)
  int y = 0;
  if (j < m) {
    const uint32_t p = (uint32_t)ranked[j];
    const bool ok = (int64_t)p < n;                                            // (always; a guard for the gathers)
    out_pos[j] = ok ? (int32_t)p : -1;
    out_score[j] = ok ? score[p] : 0.0f;
    y = (ok && label) ? (int)(label[p] == 1) : 0;
    if (out_cumpos) out_cumpos[j] = y;                                         // parked for k_tkw_cum, which overwrites it
  } else if (j < k) {
    out_pos[j] = -1;
    out_score[j] = 0.0f;
  }
  if (out_cumpos && (int)blockIdx.x * TK_T < m) {                              // (uniform)
    const int tot = rk_block_sum(s16, y);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
  }
}

__global__ void __launch_bounds__(TK_T) k_tkw_cum(const int32_t *__restrict__ ws, int k, int m, const int32_t *__restrict__ cnt,
                                                  int32_t *__restrict__ out_cumpos, int64_t *__restrict__ out_meta) {
  __shared__ RkScan S;
  __shared__ int32_t s16[TK_T / GGAD_WAVE];
  const int t = threadIdx.x;
  if (out_cumpos) {
    const int nb = (m + TK_T - 1) / TK_T;                                      // blocks of ranks that hold any (<= 4,096)
    const int upto = (int)blockIdx.x < nb ? (int)blockIdx.x : nb;
    int s = 0;
    for (int i = t; i < upto; i += TK_T) s += cnt[i];
    const int before = rk_block_sum(s16, s);
    const int j = blockIdx.x * TK_T + t;
    const int y = j < m ? out_cumpos[j] : 0;
    int tot = 0;
    const int incl = rk_block_scan(S, y, &tot);
    if (j < m) out_cumpos[j] = before + incl;
    else if (j < k) out_cumpos[j] = before + tot;                              // the padding: cum_pos of the last rank
  }
  if (blockIdx.x == 0) tk_write_meta(S, ws, m, out_meta);                      // (uniform)
}

// the select stage of both entry points: five launches that leave the m candidates in ckey / cpos, in any order
int tk_select_stage(const float *score, const uint8_t *label, int64_t n, int m, const TkLayout &L, int32_t *workspace,
                    int32_t *range_hist, uint32_t *ckey, int32_t *cpos, hipStream_t st) {
  const dim3 grid(L.g), block(TK_T);
  k_tk_init<<<dim3(1), block, 0, st>>>(workspace);
  GGAD_CHECK_LAUNCH("topk init");
  k_tk_hist<0><<<grid, block, 0, st>>>(score, label, n, m, L.per_block, workspace, range_hist);
  GGAD_CHECK_LAUNCH("topk hist 0");
  k_tk_hist<1><<<grid, block, 0, st>>>(score, label, n, m, L.per_block, workspace, range_hist);
  GGAD_CHECK_LAUNCH("topk hist 1");
  k_tk_hist<2><<<grid, block, 0, st>>>(score, label, n, m, L.per_block, workspace, range_hist);
  GGAD_CHECK_LAUNCH("topk hist 2");
  k_tk_select<<<grid, block, 0, st>>>(score, n, m, L.per_block, workspace, range_hist, ckey, cpos);
  GGAD_CHECK_LAUNCH("topk select");
  return GGAD_OK;
}

}  // namespace

extern "C" {

int32_t ggad_topk_max_k(void) { return TK_CAP; }
int32_t ggad_topk_wide_max_k(void) { return TKW_CAP; }

int64_t ggad_topk_workspace_elems(int64_t n, int32_t k) {
  if (n < 0 || n > INT32_MAX || k < 1 || k > TK_CAP) return 0;
  return tk_layout(n).total(k);
}

int64_t ggad_topk_wide_workspace_elems(int64_t n, int32_t k) {
  if (!tkw_args_ok(n, k)) return 0;
  return tkw_layout(n, k).total;
}

int ggad_topk_f32(const float *score, const uint8_t *label, int64_t n, int32_t k, int32_t *out_pos, float *out_score,
                  int32_t *out_cumpos, int64_t *out_meta, int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(out_pos && out_score && out_meta && workspace && n >= 0 && n <= INT32_MAX && k >= 1 && k <= TK_CAP && (n == 0 || score));
  const TkLayout L = tk_layout(n);
  static ggad_lds_optin lds;
  const int ready = ggad_lds_opt_in(lds, TK_SORT_LDS, k_tk_sort);
  if (ready == 0) return GGAD_E_INVALID;
  if (ready != 1) { ggad_set_error(hipErrorInvalidValue, "topk: this device cannot give k_tk_sort its LDS"); return GGAD_E_LAUNCH; }
  hipStream_t st = as_stream(stream);
  const int m = (int)(n < k ? n : k);
  int M = 64;
  while (M < m) M <<= 1;
  uint32_t *ckey = reinterpret_cast<uint32_t *>(workspace + L.o_key());
  int32_t *cpos = workspace + L.o_pos(k);
  const int rc = tk_select_stage(score, label, n, m, L, workspace, workspace + L.o_range(k), ckey, cpos, st);
  if (rc != GGAD_OK) return rc;
  k_tk_sort<<<dim3(1), dim3(TK_T), (size_t)M * 8, st>>>(score, label, n, k, m, M, workspace, ckey, cpos, out_pos, out_score, out_cumpos, out_meta);
  GGAD_CHECK_LAUNCH("topk sort");
  return GGAD_OK;
}

int ggad_topk_wide_f32(const float *score, const uint8_t *label, int64_t n, int32_t k, int32_t *out_pos, float *out_score,
                       int32_t *out_cumpos, int64_t *out_meta, int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(out_pos && out_score && out_meta && workspace && ((uintptr_t)workspace & 7) == 0 && tkw_args_ok(n, k) && (n == 0 || score));
  const TkwLayout L = tkw_layout(n, k);
  hipStream_t st = as_stream(stream);
  const int m = L.m;
  uint32_t *ckey = reinterpret_cast<uint32_t *>(workspace + L.sel.o_key());
  int32_t *cpos = workspace + L.sel.o_pos(k), *cnt = workspace + L.o_cnt;
  unsigned long long *buf[2] = {reinterpret_cast<unsigned long long *>(workspace + L.o_buf0),
                                reinterpret_cast<unsigned long long *>(workspace + L.o_buf1)};
  const int rc = tk_select_stage(score, label, n, m, L.sel, workspace, workspace + L.sel.o_range(k), ckey, cpos, st);
  if (rc != GGAD_OK) return rc;
  const dim3 block(TK_T);
  if (L.runs > 0) {
    k_tkw_runs<<<dim3(L.runs), block, 0, st>>>(ckey, cpos, m, buf[0]);
    GGAD_CHECK_LAUNCH("topk_wide runs");
  }
  for (int p = 0; p < L.passes; ++p) {
    k_tkw_merge<<<dim3((m + TK_T - 1) / TK_T), block, 0, st>>>(buf[p & 1], buf[(p & 1) ^ 1], m, TKW_RUN << p);
    GGAD_CHECK_LAUNCH("topk_wide merge");
  }
  k_tkw_emit<<<dim3((k + TK_T - 1) / TK_T), block, 0, st>>>(score, label, n, k, m, buf[L.passes & 1], out_pos, out_score, out_cumpos, cnt);
  GGAD_CHECK_LAUNCH("topk_wide emit");
  k_tkw_cum<<<dim3(out_cumpos ? (k + TK_T - 1) / TK_T : 1), block, 0, st>>>(workspace, k, m, cnt, out_cumpos, out_meta);
  GGAD_CHECK_LAUNCH("topk_wide cum");
  return GGAD_OK;
}

}  // extern "C"
