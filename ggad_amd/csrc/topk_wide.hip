// ggad_topk_f32 (topk.hip) above the 16,384 ranks one workgroup sorts in LDS, up to TKW_CAP = 4,194,304: the same ranking (score
// descending, equal scores by ascending position, -0.0 tied with +0.0), the same outputs, padding, meta words and status codes, and
// for k <= 16,384 the same bits in every output.  With m = min(k, n), R = ceil(m / 2,048) and B = ceil(m / 1,024) the launches on one
// stream are
//   k_tk_init, k_tk_hist<0..2>, k_tk_select   the select stage of topk_common.h, unchanged: the m (key, position) candidates, in any
//                 order, and the flags, the positives among all n and the histograms that give `tied_left_out`
//   k_tkw_runs    R workgroups.  Run r packs candidates [2,048 r, ...) into 64-bit words (~key << 32) | position, whose ASCENDING
//                 unsigned order is "key descending, position ascending" = the ranking, pads with ~0 (above every word: a key is
//                 never 0), and sorts them with the bitonic network in 16 KB of static LDS
//   k_tkw_merge   ceil(log2(R)) passes, ping-pong between two word buffers, one thread per word: a word's place in the merged pair of
//                 runs is its index in its own run plus its rank in the partner run.  Positions are distinct, so the words are, and
//                 one lower bound serves both sides.  An unpaired last run is copied through, so the ranking always ends in the
//                 buffer the pass count names
//   k_tkw_emit    one thread per output slot: out_pos, out_score = score[pos], the padding beyond m; with out_cumpos the 0/1 label of
//                 the rank is parked in out_cumpos and the label-1 ranks of each block of 1,024 are stored with plain stores
//   k_tkw_cum     workgroup b sums the block counts before it (at most 4,096 ints, a fixed order), scans its own 1,024 parked labels
//                 and writes out_cumpos, padding included; workgroup 0 writes out_meta
// 5 + 1 + ceil(log2(R)) + 2 launches: 19 at the cap.  No host synchronisation, integer atomics only (those of the select stage),
// nothing waits on another workgroup, and every word a launch reads was written by the host or by an earlier launch of the same call:
// a workspace of arbitrary bits needs no preparation, and the call is captured and replayed as one linear chain.
//
// Workspace, in int32 elements, with W = max(m, 1):  the select stage's tk_layout(n).total(k)  +  2 buffers x 2 W (the 64-bit words)
// +  ceil(W / 1,024) block counts.  At n >= k = 2^22 that is 32 MB of candidates + 64 MB of words + 16 KB of counts.
//
// Runs of 2,048 and the merge by rank are rank_wide.hip's choices, for its measured reasons (head of that file).
#include "topk_common.h"

namespace {

constexpr int TKW_CAP = 1 << 22;          // k at most: one call ranks every node of DGraph-Fin (3,700,550); 2,048 runs, 11 merge passes
constexpr int TKW_RUN = 2048;             // words one workgroup sorts: 16 KB of LDS, one exchange per thread and step

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
  __syncthreads();
  for (int size = 2; size <= M; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < (M >> 1); i += TK_T) {
        const int a = 2 * i - (i & (stride - 1)), b = a + stride;
        const bool up = (a & size) == 0;
        const unsigned long long x = w[a], y = w[b];
        if ((x > y) == up) { w[a] = y; w[b] = x; }
      }
      __syncthreads();
    }
  }
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

// the sum of one int per thread over the workgroup, for every thread (16 wave totals through LDS, added in wave order)
__device__ __forceinline__ int tkw_block_sum(int32_t *s16, int v) {
  v = wave_sum_i(v);
  if (lane_id() == 0) s16[threadIdx.x / GGAD_WAVE] = v;
  __syncthreads();
  int tot = 0;
#pragma unroll
  for (int w = 0; w < TK_T / GGAD_WAVE; ++w) tot += s16[w];
  __syncthreads();
  return tot;
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
    const int tot = tkw_block_sum(s16, y);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
  }
}

__global__ void __launch_bounds__(TK_T) k_tkw_cum(const int32_t *__restrict__ ws, int k, int m, const int32_t *__restrict__ cnt,
                                                  int32_t *__restrict__ out_cumpos, int64_t *__restrict__ out_meta) {
  __shared__ TkScan S;
  __shared__ int32_t s16[TK_T / GGAD_WAVE];
  const int t = threadIdx.x;
  if (out_cumpos) {
    const int nb = (m + TK_T - 1) / TK_T;                                      // blocks of ranks that hold any (<= 4,096)
    const int upto = (int)blockIdx.x < nb ? (int)blockIdx.x : nb;
    int s = 0;
    for (int i = t; i < upto; i += TK_T) s += cnt[i];
    const int before = tkw_block_sum(s16, s);
    const int j = blockIdx.x * TK_T + t;
    const int y = j < m ? out_cumpos[j] : 0;
    int tot = 0;
    const int incl = tk_block_scan(S, y, &tot);
    if (j < m) out_cumpos[j] = before + incl;
    else if (j < k) out_cumpos[j] = before + tot;                              // the padding: cum_pos of the last rank
  }
  if (blockIdx.x == 0) {                                                       // (uniform)
    int left_out = 0;
    if (m > 0) {
      int d0, a0, d1, a1, d2, a2;
      tk_pick(S, ws + TK_O_H0, TK_B01, m, d0, a0);
      tk_pick(S, ws + TK_O_H1, TK_B01, m - a0, d1, a1);
      tk_pick(S, ws + TK_O_H2, TK_B2, m - a0 - a1, d2, a2);
      left_out = ws[TK_O_H2 + d2] - (m - a0 - a1 - a2);
    }
    if (t == 0) {
      const int flags = m > 0 ? ws[TK_O_CTR + 0] : 0;
      out_meta[0] = m;
      out_meta[1] = (flags & 2) ? 4 : (flags & 1) ? 3 : 0;
      out_meta[2] = m > 0 ? ws[TK_O_CTR + 1] : 0;
      out_meta[3] = left_out;
    }
  }
}

}  // namespace

extern "C" {

int32_t ggad_topk_wide_max_k(void) { return TKW_CAP; }

int64_t ggad_topk_wide_workspace_elems(int64_t n, int32_t k) {
  if (!tkw_args_ok(n, k)) return 0;
  return tkw_layout(n, k).total;
}

int ggad_topk_wide_f32(const float *score, const uint8_t *label, int64_t n, int32_t k, int32_t *out_pos, float *out_score,
                       int32_t *out_cumpos, int64_t *out_meta, int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(out_pos && out_score && out_meta && workspace && ((uintptr_t)workspace & 7) == 0 && tkw_args_ok(n, k) && (n == 0 || score));
  const TkwLayout L = tkw_layout(n, k);
  hipStream_t st = as_stream(stream);
  const int m = L.m;
  uint32_t *ckey = reinterpret_cast<uint32_t *>(workspace + L.sel.o_key());
  int32_t *cpos = workspace + L.sel.o_pos(k), *range_hist = workspace + L.sel.o_range(k), *cnt = workspace + L.o_cnt;
  unsigned long long *buf[2] = {reinterpret_cast<unsigned long long *>(workspace + L.o_buf0),
                                reinterpret_cast<unsigned long long *>(workspace + L.o_buf1)};
  const dim3 grid(L.sel.g), block(TK_T);
  k_tk_init<<<dim3(1), block, 0, st>>>(workspace);
  GGAD_CHECK_LAUNCH("topk_wide init");
  k_tk_hist<0><<<grid, block, 0, st>>>(score, label, n, m, L.sel.per_block, workspace, range_hist);
  GGAD_CHECK_LAUNCH("topk_wide hist 0");
  k_tk_hist<1><<<grid, block, 0, st>>>(score, label, n, m, L.sel.per_block, workspace, range_hist);
  GGAD_CHECK_LAUNCH("topk_wide hist 1");
  k_tk_hist<2><<<grid, block, 0, st>>>(score, label, n, m, L.sel.per_block, workspace, range_hist);
  GGAD_CHECK_LAUNCH("topk_wide hist 2");
  k_tk_select<<<grid, block, 0, st>>>(score, n, m, L.sel.per_block, workspace, range_hist, ckey, cpos);
  GGAD_CHECK_LAUNCH("topk_wide select");
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
