// Exact, deterministic top-k of float32 scores: the k highest scores of n, ranked by score descending and, among equal scores, by
// ascending position in the input (-0.0 ties with +0.0, +-inf are ordinary values, a NaN anywhere is reported in the status word);
// beside them the running count of label-1 elements along the ranking (precision / recall @ j), the positives among all n, and how
// many elements tie with the last rank but were left out.  No host synchronisation, integer atomics only, nothing that waits on
// another workgroup; equal inputs give equal bits in every output.
//
// The 32-bit order-preserving key of a score is cut into three digits (11 + 11 + 10 bits, most significant first).  With m = min(k, n):
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
//                 ties in position order (chunks of 1,024 consecutive elements, ballots and a 16-entry table per chunk)
//   k_tk_sort     one workgroup: the m (key, position) pairs as 64-bit words in LDS, bitonic network (a total order, so the append
//                 order above cannot show; up to three strides per pass over LDS), scores and labels gathered, labels prefix-summed,
//                 out_meta
// Every word a launch reads was written by an earlier launch of the same call: the workspace needs no preparation and the call can
// be captured and replayed.  Everything up to k_tk_select lives in topk_common.h, which topk_wide.hip (k above 16,384) shares.
#include "topk_common.h"

#include <mutex>

namespace {

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
  __shared__ TkScan S;
  const int t = threadIdx.x;
  int left_out = 0, total = 0;
  if (m > 0) {
    int d0, a0, d1, a1, d2, a2;
    tk_pick(S, ws + TK_O_H0, TK_B01, m, d0, a0);
    tk_pick(S, ws + TK_O_H1, TK_B01, m - a0, d1, a1);
    tk_pick(S, ws + TK_O_H2, TK_B2, m - a0 - a1, d2, a2);
    left_out = ws[TK_O_H2 + d2] - (m - a0 - a1 - a2);
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
    int run = tk_block_scan(S, local, &total) - local;
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
  if (t == 0) {
    const int flags = m > 0 ? ws[TK_O_CTR + 0] : 0;
    out_meta[0] = m;
    out_meta[1] = (flags & 2) ? 4 : (flags & 1) ? 3 : 0;
    out_meta[2] = m > 0 ? ws[TK_O_CTR + 1] : 0;
    out_meta[3] = left_out;
  }
}

}  // namespace

extern "C" {

int32_t ggad_topk_max_k(void) { return TK_CAP; }

int64_t ggad_topk_workspace_elems(int64_t n, int32_t k) {
  if (n < 0 || n > INT32_MAX || k < 1 || k > TK_CAP) return 0;
  return tk_layout(n).total(k);
}

int ggad_topk_f32(const float *score, const uint8_t *label, int64_t n, int32_t k, int32_t *out_pos, float *out_score,
                  int32_t *out_cumpos, int64_t *out_meta, int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(out_pos && out_score && out_meta && workspace && n >= 0 && n <= INT32_MAX && k >= 1 && k <= TK_CAP && (n == 0 || score));
  const TkLayout L = tk_layout(n);
  {  // more than 64 KB of dynamic LDS is a per-DEVICE attribute of the kernel: set (and checked) once per device of the process
    static std::mutex mu;
    static int state[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return GGAD_E_INVALID;
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev] == 0) {
      const bool ok = hipFuncSetAttribute((const void *)k_tk_sort, hipFuncAttributeMaxDynamicSharedMemorySize, TK_SORT_LDS) == hipSuccess;
      (void)hipGetLastError();
      state[dev] = ok ? 1 : -1;
    }
    if (state[dev] != 1) { ggad_set_error(hipErrorInvalidValue, "topk: this device cannot give k_tk_sort its LDS"); return GGAD_E_LAUNCH; }
  }
  hipStream_t st = as_stream(stream);
  const int m = (int)(n < k ? n : k);
  int M = 64;
  while (M < m) M <<= 1;
  uint32_t *ckey = reinterpret_cast<uint32_t *>(workspace + L.o_key());
  int32_t *cpos = workspace + L.o_pos(k), *range_hist = workspace + L.o_range(k);
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
  k_tk_sort<<<dim3(1), block, (size_t)M * 8, st>>>(score, label, n, k, m, M, workspace, ckey, cpos, out_pos, out_score, out_cumpos, out_meta);
  GGAD_CHECK_LAUNCH("topk sort");
  return GGAD_OK;
}

}  // extern "C"
