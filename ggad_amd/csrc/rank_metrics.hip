// Rank metrics of a binary classifier from float32 scores and uint8 labels: AUROC, average precision and the confusion counts of
// `score >= thres`, with scikit-learn's treatment of tied scores, as EXACT counts -- no full sort, no host synchronisation, no
// floating-point atomics, nothing that waits on another workgroup.  With P positives, Nn negatives and pos[] the sorted positive
// scores, for positive k
//     L_k = negatives with score <  pos[k]        E_k = negatives with score == pos[k]        G_k = positives with score >= pos[k]
//     AUROC = sum_k (2 L_k + E_k) / (2 P Nn)      (the numerator an exact int64: ONE float64 division)
//     AP    = (1 / P) sum_k G_k / (G_k + Nn - L_k)    (float64 terms, summed in a fixed order)
// Only the positives are sorted (one workgroup, bitonic network in LDS); every negative is bucketed against them by binary search.
//
// Four launches on one stream:
//   k_rm_scan    all n elements, RM_G workgroups over contiguous ranges: confusion counts and flags per workgroup (plain stores),
//                the keys of the positives appended to the workgroup's own segment; clears the two histograms of k_rm_bucket
//   k_rm_sort    one workgroup: totals, status, the segments gathered and sorted
//   k_rm_bucket  the sorted keys in LDS; per negative a lower- and an upper-bound search, +1 in two LDS histograms of P + 1 bins,
//                flushed with integer atomics (integers: the result does not depend on the order)
//   k_rm_finish  one workgroup: prefix sums, the two formulas, out8
// Everything a launch reads was written by an earlier launch of the same call, so the workspace needs no preparation and the call
// can be captured and replayed.
#include "common.h"

#include <mutex>

namespace {

constexpr int RM_CAP = 8192;              // positives one call takes: keys (32 KB) + two histograms (2 x 32 KB) in the 160 KB LDS
constexpr int RM_T = 1024;                // threads of every workgroup
constexpr int RM_G = 256;                 // workgroups of k_rm_scan at most (one segment of keys each)
constexpr int RM_GB = 64;                 // workgroups of k_rm_bucket at most
constexpr int RM_HDR = 8;                 // ints per workgroup of k_rm_scan: tp, fp, fn, tn, positives, flags
constexpr int RM_META = 16;               // ints of k_rm_sort's summary: tp, fp, fn, tn, P, status
constexpr int RM_BUCKET_LDS = RM_CAP * 4 + 2 * (RM_CAP + 1) * 4;

struct RmLayout {                         // int32 offsets into the workspace
  int64_t per_block, seg_cap;
  int g;
  int64_t o_hdr() const { return 0; }
  int64_t o_meta() const { return (int64_t)RM_G * RM_HDR; }
  int64_t o_keys() const { return o_meta() + RM_META; }
  int64_t o_hist() const { return o_keys() + RM_CAP; }                    // histU[RM_CAP + 1] then histE[RM_CAP + 1]
  int64_t o_seg() const { return o_hist() + 2 * (RM_CAP + 1); }
  int64_t total() const { return o_seg() + (int64_t)g * seg_cap; }
};

RmLayout rm_layout(int64_t n) {
  RmLayout L;
  int64_t g = (n + RM_T - 1) / RM_T;
  L.g = (int)(g < 1 ? 1 : (g > RM_G ? RM_G : g));
  L.per_block = (n + L.g - 1) / L.g;
  L.seg_cap = L.per_block < RM_CAP ? L.per_block : RM_CAP;
  if (L.seg_cap < 1) L.seg_cap = 1;
  return L;
}

// order-preserving image of a float (not NaN): a < b <=> key(a) < key(b), and -0.0 ties with +0.0
__device__ __forceinline__ uint32_t rm_key(float s) {
  const uint32_t b = s == 0.0f ? 0u : __float_as_uint(s);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

__global__ void __launch_bounds__(RM_T) k_rm_scan(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n,
                                                  float thres, int64_t per_block, int seg_cap, int32_t *__restrict__ hdr,
                                                  uint32_t *__restrict__ seg, int32_t *__restrict__ hist) {
  __shared__ int s_cnt[6];
  for (int i = blockIdx.x * RM_T + threadIdx.x; i < 2 * (RM_CAP + 1); i += gridDim.x * RM_T) hist[i] = 0;
  if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * per_block;
  const int64_t hi = lo + per_block < n ? lo + per_block : n;
  uint32_t *my = seg + (int64_t)blockIdx.x * seg_cap;
  const int lane = lane_id();
  int tp = 0, fp = 0, fn = 0, tn = 0, flags = 0;
  for (int64_t base = lo + (threadIdx.x - lane); base < hi; base += RM_T) {        // (whole waves: the ballot below needs every lane)
    const int64_t i = base + lane;
    bool is_pos = false;
    uint32_t key = 0;
    if (i < hi) {
      const float s = score[i];
      const int y = label[i];
      if (s != s) flags |= 1;
      if (y > 1) flags |= 2;
      const bool pred = s >= thres;
      is_pos = y == 1;
      tp += pred && is_pos;  fp += pred && !is_pos;  fn += !pred && is_pos;  tn += !pred && !is_pos;
      key = rm_key(s);
    }
    const unsigned long long m = __ballot(is_pos);
    if (m) {                                                                       // one LDS atomic per wave that holds positives
      const int leader = __ffsll(m) - 1;
      int slot0 = 0;
      if (lane == leader) slot0 = atomicAdd(&s_cnt[4], __popcll(m));
      slot0 = __shfl(slot0, leader, GGAD_WAVE);
      const int slot = slot0 + __popcll(m & ((1ull << lane) - 1ull));
      if (is_pos && slot < seg_cap) my[slot] = key;
    }
  }
  tp = wave_sum_i(tp);  fp = wave_sum_i(fp);  fn = wave_sum_i(fn);  tn = wave_sum_i(tn);
  if (lane == 0) {
    atomicAdd(&s_cnt[0], tp);  atomicAdd(&s_cnt[1], fp);  atomicAdd(&s_cnt[2], fn);  atomicAdd(&s_cnt[3], tn);
  }
  if (flags) atomicOr(&s_cnt[5], flags);
  __syncthreads();
  if (threadIdx.x < 6) hdr[blockIdx.x * RM_HDR + threadIdx.x] = s_cnt[threadIdx.x];
}

__global__ void __launch_bounds__(RM_T) k_rm_sort(const int32_t *__restrict__ hdr, int g, int seg_cap, const uint32_t *__restrict__ seg,
                                                  int32_t *__restrict__ meta, uint32_t *__restrict__ keys_out) {
  __shared__ uint32_t keys[RM_CAP];
  __shared__ int32_t off[RM_G + 1];
  __shared__ int64_t tot[6];
  const int t = threadIdx.x;
  if (t == 0) {                                                   // <= 256 workgroups: a serial pass over their headers
    int64_t a[4] = {0, 0, 0, 0}, p = 0;
    int flags = 0;
    for (int b = 0; b < g; ++b) {
      const int32_t *h = hdr + b * RM_HDR;
      for (int j = 0; j < 4; ++j) a[j] += h[j];
      off[b] = (int32_t)(p < RM_CAP + 1 ? p : RM_CAP + 1);
      p += h[4];
      flags |= h[5];
    }
    off[g] = (int32_t)(p < RM_CAP + 1 ? p : RM_CAP + 1);
    const int64_t nn = a[1] + a[3];
    int status = 0;
    if (flags & 2) status = 4;
    else if (flags & 1) status = 3;
    else if (p > RM_CAP) status = 2;
    else if (p == 0 || nn == 0) status = 1;
    for (int j = 0; j < 4; ++j) { meta[j] = (int32_t)a[j]; tot[j] = a[j]; }
    meta[4] = (int32_t)p;
    meta[5] = status;
    tot[4] = p;  tot[5] = status;
  }
  __syncthreads();
  if (tot[5] != 0) return;
  const int P = (int)tot[4];
  int M = 64;
  while (M < P) M <<= 1;
  for (int i = t; i < M; i += RM_T) {
    uint32_t k = 0xFFFFFFFFu;                                     // padding: above every key (NaN scores never get here)
    if (i < P) {
      int lo = 0, hi = g;                                         // the segment that holds the i-th positive: last b with off[b] <= i
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
      k = seg[(int64_t)lo * seg_cap + (i - off[lo])];
    }
    keys[i] = k;
  }
  __syncthreads();
  for (int size = 2; size <= M; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < (M >> 1); i += RM_T) {
        const int a = 2 * i - (i & (stride - 1)), b = a + stride;
        const bool up = (a & size) == 0;
        const uint32_t x = keys[a], y = keys[b];
        if ((x > y) == up) { keys[a] = y; keys[b] = x; }
      }
      __syncthreads();
    }
  }
  for (int i = t; i < P; i += RM_T) keys_out[i] = keys[i];
}

__global__ void __launch_bounds__(RM_T) k_rm_bucket(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n,
                                                    const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys_in,
                                                    int32_t *__restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rm_lds[];
  if (meta[5] != 0) return;
  const int P = meta[4];
  uint32_t *keys = rm_lds;
  int *hu = reinterpret_cast<int *>(rm_lds + RM_CAP), *he = hu + (RM_CAP + 1);
  for (int i = threadIdx.x; i < P; i += RM_T) keys[i] = keys_in[i];
  for (int i = threadIdx.x; i <= P; i += RM_T) { hu[i] = 0; he[i] = 0; }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * RM_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * RM_T) {
    if (label[i] != 0) continue;
    const uint32_t key = rm_key(score[i]);
    int lo = 0, hi = P;                                           // lb = positives below this score = first index of its run, if any
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
    const int lb = lo;
    hi = P;                                                       // ub = positives at or below it
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] <= key) lo = mid + 1; else hi = mid; }
    atomicAdd(&hu[lo], 1);
    if (lo > lb) atomicAdd(&he[lb], 1);
  }
  __syncthreads();
  int32_t *gu = hist, *ge = hist + (RM_CAP + 1);
  for (int i = threadIdx.x; i <= P; i += RM_T) {
    if (hu[i]) atomicAdd(&gu[i], hu[i]);
    if (he[i]) atomicAdd(&ge[i], he[i]);
  }
}

__global__ void __launch_bounds__(RM_T) k_rm_finish(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys_in,
                                                    const int32_t *__restrict__ hist, double *__restrict__ out8) {
  constexpr int CH = RM_CAP / RM_T;                               // consecutive positives of one thread
  __shared__ uint32_t keys[RM_CAP];
  __shared__ int32_t scan[2][RM_T];                              // (every prefix is a count of negatives: n <= INT32_MAX)
  __shared__ double red[RM_T];
  __shared__ int64_t redi[RM_T];
  const int t = threadIdx.x;
  const int status = meta[5];
  const int64_t tp = meta[0], fp = meta[1], fn = meta[2], tn = meta[3];
  const int P = status == 0 ? meta[4] : 0;
  const int64_t Nn = fp + tn;
  const int32_t *hu = hist, *he = hist + (RM_CAP + 1);
  for (int i = t; i < P; i += RM_T) keys[i] = keys_in[i];
  int64_t loc[CH];
  int64_t run = 0;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int k = t * CH + j;
    if (k < P) run += hu[k];
    loc[j] = run;
  }
  scan[0][t] = (int32_t)run;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < RM_T; d <<= 1) {                            // inclusive scan of the threads' totals
    scan[cur ^ 1][t] = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const int64_t before = t > 0 ? scan[cur][t - 1] : 0;
  double ap = 0.0;
  int64_t num = 0;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int k = t * CH + j;
    if (k >= P) continue;
    const int64_t L = before + loc[j];
    const uint32_t key = keys[k];
    int lo = 0, hi = k;                                           // first index of the run of equal keys that holds k
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
    const int64_t G = P - lo;
    num += 2 * L + he[lo];
    ap += (double)G / (double)(G + Nn - L);
  }
  red[t] = ap;
  redi[t] = num;
  __syncthreads();
  for (int d = RM_T / 2; d > 0; d >>= 1) {
    if (t < d) { red[t] += red[t + d]; redi[t] += redi[t + d]; }
    __syncthreads();
  }
  if (t == 0) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const int64_t n_pos = meta[4];
    double auroc = nan, avp = nan;
    if (status == 0) {
      auroc = (double)redi[0] / (double)(2 * (int64_t)P * Nn);
      avp = red[0] / (double)P;
    } else if (status == 1) {
      avp = n_pos == 0 ? 0.0 : 1.0;                               // no positives: 0.0; positives only: every precision is 1
    }
    out8[0] = auroc;  out8[1] = avp;
    out8[2] = (double)tp;  out8[3] = (double)fp;  out8[4] = (double)fn;  out8[5] = (double)tn;
    out8[6] = (double)n_pos;  out8[7] = (double)status;
  }
}

}  // namespace

extern "C" {

int32_t ggad_rank_metrics_max_pos(void) { return RM_CAP; }

int64_t ggad_rank_metrics_workspace_elems(int64_t n) {
  if (n < 0 || n > INT32_MAX) return 0;
  return rm_layout(n).total();
}

int ggad_rank_metrics_f32(const float *score, const uint8_t *label, int64_t n, float thres, double *out8, int32_t *workspace,
                          ggad_stream_t stream) {
  GGAD_REQUIRE(out8 && workspace && n >= 0 && n <= INT32_MAX && (n == 0 || (score && label)));
  const RmLayout L = rm_layout(n);
  {  // more than 64 KB of dynamic LDS is a per-DEVICE attribute of the kernel: set (and checked) once per device of the process
    static std::mutex mu;
    static int state[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return GGAD_E_INVALID;
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev] == 0) {
      const bool ok = hipFuncSetAttribute((const void *)k_rm_bucket, hipFuncAttributeMaxDynamicSharedMemorySize, RM_BUCKET_LDS) == hipSuccess;
      (void)hipGetLastError();
      state[dev] = ok ? 1 : -1;
    }
    if (state[dev] != 1) { ggad_set_error(hipErrorInvalidValue, "rank_metrics: this device cannot give k_rm_bucket its LDS"); return GGAD_E_LAUNCH; }
  }
  hipStream_t st = as_stream(stream);
  int32_t *hdr = workspace + L.o_hdr(), *meta = workspace + L.o_meta(), *hist = workspace + L.o_hist();
  uint32_t *keys = reinterpret_cast<uint32_t *>(workspace + L.o_keys()), *seg = reinterpret_cast<uint32_t *>(workspace + L.o_seg());
  k_rm_scan<<<dim3(L.g), dim3(RM_T), 0, st>>>(score, label, n, thres, L.per_block, (int)L.seg_cap, hdr, seg, hist);
  GGAD_CHECK_LAUNCH("rank_metrics scan");
  k_rm_sort<<<dim3(1), dim3(RM_T), 0, st>>>(hdr, L.g, (int)L.seg_cap, seg, meta, keys);
  GGAD_CHECK_LAUNCH("rank_metrics sort");
  int64_t gb = (n + 16 * RM_T - 1) / (16 * RM_T);
  gb = gb < 1 ? 1 : (gb > RM_GB ? RM_GB : gb);
  k_rm_bucket<<<dim3((unsigned)gb), dim3(RM_T), RM_BUCKET_LDS, st>>>(score, label, n, meta, keys, hist);
  GGAD_CHECK_LAUNCH("rank_metrics bucket");
  k_rm_finish<<<dim3(1), dim3(RM_T), 0, st>>>(meta, keys, hist, out8);
  GGAD_CHECK_LAUNCH("rank_metrics finish");
  return GGAD_OK;
}

}  // extern "C"
