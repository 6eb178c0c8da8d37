// Rank metrics of a binary classifier from float32 scores and uint8 labels: AUROC, average precision and the confusion counts of
// `score >= thres`, with scikit-learn's treatment of tied scores, as EXACT counts -- no full sort, no host synchronisation, no
// floating-point atomics, nothing that waits on another workgroup.  With P positives, Nn negatives and pos[] the sorted positive
// scores, for positive k
//     L_k = negatives with score <  pos[k]        E_k = negatives with score == pos[k]        G_k = positives with score >= pos[k]
//     AUROC = sum_k (2 L_k + E_k) / (2 P Nn)      (the numerator an exact int64: ONE float64 division)
//     AP    = (1 / P) sum_k G_k / (G_k + Nn - L_k)    (float64 terms, summed in a fixed order)
// Only the positives are sorted; every negative is bucketed against them by binary search.  No launch reads a word that an earlier
// launch of the same call did not write, so the workspace needs no preparation and a call can be captured and replayed.  Two chains
// share the pieces of this file and of rank_common.h (the key, the bounds, the bitonic network, the workgroup scan):
//
// ggad_rank_metrics_f32, at most RM_CAP = 8,192 positives: four launches
//   k_rm_scan    all n elements, <= 256 workgroups over contiguous ranges: confusion counts and flags per workgroup (plain stores),
//                the keys of the positives appended to the workgroup's own segment; clears the two histograms of k_rm_bucket
//   k_rm_sort    one workgroup: totals, status, the segments gathered and sorted with the bitonic network in LDS
//   k_rm_bucket  the sorted keys in LDS; per negative a lower- and an upper-bound search, +1 in two LDS histograms of P + 1 bins,
//                flushed with integer atomics (integers: the result does not depend on the order)
//   k_rm_finish  one workgroup: prefix sums, the two formulas (8 consecutive positives per thread, then a halving tree), out8
//
// ggad_rank_wide_f32, at most RW_MAX = 1,048,576 positives.  `pos_cap` is the caller's bound on the positives; grids and workspace
// follow from (n, pos_cap) alone.  With pc = min(pos_cap, max(n, 1)), TILE = 8,192, Tc = ceil(pc / TILE) and Sc = ceil(pc / 2,048):
//   k_rw_scan    k_rm_scan's range scan (the one rm_scan_range); the segment capacity is min(per_block, pc); it clears nothing
//   k_rw_sort    Sc workgroups.  Each sums the <= 256 headers (totals, status, segment offsets: one thread per header, a scan and a
//                tree in LDS); workgroup 0 stores the summary.  Workgroup r gathers keys [2,048 r, min(P, 2,048 (r + 1))) from the
//                segments, sorts them with the bitonic network and clears the histogram bins of its range; runs beyond P return
//   k_rw_merge   ceil(log2(Sc)) passes, ping-pong between two key buffers, one thread per key: the key's place in the merged pair of
//                runs is its index in its own run plus its rank in the partner run (lower bound from the left run, upper bound from
//                the right one: equal keys keep distinct places).  An unpaired last run -- and a run that already covers P -- is
//                copied through, so the sorted keys always end in the buffer the pass count names
//   k_rw_bucket  a (Tc x rows) grid.  Column t holds tile t of the sorted keys and two histograms in LDS and walks the n elements; a
//                negative belongs to the ONE tile with first key of t <= key < first key of t + 1 (open ends), where its upper bound
//                ub is t TILE + the local one.  +1 in histU[ub], and, when the key at ub - 1 equals it, +1 in histE[ub - 1]: ties
//                are counted at the END of a run, so a run that crosses a tile edge needs no look into another tile.  Flushed with
//                integer atomics
//   k_rw_terms   workgroup b owns positives [b TILE, (b + 1) TILE): sum of histU before them, a scan inside, per positive k the start s
//                and end e of its run (neighbours first, binary search only inside a run); L_k = prefix of histU through k,
//                E_k = histE[e], G_k = P - s.  Partial int64 numerator and float64 AP sum per workgroup, in k_rm_finish's order
//   k_rw_final   the partials in a halving tree over the tiles, out8 (the one rm_write_out8)
//
// ggad_rank_operating_f32: the run-merge chain's front (rw_front: scan .. bucket) and, in place of the last two launches,
//   k_ro_terms   k_rw_terms' sums from the one rw_terms_tile, and per run of equal positives the candidate (tp = G_k, fp = Nn - L_k:
//                the confusion counts of `score >= pos[k]`): the curve stores, the best candidate per thread, a tree over the workgroup
//   k_ro_final   k_rw_final's tree into out16[0..7] and a tree over the tiles' candidates into out16[8..15]
// At 8,192 positives or fewer that is one tile and no merge pass, so there is no narrow chain for it.
//
// ggad_rank_delong_f32 / ggad_rank_delong_pair_f32: the same front (twice for the pair, into two halves of the workspace) and
//   k_rd_terms   k_rw_terms' sums in its order, and the tile's exact 128-bit share of sum a^2 (positives) and sum b^2 (negatives, from
//                the two histograms alone); the pair's variant also stores L_k per sorted rank
//   k_rd_cross   pair only: every element looks its key up in both models' sorted keys and adds a^A a^B or b^A b^B in 128 bits
//   k_rd_final / k_rd_pair_final   k_rw_final's tree with the 128-bit sums beside it; the variance numerators, each converted ONCE
// (the formulas: above k_rd_terms, further down)
//
// ggad_rank_bootstrap_f32: ggad_rank_wide_f32's launches as they are (out16[0..7] = its out8) and ONE more,
//   k_rb_boot    one workgroup per replicate of a stratified bootstrap: Philox draws binned by a search in the prefix of histU, three
//                integer histograms in LDS, AP* and the AUROC numerator of the replicate (the scheme: above rb_philox, further down)
//
// ggad_rank_bootstrap_pair_f32: ggad_rank_wide_f32's launches twice, into two halves of the workspace (out24[0..7], [8..15]), and
//   k_rp_cells   one pass over the n elements: per negative a uint16 cell (ub | tie << 15) under A and under B, per positive its two
//                uint16 ranks, stored at the element's number among its class in position order (k_rw_scan's headers give the offsets)
//   k_rp_boot    one workgroup per replicate of a PAIRED bootstrap: the replicate draws element numbers, and each model's three
//                histograms come from one 2-byte gather per draw; model A completely, then B from the same regenerated draws
// Why runs of 2,048 and a merge by rank: head of rank_common.h.  Why the narrow chain stays although the wide one is twice as fast at
// DGraph-Fin's size: inside a captured training epoch (run.py --select) a validation list of 3,935 nodes costs the wide chain six
// launches against four, and the epoch is 21 us longer (profiles/rank_one_chain_time_line.json).
#include "rank_common.h"

namespace {

constexpr int RW_TILE = 8192;             // keys of one tile: keys (32 KB) + two histograms (2 x 32 KB) in the 160 KB LDS
constexpr int RM_CAP = 8192;              // positives the narrow chain takes: keys (32 KB) + two histograms (2 x 32 KB) in LDS
constexpr int RM_GB = 64;                 // workgroups of k_rm_bucket at most
constexpr int RW_STILE = RK_RUN;          // keys one workgroup sorts
constexpr int RW_MAX = 1 << 20;           // positives one call takes: 128 tiles, 512 sorted runs, 9 merge passes
constexpr int RW_TMAX = RW_MAX / RW_TILE;
constexpr int RW_T = RK_T;                // threads of every workgroup
constexpr int RW_G = 256;                 // workgroups of k_rw_scan at most (one segment of keys each)
constexpr int RW_ROWS = 128;              // rows of k_rw_bucket's grid at most
constexpr int RW_HDR = 8;                 // ints per workgroup of k_rw_scan: tp, fp, fn, tn, positives, flags
constexpr int RW_META = 16;               // ints of the summary: tp, fp, fn, tn, P, status, tiles
constexpr int RW_BUCKET_LDS = RW_TILE * 4 + 2 * (RW_TILE + 1) * 4;
constexpr int RO_PART = 8;                // ints per tile of k_ro_terms: tp, fp, key, candidates, the float64 value, two spare
constexpr int RO_CRITERIA = 5;            // f1, f1_macro, gmean, precision, fpr

static_assert(RM_CAP == RW_TILE, "k_rm_bucket and k_rw_bucket take the same RW_BUCKET_LDS bytes");
static_assert((RW_G * RW_HDR + RW_META + 4 * RW_TMAX) % 4 == 0 && RW_TILE % 4 == 0, "o_part, o_keys and o_hist stay 16-byte aligned");

struct RwLayout {                         // int32 offsets into the workspace (o_part: 8-byte aligned; o_hist: 16-byte aligned)
  int64_t per_block, seg_cap, pc;
  int g, tc, st, passes, rows;
  int64_t o_hdr() const { return 0; }
  int64_t o_meta() const { return (int64_t)RW_G * RW_HDR; }
  int64_t o_part() const { return o_meta() + RW_META; }                   // double ap[RW_TMAX] then int64 num[RW_TMAX]
  int64_t o_keys() const { return o_part() + 4 * RW_TMAX; }               // two buffers of tc tiles
  int64_t o_hist() const { return o_keys() + 2 * (int64_t)tc * RW_TILE; } // histU[pc + 1] then histE[pc + 1]
  int64_t o_seg() const { return o_hist() + 2 * (pc + 1); }
  int64_t total() const { return o_seg() + (int64_t)g * seg_cap; }
  int64_t o_op() const { return (total() + 3) & ~(int64_t)3; }            // ggad_rank_operating_f32 only: RO_PART ints per tile
  int64_t total_op() const { return o_op() + (int64_t)RO_PART * RW_TMAX; }
};

struct RmLayout {                         // the narrow chain's int32 offsets into the workspace
  int64_t per_block, seg_cap;
  int g;
  int64_t o_hdr() const { return 0; }
  int64_t o_meta() const { return (int64_t)RW_G * RW_HDR; }
  int64_t o_keys() const { return o_meta() + RW_META; }
  int64_t o_hist() const { return o_keys() + RM_CAP; }                    // histU[RM_CAP + 1] then histE[RM_CAP + 1]
  int64_t o_seg() const { return o_hist() + 2 * (RM_CAP + 1); }
  int64_t total() const { return o_seg() + (int64_t)g * seg_cap; }
};

RmLayout rm_layout(int64_t n) {
  RmLayout L;
  int64_t g = (n + RW_T - 1) / RW_T;
  L.g = (int)(g < 1 ? 1 : (g > RW_G ? RW_G : g));
  L.per_block = (n + L.g - 1) / L.g;
  L.seg_cap = L.per_block < RM_CAP ? L.per_block : RM_CAP;
  if (L.seg_cap < 1) L.seg_cap = 1;
  return L;
}

RwLayout rw_layout(int64_t n, int64_t pos_cap) {
  RwLayout L;
  int64_t g = (n + RW_T - 1) / RW_T;
  L.g = (int)(g < 1 ? 1 : (g > RW_G ? RW_G : g));
  L.per_block = (n + L.g - 1) / L.g;
  L.pc = pos_cap < (n > 1 ? n : 1) ? pos_cap : (n > 1 ? n : 1);           // more positives than elements cannot be
  L.seg_cap = L.per_block < L.pc ? L.per_block : L.pc;
  if (L.seg_cap < 1) L.seg_cap = 1;
  L.tc = (int)((L.pc + RW_TILE - 1) / RW_TILE);
  L.st = (int)((L.pc + RW_STILE - 1) / RW_STILE);
  L.passes = 0;
  while ((1 << L.passes) < L.st) ++L.passes;
  int64_t rows = (n + 16 * RW_T - 1) / (16 * RW_T);
  const int64_t most = 256 / L.tc > RW_ROWS ? RW_ROWS : (256 / L.tc < 1 ? 1 : 256 / L.tc);
  L.rows = (int)(rows < 1 ? 1 : (rows > most ? most : rows));
  return L;
}

// The scan of both chains: workgroup b takes elements [b per_block, ...): confusion counts, flags and the number of positives to its
// header by plain stores, the keys of the positives appended to its own segment.
__device__ __forceinline__ void rm_scan_range(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n, float thres,
                                              int64_t per_block, int seg_cap, int32_t *__restrict__ hdr, uint32_t *__restrict__ seg) {
  __shared__ int s_cnt[6];
  if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * per_block;
  const int64_t hi = lo + per_block < n ? lo + per_block : n;
  uint32_t *my = seg + (int64_t)blockIdx.x * seg_cap;
  const int lane = lane_id();
  int tp = 0, fp = 0, fn = 0, tn = 0, flags = 0;
  for (int64_t base = lo + (threadIdx.x - lane); base < hi; base += RW_T) {        // (whole waves: the ballot below needs every lane)
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
      key = rk_key(s);
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
  if (threadIdx.x < 6) hdr[blockIdx.x * RW_HDR + threadIdx.x] = s_cnt[threadIdx.x];
}

__global__ void __launch_bounds__(RW_T) k_rw_scan(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n,
                                                  float thres, int64_t per_block, int seg_cap, int32_t *__restrict__ hdr,
                                                  uint32_t *__restrict__ seg) {
  rm_scan_range(score, label, n, thres, per_block, seg_cap, hdr, seg);
}

// ---- the narrow chain (head of the file): four launches for at most RM_CAP positives
__global__ void __launch_bounds__(RW_T) k_rm_scan(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n,
                                                  float thres, int64_t per_block, int seg_cap, int32_t *__restrict__ hdr,
                                                  uint32_t *__restrict__ seg, int32_t *__restrict__ hist) {
  for (int i = blockIdx.x * RW_T + threadIdx.x; i < 2 * (RM_CAP + 1); i += gridDim.x * RW_T) hist[i] = 0;     // k_rm_bucket's histograms
  rm_scan_range(score, label, n, thres, per_block, seg_cap, hdr, seg);
}

__global__ void __launch_bounds__(RW_T) k_rm_sort(const int32_t *__restrict__ hdr, int g, int seg_cap, const uint32_t *__restrict__ seg,
                                                  int32_t *__restrict__ meta, uint32_t *__restrict__ keys_out) {
  __shared__ uint32_t keys[RM_CAP];
  __shared__ int32_t off[RW_G + 1];
  __shared__ int64_t tot[6];
  const int t = threadIdx.x;
  if (t == 0) {                                                   // <= 256 workgroups: a serial pass over their headers
    int64_t a[4] = {0, 0, 0, 0}, p = 0;
    int flags = 0;
    for (int b = 0; b < g; ++b) {
      const int32_t *h = hdr + b * RW_HDR;
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
  for (int i = t; i < M; i += RW_T) {
    uint32_t k = 0xFFFFFFFFu;                                     // padding: above every key (NaN scores never get here)
    if (i < P) {
      int lo = 0, hi = g;                                         // the segment that holds the i-th positive: last b with off[b] <= i
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
      k = seg[(int64_t)lo * seg_cap + (i - off[lo])];
    }
    keys[i] = k;
  }
  rk_bitonic(keys, M);
  for (int i = t; i < P; i += RW_T) keys_out[i] = keys[i];
}

__global__ void __launch_bounds__(RW_T) k_rm_bucket(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n,
                                                    const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys_in,
                                                    int32_t *__restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rm_lds[];
  if (meta[5] != 0) return;
  const int P = meta[4];
  uint32_t *keys = rm_lds;
  int *hu = reinterpret_cast<int *>(rm_lds + RM_CAP), *he = hu + (RM_CAP + 1);
  for (int i = threadIdx.x; i < P; i += RW_T) keys[i] = keys_in[i];
  for (int i = threadIdx.x; i <= P; i += RW_T) { hu[i] = 0; he[i] = 0; }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * RW_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * RW_T) {
    if (label[i] != 0) continue;
    const uint32_t key = rk_key(score[i]);
    const int lb = rk_lower(keys, 0, P, key);                     // positives below this score = first index of its run, if any
    const int ub = rk_upper(keys, lb, P, key);                    // positives at or below it
    atomicAdd(&hu[ub], 1);
    if (ub > lb) atomicAdd(&he[lb], 1);
  }
  __syncthreads();
  int32_t *gu = hist, *ge = hist + (RM_CAP + 1);
  for (int i = threadIdx.x; i <= P; i += RW_T) {
    if (hu[i]) atomicAdd(&gu[i], hu[i]);
    if (he[i]) atomicAdd(&ge[i], he[i]);
  }
}

// out8 of both chains from the summary words, the exact numerator and the AP sum: ONE float64 division each
__device__ __forceinline__ void rm_write_out8(const int32_t *__restrict__ meta, int64_t num, double ap_sum, double *__restrict__ out8) {
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const int64_t tp = meta[0], fp = meta[1], fn = meta[2], tn = meta[3], n_pos = meta[4];
  const int status = meta[5];
  const int64_t Nn = fp + tn;
  double auroc = nan, avp = nan;
  if (status == 0) {
    auroc = (double)num / (double)(2 * n_pos * Nn);
    avp = ap_sum / (double)n_pos;
  } else if (status == 1) {
    avp = n_pos == 0 ? 0.0 : 1.0;                                 // no positives: 0.0; positives only: every precision is 1
  }
  out8[0] = auroc;  out8[1] = avp;
  out8[2] = (double)tp;  out8[3] = (double)fp;  out8[4] = (double)fn;  out8[5] = (double)tn;
  out8[6] = (double)n_pos;  out8[7] = (double)status;
}

__global__ void __launch_bounds__(RW_T) k_rm_finish(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys_in,
                                                    const int32_t *__restrict__ hist, double *__restrict__ out8) {
  constexpr int CH = RM_CAP / RW_T;                               // consecutive positives of one thread
  __shared__ uint32_t keys[RM_CAP];
  __shared__ RkScan S;                                            // (every prefix is a count of negatives: n <= INT32_MAX)
  __shared__ double red[RW_T];
  __shared__ int64_t redi[RW_T];
  const int t = threadIdx.x;
  const int P = meta[5] == 0 ? meta[4] : 0;
  const int64_t Nn = (int64_t)meta[1] + meta[3];
  const int32_t *hu = hist, *he = hist + (RM_CAP + 1);
  for (int i = t; i < P; i += RW_T) keys[i] = keys_in[i];
  int64_t loc[CH];
  int64_t run = 0;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int k = t * CH + j;
    if (k < P) run += hu[k];
    loc[j] = run;
  }
  const int64_t before = rk_block_scan(S, (int32_t)run, nullptr) - (int32_t)run;    // scan of the threads' totals (its barriers also
  double ap = 0.0;                                                                   // publish keys[])
  int64_t num = 0;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int k = t * CH + j;
    if (k >= P) continue;
    const int64_t L = before + loc[j];
    const int lo = rk_lower(keys, 0, k, keys[k]);                 // first index of the run of equal keys that holds k
    const int64_t G = P - lo;
    num += 2 * L + he[lo];
    ap += (double)G / (double)(G + Nn - L);
  }
  red[t] = ap;
  redi[t] = num;
  __syncthreads();
  for (int d = RW_T / 2; d > 0; d >>= 1) {
    if (t < d) { red[t] += red[t + d]; redi[t] += redi[t + d]; }
    __syncthreads();
  }
  if (t == 0) rm_write_out8(meta, redi[0], red[0], out8);
}

// ---- the run-merge chain

__global__ void __launch_bounds__(RW_T) k_rw_sort(const int32_t *__restrict__ hdr, int g, int seg_cap, int pc,
                                                  const uint32_t *__restrict__ seg, int32_t *__restrict__ meta,
                                                  uint32_t *__restrict__ keys_out, int32_t *__restrict__ hist) {
  __shared__ uint32_t keys[RW_STILE];
  __shared__ int32_t off[RW_G + 1];
  __shared__ int32_t hs[6][RW_G];                                 // the headers, one thread each (a serial pass over 256 of them
  __shared__ RkScan S;                                            // is ~100 us of dependent loads); every sum is <= n <= INT32_MAX
  __shared__ int32_t tot[2];
  const int t = threadIdx.x;
  if (t < RW_G) {
#pragma unroll
    for (int j = 0; j < 6; ++j) hs[j][t] = t < g ? hdr[t * RW_HDR + j] : 0;
  }
  const int upto = rk_block_scan(S, t < g ? hdr[t * RW_HDR + 4] : 0, nullptr);    // inclusive scan of the segments' counts
  if (t < RW_G) off[t + 1] = upto;                                // (segments past g hold nothing: off[b] = P for b >= g)
  if (t == 0) off[0] = 0;
  for (int d = RW_G / 2; d > 0; d >>= 1) {                        // totals (integers: any order) and the flags
    if (t < d) {
#pragma unroll
      for (int j = 0; j < 4; ++j) hs[j][t] += hs[j][t + d];
      hs[5][t] |= hs[5][t + d];
    }
    __syncthreads();
  }
  if (t == 0) {
    const int p = off[RW_G], flags = hs[5][0];
    const int64_t nn = (int64_t)hs[1][0] + hs[3][0];
    int status = 0;
    if (flags & 2) status = 4;
    else if (flags & 1) status = 3;
    else if (p > pc) status = 2;
    else if (p == 0 || nn == 0) status = 1;
    if (blockIdx.x == 0) {
      for (int j = 0; j < 4; ++j) meta[j] = hs[j][0];
      meta[4] = p;
      meta[5] = status;
      meta[6] = (int32_t)(((int64_t)p + RW_TILE - 1) / RW_TILE);
    }
    tot[0] = p;  tot[1] = status;
  }
  __syncthreads();
  if (tot[1] != 0) return;
  const int P = tot[0];
  const int base = blockIdx.x * RW_STILE;
  if (base >= P) return;
  const int len = P - base < RW_STILE ? P - base : RW_STILE;
  int32_t *gu = hist, *ge = hist + (pc + 1);
  for (int i = t; i <= len; i += RW_T) { gu[base + i] = 0; ge[base + i] = 0; }    // bins base .. base + len <= P <= pc (the next run
                                                                                  // clears bin base + len again: the same zero)
  int M = 64;
  while (M < len) M <<= 1;
  for (int i = t; i < M; i += RW_T) {
    uint32_t k = 0xFFFFFFFFu;                                     // padding: above every key (NaN scores never get here)
    if (i < len) {
      const int q = base + i;
      int lo = 0, hi = g;                                         // the segment that holds the q-th positive: last b with off[b] <= q
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= q) lo = mid; else hi = mid; }
      k = seg[(int64_t)lo * seg_cap + (q - off[lo])];
    }
    keys[i] = k;
  }
  rk_bitonic(keys, M);
  for (int i = t; i < len; i += RW_T) keys_out[base + i] = keys[i];
}

// one pass: runs of `width` keys of src[0, P) merged in pairs into dst[0, P)
__global__ void __launch_bounds__(RW_T) k_rw_merge(const int32_t *__restrict__ meta, const uint32_t *__restrict__ src,
                                                   uint32_t *__restrict__ dst, int width) {
  if (meta[5] != 0) return;
  const int P = meta[4];
  const int i = blockIdx.x * RW_T + threadIdx.x;
  if (i >= P) return;
  const uint32_t key = src[i];
  const int base = (i / (2 * width)) * (2 * width);               // (2 * width <= 2^20)
  const int mid = base + width;
  if (mid >= P) { dst[i] = key; return; }                         // an unpaired run: carried through
  const int end = mid + width < P ? mid + width : P;
  const int at = i < mid ? (i - base) + (rk_lower(src, mid, end, key) - mid) : (i - mid) + (rk_upper(src, base, mid, key) - base);
  dst[base + at] = key;
}

__global__ void __launch_bounds__(RW_T) k_rw_bucket(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n,
                                                    const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys_in, int pc,
                                                    int32_t *__restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rw_lds[];
  if (meta[5] != 0) return;
  const int P = meta[4], T = meta[6];
  const int tile = blockIdx.x;
  if (tile >= T) return;
  const int base = tile * RW_TILE;
  const int len = P - base < RW_TILE ? P - base : RW_TILE;
  uint32_t *keys = rw_lds;
  int *hu = reinterpret_cast<int *>(rw_lds + RW_TILE), *he = hu + (RW_TILE + 1);
  for (int i = threadIdx.x; i < len; i += RW_T) keys[i] = keys_in[base + i];
  for (int i = threadIdx.x; i <= len; i += RW_T) { hu[i] = 0; he[i] = 0; }
  const bool open_lo = tile == 0, open_hi = tile == T - 1;
  const uint32_t first = keys_in[base], next = open_hi ? 0u : keys_in[base + RW_TILE];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.y * RW_T + threadIdx.x; i < n; i += (int64_t)gridDim.y * RW_T) {
    if (label[i] != 0) continue;
    const uint32_t key = rk_key(score[i]);
    if (!((open_lo || key >= first) && (open_hi || key < next))) continue;        // another tile's negative
    const int ub = rk_upper(keys, 0, len, key);                   // positives of this tile at or below it (>= 1 unless tile 0)
    atomicAdd(&hu[ub], 1);
    if (ub > 0 && keys[ub - 1] == key) atomicAdd(&he[ub - 1], 1);
  }
  __syncthreads();
  int32_t *gu = hist + base, *ge = hist + (pc + 1) + base;
  for (int i = threadIdx.x; i <= len; i += RW_T) {
    if (hu[i]) atomicAdd(&gu[i], hu[i]);
    if (i < len && he[i]) atomicAdd(&ge[i], he[i]);
  }
}

// ---- the operating point (ggad_rank_operating_f32).  A candidate is the run of equal positives [s, e]: threshold pos[s], tp = G,
// fp = Nn - L, both exact.  tp == 0 marks "none" (a real candidate holds its own positive).
struct RoCand {
  int32_t tp, fp;
  uint32_t key;
  double v;                                                       // criterion 1 only: 0.5 (F1 of class 1 + F1 of class 0)
};

struct RoArgs {
  int crit;
  double param;
  float *curve_thres;                                             // all three or none
  int32_t *curve_tp, *curve_fp;
  int32_t *part;                                                  // RO_PART ints per tile
};

__device__ __forceinline__ float ro_score(uint32_t key) { return __uint_as_float((key >> 31) ? (key & 0x7FFFFFFFu) : ~key); }    // rk_key back

// the candidate of (tp, fp, key) under the criterion: macro-F1 formed as metrics._confusion_scores forms it (each class F1 one
// division of exact integers, a zero denominator counts 0); criteria 3 and 4 drop what misses the constraint
__device__ __forceinline__ RoCand ro_make(int crit, double param, int64_t P, int64_t Nn, int64_t tp, int64_t fp, uint32_t key) {
  RoCand c;
  c.tp = (int32_t)tp;  c.fp = (int32_t)fp;  c.key = key;  c.v = 0.0;
  if (crit == 1) {
    const int64_t fn = P - tp, tn = Nn - fp, d0 = 2 * tn + fn + fp;
    const double f1 = 2.0 * (double)tp / (double)(2 * tp + fp + fn);
    const double f0 = d0 ? 2.0 * (double)tn / (double)d0 : 0.0;
    c.v = 0.5 * (f1 + f0);
  } else if (crit == 3) {
    c.tp = (double)tp >= param * (double)(tp + fp) ? c.tp : 0;
  } else if (crit == 4) {
    c.tp = (double)fp <= param * (double)Nn ? c.tp : 0;
  }
  return c;
}

// does b replace a?  Criteria 0 and 2 in exact int64 (cross-multiplied F1 < 2^54, tp tn < 2^51), 1 in float64, 3 and 4 by recall;
// equal values: the higher threshold.  A total order, so the reduction's shape does not move the result.
// Written without a branch on the candidates (`crit` is uniform over the launch; the rest are selects): the callers keep the winner
// with selects too (ro_pick), so the per-thread loop of k_ro_terms has no divergent control flow around its four running fields.  Keep
// it so: `if (better) best = c;` with early returns in here compiled, for gfx950, to code that left best.fp behind (DESIGN.md section 4;
// tests/test_operating_point_gpu.py::test_tie_rule_by_hand and the case n63 show it).
__device__ __forceinline__ bool ro_better(int crit, int64_t P, int64_t Nn, const RoCand &a, const RoCand &b) {
  int64_t l = b.tp, r = a.tp;                                     // criteria 3 and 4: the greater recall
  if (crit == 0) {                                                // 2tp / (2tp + fp + fn) = 2tp / (tp + fp + P)
    l = (int64_t)b.tp * ((int64_t)a.tp + a.fp + P);  r = (int64_t)a.tp * ((int64_t)b.tp + b.fp + P);
  } else if (crit == 2) {
    l = (int64_t)b.tp * (Nn - b.fp);  r = (int64_t)a.tp * (Nn - a.fp);
  }
  bool gt = l > r, eq = l == r;
  if (crit == 1) { gt = b.v > a.v;  eq = b.v == a.v; }            // (no NaN: both are sums of two quotients in [0, 1])
  const bool wins = gt | (eq & (b.key > a.key));
  return (b.tp != 0) & ((a.tp == 0) | wins);
}

// a, or b where it replaces a: four selects
__device__ __forceinline__ RoCand ro_pick(bool take_b, const RoCand &a, const RoCand &b) {
  RoCand c;
  c.tp = take_b ? b.tp : a.tp;  c.fp = take_b ? b.fp : a.fp;  c.key = take_b ? b.key : a.key;  c.v = take_b ? b.v : a.v;
  return c;
}

struct RoLds {                                                    // the candidate tree of one workgroup
  int32_t tp[RW_T], fp[RW_T];
  uint32_t key[RW_T];
  double v[RW_T];
};

// k_rw_terms (OP = false) and k_ro_terms (OP = true): the same sums in the same order; OP adds the curve stores and the arg-max
template <bool OP>
__device__ __forceinline__ void rw_terms_tile(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys, int pc,
                                              const int32_t *__restrict__ hist, double *__restrict__ part_ap,
                                              int64_t *__restrict__ part_num, const RoArgs &A, RoLds *C) {
  constexpr int CH = RW_TILE / RW_T;                              // consecutive positives of one thread
  __shared__ RkScan S;                                            // (every prefix is a count of negatives: n <= INT32_MAX)
  __shared__ double red[RW_T];
  __shared__ int64_t redi[RW_T];
  if (meta[5] != 0) return;
  const int t = threadIdx.x;
  const int P = meta[4];
  const int base = blockIdx.x * RW_TILE;
  if (base >= P) return;
  const int64_t Nn = (int64_t)meta[1] + meta[3];
  const int32_t *hu = hist, *he = hist + (pc + 1);
  int32_t mine = 0;                                               // negatives binned before this workgroup's positives
  const int4 *hu4 = reinterpret_cast<const int4 *>(hu);          // (histU starts on a 16-byte boundary, base is a multiple of 8,192)
  for (int i = t; i < base / 4; i += RW_T) { const int4 v = hu4[i]; mine += v.x + v.y + v.z + v.w; }
  const int64_t before_all = rk_block_sum(S.wsum, mine);
  int64_t loc[CH];
  int64_t run = 0;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int k = base + t * CH + j;
    if (k < P) run += hu[k];
    loc[j] = run;
  }
  const int64_t before = before_all + (rk_block_scan(S, (int32_t)run, nullptr) - (int32_t)run);    // scan of the threads' totals
  double ap = 0.0;
  int64_t num = 0;
  RoCand best = {0, 0, 0u, 0.0};
  int cands = 0;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int k = base + t * CH + j;
    if (k >= P) continue;
    const int64_t L = before + loc[j];
    const uint32_t key = keys[k];
    int s = k, e = k;                                             // the run of equal keys that holds k: [s, e]
    if (k > 0 && keys[k - 1] == key) s = rk_lower(keys, 0, k - 1, key);
    if (k + 1 < P && keys[k + 1] == key) e = rk_upper(keys, k + 2, P, key) - 1;
    const int64_t G = P - s;
    num += 2 * L + he[e];
    ap += (double)G / (double)(G + Nn - L);
    if constexpr (OP) {
      if (A.curve_thres) {                                        // entry j: the run of the j-th highest positive
        const int j = P - 1 - k;
        A.curve_thres[j] = ro_score(key);  A.curve_tp[j] = (int32_t)G;  A.curve_fp[j] = (int32_t)(Nn - L);
      }
      const bool first = s == k;                                  // one candidate per run, ascending: a later equal value wins
      cands += first;
      const RoCand c = ro_make(A.crit, A.param, P, Nn, G, Nn - L, key);
      best = ro_pick(first & ro_better(A.crit, P, Nn, best, c), best, c);
    }
  }
  red[t] = ap;
  redi[t] = num;
  if constexpr (OP) { C->tp[t] = best.tp;  C->fp[t] = best.fp;  C->key[t] = best.key;  C->v[t] = best.v; }
  __syncthreads();
  for (int d = RW_T / 2; d > 0; d >>= 1) {
    if (t < d) {
      red[t] += red[t + d];  redi[t] += redi[t + d];
      if constexpr (OP) {
        const RoCand a = {C->tp[t], C->fp[t], C->key[t], C->v[t]}, b = {C->tp[t + d], C->fp[t + d], C->key[t + d], C->v[t + d]};
        const RoCand w = ro_pick(ro_better(A.crit, P, Nn, a, b), a, b);
        C->tp[t] = w.tp;  C->fp[t] = w.fp;  C->key[t] = w.key;  C->v[t] = w.v;
      }
    }
    __syncthreads();
  }
  if (t == 0) { part_ap[blockIdx.x] = red[0]; part_num[blockIdx.x] = redi[0]; }
  if constexpr (OP) {
    const int all = rk_block_sum(S.wsum, cands);
    if (t == 0) {
      int32_t *o = A.part + (int64_t)blockIdx.x * RO_PART;
      o[0] = C->tp[0];  o[1] = C->fp[0];  o[2] = (int32_t)C->key[0];  o[3] = all;
      *reinterpret_cast<double *>(o + 4) = C->v[0];
    }
  }
}

__global__ void __launch_bounds__(RW_T) k_rw_terms(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys, int pc,
                                                   const int32_t *__restrict__ hist, double *__restrict__ part_ap,
                                                   int64_t *__restrict__ part_num) {
  rw_terms_tile<false>(meta, keys, pc, hist, part_ap, part_num, RoArgs{}, nullptr);
}

__global__ void __launch_bounds__(RW_T) k_ro_terms(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys, int pc,
                                                   const int32_t *__restrict__ hist, double *__restrict__ part_ap,
                                                   int64_t *__restrict__ part_num, RoArgs A) {
  __shared__ RoLds C;
  rw_terms_tile<true>(meta, keys, pc, hist, part_ap, part_num, A, &C);
}

__global__ void __launch_bounds__(RW_TMAX) k_rw_final(const int32_t *__restrict__ meta, const double *__restrict__ part_ap,
                                                      const int64_t *__restrict__ part_num, double *__restrict__ out8) {
  __shared__ double red[RW_TMAX];
  __shared__ int64_t redi[RW_TMAX];
  const int t = threadIdx.x;
  const int status = meta[5];
  const int T = status == 0 ? meta[6] : 0;
  red[t] = t < T ? part_ap[t] : 0.0;
  redi[t] = t < T ? part_num[t] : 0;
  __syncthreads();
  for (int d = RW_TMAX / 2; d > 0; d >>= 1) {
    if (t < d) { red[t] += red[t + d]; redi[t] += redi[t + d]; }
    __syncthreads();
  }
  if (t == 0) rm_write_out8(meta, redi[0], red[0], out8);
}

// k_rw_final's tree (the same out8 bits into out16[0..7]) and beside it the tree over the tiles' candidates: out16[8..15]
__global__ void __launch_bounds__(RW_TMAX) k_ro_final(const int32_t *__restrict__ meta, const double *__restrict__ part_ap,
                                                      const int64_t *__restrict__ part_num, const int32_t *__restrict__ part, int crit,
                                                      double *__restrict__ out16) {
  __shared__ double red[RW_TMAX];
  __shared__ int64_t redi[RW_TMAX];
  __shared__ int32_t ctp[RW_TMAX], cfp[RW_TMAX], cnt[RW_TMAX];
  __shared__ uint32_t ckey[RW_TMAX];
  __shared__ double cv[RW_TMAX];
  const int t = threadIdx.x;
  const int status = meta[5];
  const int T = status == 0 ? meta[6] : 0;
  const int64_t P = meta[4], Nn = (int64_t)meta[1] + meta[3];
  const int32_t *mine = part + (int64_t)t * RO_PART;
  red[t] = t < T ? part_ap[t] : 0.0;
  redi[t] = t < T ? part_num[t] : 0;
  ctp[t] = t < T ? mine[0] : 0;
  cfp[t] = t < T ? mine[1] : 0;
  ckey[t] = t < T ? (uint32_t)mine[2] : 0u;
  cnt[t] = t < T ? mine[3] : 0;
  cv[t] = t < T ? *reinterpret_cast<const double *>(mine + 4) : 0.0;
  __syncthreads();
  for (int d = RW_TMAX / 2; d > 0; d >>= 1) {
    if (t < d) {
      red[t] += red[t + d];  redi[t] += redi[t + d];  cnt[t] += cnt[t + d];
      const RoCand a = {ctp[t], cfp[t], ckey[t], cv[t]}, b = {ctp[t + d], cfp[t + d], ckey[t + d], cv[t + d]};
      const RoCand w = ro_pick(ro_better(crit, P, Nn, a, b), a, b);
      ctp[t] = w.tp;  cfp[t] = w.fp;  ckey[t] = w.key;  cv[t] = w.v;
    }
    __syncthreads();
  }
  if (t != 0) return;
  rm_write_out8(meta, redi[0], red[0], out16);
  if (status != 0) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int j = 8; j < 15; ++j) out16[j] = nan;
    out16[15] = (double)status;
    return;
  }
  const int64_t tp = ctp[0], fp = cfp[0];
  out16[14] = (double)cnt[0];
  if (tp == 0) {                                                  // no candidate meets the constraint: alert on nothing
    out16[8] = __longlong_as_double(0x7FF0000000000000ll);
    out16[9] = 0.0;  out16[10] = 0.0;  out16[11] = (double)P;  out16[12] = (double)Nn;
    out16[13] = 0.0;  out16[15] = 5.0;
    return;
  }
  const int64_t fn = P - tp, tn = Nn - fp;
  double v;
  if (crit == 0) v = 2.0 * (double)tp / (double)(2 * tp + fp + fn);
  else if (crit == 1) v = cv[0];
  else if (crit == 2) v = sqrt((double)(tp * tn) / (double)(P * Nn));
  else v = (double)tp / (double)P;
  out16[8] = (double)ro_score(ckey[0]);
  out16[9] = (double)tp;  out16[10] = (double)fp;  out16[11] = (double)fn;  out16[12] = (double)tn;
  out16[13] = v;  out16[15] = 0.0;
}

bool rw_args_ok(int64_t n, int64_t pos_cap) { return n >= 0 && n <= INT32_MAX && pos_cap >= 1 && pos_cap <= RW_MAX; }

// The front of the run-merge chain, which ggad_rank_wide_f32 and ggad_rank_operating_f32 share: scan, sorted runs, merge passes,
// the tile bucket.  Leaves the sorted keys, the two histograms and the summary; the caller launches its terms and its final.
struct RwFront {
  RwLayout L;
  hipStream_t st;
  int32_t *meta, *hist;
  double *part_ap;
  int64_t *part_num;
  const uint32_t *keys;
};

int rw_front(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, int32_t *workspace,
             ggad_stream_t stream, RwFront &F) {
  const RwLayout L = rw_layout(n, pos_cap);
  static ggad_lds_optin lds;
  const int ready = ggad_lds_opt_in(lds, RW_BUCKET_LDS, k_rw_bucket);
  if (ready == 0) return GGAD_E_INVALID;
  if (ready != 1) { ggad_set_error(hipErrorInvalidValue, "rank_wide: this device cannot give k_rw_bucket its LDS"); return GGAD_E_LAUNCH; }
  hipStream_t st = as_stream(stream);
  const int pc = (int)L.pc;
  int32_t *hdr = workspace + L.o_hdr(), *meta = workspace + L.o_meta(), *hist = workspace + L.o_hist();
  uint32_t *buf[2] = {reinterpret_cast<uint32_t *>(workspace + L.o_keys()),
                      reinterpret_cast<uint32_t *>(workspace + L.o_keys() + (int64_t)L.tc * RW_TILE)};
  uint32_t *seg = reinterpret_cast<uint32_t *>(workspace + L.o_seg());
  k_rw_scan<<<dim3(L.g), dim3(RW_T), 0, st>>>(score, label, n, thres, L.per_block, (int)L.seg_cap, hdr, seg);
  GGAD_CHECK_LAUNCH("rank_wide scan");
  k_rw_sort<<<dim3(L.st), dim3(RW_T), 0, st>>>(hdr, L.g, (int)L.seg_cap, pc, seg, meta, buf[0], hist);
  GGAD_CHECK_LAUNCH("rank_wide sort");
  for (int p = 0; p < L.passes; ++p) {
    k_rw_merge<<<dim3((unsigned)((L.pc + RW_T - 1) / RW_T)), dim3(RW_T), 0, st>>>(meta, buf[p & 1], buf[(p & 1) ^ 1], RW_STILE << p);
    GGAD_CHECK_LAUNCH("rank_wide merge");
  }
  const uint32_t *keys = buf[L.passes & 1];
  k_rw_bucket<<<dim3(L.tc, L.rows), dim3(RW_T), RW_BUCKET_LDS, st>>>(score, label, n, meta, keys, pc, hist);
  GGAD_CHECK_LAUNCH("rank_wide bucket");
  F.L = L;  F.st = st;  F.meta = meta;  F.hist = hist;  F.keys = keys;
  F.part_ap = reinterpret_cast<double *>(workspace + L.o_part());
  F.part_num = reinterpret_cast<int64_t *>(F.part_ap + RW_TMAX);
  return GGAD_OK;
}

// ---- DeLong's variance of the AUROC, and the covariance of two AUROCs on the same labels (ggad_rank_delong_f32, _pair_f32).
// With m = P, n = Nn, a_k = 2 L_k + E_k per positive and b_j = 2 #{pos > y_j} + #{pos == y_j} per negative (the placements, doubled):
//     S1 = sum a = sum b (the AUROC numerator)    S2 = sum a^2    T2 = sum b^2    N10 = m S2 - S1^2    N01 = n T2 - S1^2
//     var = N10 / (4 n^2 m^2 (m - 1)) + N01 / (4 m^2 n^2 (n - 1))
// and for two models C10 = sum_i a_i^A a_i^B, C01 = sum_j b_j^A b_j^B by ELEMENT; the variance of the difference has numerators of
// its own, ND10 = m (S2A + S2B - 2 C10) - (S1A - S1B)^2 and ND01 alike, so nothing cancels in floating point.  Every sum is an exact
// integer below 2^106 (a, b <= 2^32, m <= 2^20) in 128 bits; each numerator is converted to float64 ONCE (rd_to_double).  Integer
// sums: the shape of a reduction does not move a bit.
typedef unsigned __int128 rd_u128;
typedef __int128 rd_i128;

constexpr int RD_SQ = 4;                  // uint64 per tile of k_rd_terms: S2 lo, hi, T2 lo, hi
constexpr int RD_XG = 256;                // workgroups of k_rd_cross at most; threads of k_rd_pair_final
constexpr int RD_XP = 4;                  // uint64 per workgroup of k_rd_cross: C10 lo, hi, C01 lo, hi

static_assert(RD_XG >= RW_TMAX, "k_rd_pair_final reduces the tiles and the cross partials with the same threads");

struct RdLayout {                         // behind the run-merge chain's words; the pair call holds two halves, then the cross partials
  RwLayout L;
  int64_t o_sq() const { return (L.total() + 3) & ~(int64_t)3; }                  // RD_SQ uint64 per tile
  int64_t total() const { return o_sq() + 2 * (int64_t)RD_SQ * RW_TMAX; }
  int64_t o_lt() const { return total(); }                                        // pair only: Lt[pc]
  int64_t half() const { return (o_lt() + L.pc + 3) & ~(int64_t)3; }
  int64_t o_cross() const { return 2 * half(); }
  int64_t total_pair() const { return o_cross() + 2 * (int64_t)RD_XP * RD_XG; }
};

// x as a float64, rounded once: the top 64 bits with a sticky bit below them (11 bits more than the significand holds)
__device__ __forceinline__ double rd_to_double(rd_u128 x) {
  const uint64_t hi = (uint64_t)(x >> 64);
  if (hi == 0) return (double)(uint64_t)x;
  const int sh = __clzll((long long)hi);
  const rd_u128 y = x << sh;
  const uint64_t top = (uint64_t)(y >> 64) | ((uint64_t)y != 0 ? 1ull : 0ull);
  return ldexp((double)top, 64 - sh);
}
__device__ __forceinline__ double rd_to_double_signed(rd_i128 x) { return x < 0 ? -rd_to_double((rd_u128)(-x)) : rd_to_double((rd_u128)x); }

// k_rw_terms' sums in k_rw_terms' order (the same out8 bits), and beside them, exact in 128 bits, the tile's share of S2 and T2.
// T2 needs no pass over the negatives: the hu[ub] negatives of bin ub have b = 2 (P - ub), except the he[ub - 1] of them that tie
// with the run [s, e = ub - 1] of equal positives (he is non-zero only at a run's end), which have b = 2 (P - ub) + (e - s + 1).
// Who owns a bin: bin ub >= 1 goes with positive k = ub - 1, so bin base + len goes to THIS tile, bin base to the tile before it, and
// bin P to the last tile; bin 0 (b = 2 P) goes to tile 0.  PAIR also stores Lt[k] = L_k for k_rd_cross.
template <bool PAIR>
__device__ __forceinline__ void rd_terms_tile(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys, int pc,
                                              const int32_t *__restrict__ hist, double *__restrict__ part_ap,
                                              int64_t *__restrict__ part_num, uint64_t *__restrict__ part_sq, int32_t *__restrict__ lt) {
  constexpr int CH = RW_TILE / RW_T;
  __shared__ RkScan S;
  __shared__ double red[RW_T];
  __shared__ int64_t redi[RW_T];
  __shared__ rd_u128 rs2[RW_T], rt2[RW_T];
  if (meta[5] != 0) return;
  const int t = threadIdx.x;
  const int P = meta[4];
  const int base = blockIdx.x * RW_TILE;
  if (base >= P) return;
  const int64_t Nn = (int64_t)meta[1] + meta[3];
  const int32_t *hu = hist, *he = hist + (pc + 1);
  int32_t mine = 0;
  const int4 *hu4 = reinterpret_cast<const int4 *>(hu);
  for (int i = t; i < base / 4; i += RW_T) { const int4 v = hu4[i]; mine += v.x + v.y + v.z + v.w; }
  const int64_t before_all = rk_block_sum(S.wsum, mine);
  int64_t loc[CH];
  int64_t run = 0;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int k = base + t * CH + j;
    if (k < P) run += hu[k];
    loc[j] = run;
  }
  const int64_t before = before_all + (rk_block_scan(S, (int32_t)run, nullptr) - (int32_t)run);
  double ap = 0.0;
  int64_t num = 0;
  rd_u128 s2 = 0, t2 = 0;
  if (base == 0 && t == 0) t2 = (rd_u128)(uint64_t)hu[0] * (uint64_t)(4 * (int64_t)P * P);
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int k = base + t * CH + j;
    if (k >= P) continue;
    const int64_t L = before + loc[j];
    const uint32_t key = keys[k];
    int s = k, e = k;
    if (k > 0 && keys[k - 1] == key) s = rk_lower(keys, 0, k - 1, key);
    if (k + 1 < P && keys[k + 1] == key) e = rk_upper(keys, k + 2, P, key) - 1;
    const int64_t G = P - s;
    const int64_t a = 2 * L + he[e];
    num += a;
    ap += (double)G / (double)(G + Nn - L);
    s2 += (rd_u128)(uint64_t)a * (uint64_t)a;
    const int64_t in_bin = hu[k + 1], tied = he[k];               // bin k + 1 <= P <= pc
    const uint64_t b0 = 2 * (uint64_t)(P - k - 1), b1 = b0 + (uint64_t)(k - s + 1);
    t2 += (rd_u128)(uint64_t)(in_bin - tied) * (b0 * b0) + (rd_u128)(uint64_t)tied * (b1 * b1);
    if constexpr (PAIR) lt[k] = (int32_t)L;
  }
  red[t] = ap;
  redi[t] = num;
  rs2[t] = s2;
  rt2[t] = t2;
  __syncthreads();
  for (int d = RW_T / 2; d > 0; d >>= 1) {
    if (t < d) { red[t] += red[t + d];  redi[t] += redi[t + d];  rs2[t] += rs2[t + d];  rt2[t] += rt2[t + d]; }
    __syncthreads();
  }
  if (t == 0) {
    part_ap[blockIdx.x] = red[0];
    part_num[blockIdx.x] = redi[0];
    uint64_t *o = part_sq + (int64_t)blockIdx.x * RD_SQ;
    o[0] = (uint64_t)rs2[0];  o[1] = (uint64_t)(rs2[0] >> 64);  o[2] = (uint64_t)rt2[0];  o[3] = (uint64_t)(rt2[0] >> 64);
  }
}

__global__ void __launch_bounds__(RW_T) k_rd_terms(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys, int pc,
                                                   const int32_t *__restrict__ hist, double *__restrict__ part_ap,
                                                   int64_t *__restrict__ part_num, uint64_t *__restrict__ part_sq) {
  rd_terms_tile<false>(meta, keys, pc, hist, part_ap, part_num, part_sq, nullptr);
}

__global__ void __launch_bounds__(RW_T) k_rd_terms_lt(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys, int pc,
                                                      const int32_t *__restrict__ hist, double *__restrict__ part_ap,
                                                      int64_t *__restrict__ part_num, uint64_t *__restrict__ part_sq,
                                                      int32_t *__restrict__ lt) {
  rd_terms_tile<true>(meta, keys, pc, hist, part_ap, part_num, part_sq, lt);
}

// One model's words for k_rd_cross and the finals
struct RdModel {
  const int32_t *meta, *hist;
  const uint32_t *keys;
  const int32_t *lt;
  const double *part_ap;
  const int64_t *part_num;
  const uint64_t *part_sq;
};

// the doubled placement of one element under one model: a for a positive (only the upper bound: its own key is among the keys), b for
// a negative (the second search only on a tie)
__device__ __forceinline__ uint64_t rd_placement(const RdModel &M, int P, int pc, uint32_t key, bool is_pos) {
  const int ub = rk_upper(M.keys, 0, P, key);
  if (is_pos) return ub > 0 ? 2 * (uint64_t)M.lt[ub - 1] + (uint64_t)M.hist[(pc + 1) + ub - 1] : 0;
  uint64_t b = 2 * (uint64_t)(P - ub);
  if (ub > 0 && M.keys[ub - 1] == key) b += (uint64_t)(ub - rk_lower(M.keys, 0, ub - 1, key));
  return b;
}

// C10 and C01 over the n elements: both models' sorted keys (at most 4 MB each, L2-resident) searched per element, as k_rw_merge
// searches them.  Per thread, a tree over the workgroup, then k_rd_pair_final's tree over the workgroups.
__global__ void __launch_bounds__(RW_T) k_rd_cross(const float *__restrict__ score_a, const float *__restrict__ score_b,
                                                   const uint8_t *__restrict__ label, int64_t n, int pc, RdModel A, RdModel B,
                                                   uint64_t *__restrict__ part_x) {
  __shared__ rd_u128 r10[RW_T], r01[RW_T];
  if (A.meta[5] != 0 || B.meta[5] != 0) return;
  const int t = threadIdx.x;
  const int P = A.meta[4];                                        // (the same labels: B's is the same)
  rd_u128 c10 = 0, c01 = 0;
  for (int64_t i = (int64_t)blockIdx.x * RW_T + t; i < n; i += (int64_t)gridDim.x * RW_T) {
    const bool is_pos = label[i] != 0;
    const uint64_t pa = rd_placement(A, P, pc, rk_key(score_a[i]), is_pos), pb = rd_placement(B, P, pc, rk_key(score_b[i]), is_pos);
    const rd_u128 prod = (rd_u128)pa * pb;
    if (is_pos) c10 += prod; else c01 += prod;
  }
  r10[t] = c10;
  r01[t] = c01;
  __syncthreads();
  for (int d = RW_T / 2; d > 0; d >>= 1) {
    if (t < d) { r10[t] += r10[t + d];  r01[t] += r01[t + d]; }
    __syncthreads();
  }
  if (t == 0) {
    uint64_t *o = part_x + (int64_t)blockIdx.x * RD_XP;
    o[0] = (uint64_t)r10[0];  o[1] = (uint64_t)(r10[0] >> 64);  o[2] = (uint64_t)r01[0];  o[3] = (uint64_t)(r01[0] >> 64);
  }
}

struct RdLds {                                                    // the trees of the two finals (RD_XG >= RW_TMAX slots)
  double red[RD_XG];
  int64_t redi[RD_XG];
  rd_u128 x[RD_XG], y[RD_XG];
};

struct RdSums {
  int64_t s1;
  double ap;
  rd_u128 s2, t2;
};

// k_rw_final's halving tree over the tiles (the same bits of the AP sum), with S2 and T2 beside it; the result for every thread
__device__ __forceinline__ RdSums rd_tile_tree(RdLds &T, const RdModel &M) {
  const int t = threadIdx.x;
  const int Tn = M.meta[5] == 0 ? M.meta[6] : 0;
  __syncthreads();                                                // (an earlier tree's result has been read)
  if (t < RW_TMAX) {
    const bool in = t < Tn;
    const uint64_t *q = M.part_sq + (int64_t)t * RD_SQ;
    T.red[t] = in ? M.part_ap[t] : 0.0;
    T.redi[t] = in ? M.part_num[t] : 0;
    T.x[t] = in ? ((rd_u128)q[1] << 64) | q[0] : (rd_u128)0;
    T.y[t] = in ? ((rd_u128)q[3] << 64) | q[2] : (rd_u128)0;
  }
  __syncthreads();
  for (int d = RW_TMAX / 2; d > 0; d >>= 1) {
    if (t < d) { T.red[t] += T.red[t + d];  T.redi[t] += T.redi[t + d];  T.x[t] += T.x[t + d];  T.y[t] += T.y[t + d]; }
    __syncthreads();
  }
  RdSums R;
  R.s1 = T.redi[0];  R.ap = T.red[0];  R.s2 = T.x[0];  R.t2 = T.y[0];
  return R;
}

__device__ __forceinline__ void rd_store_limbs(int64_t *__restrict__ sums, int at, rd_u128 v) {
  sums[2 * at] = (int64_t)(uint64_t)v;
  sums[2 * at + 1] = (int64_t)(uint64_t)(v >> 64);
}

// 4 n^2 m^2 (m - 1) and 4 m^2 n^2 (n - 1) in float64
__device__ __forceinline__ double rd_den(double m, double n, double side) { return 4.0 * n * n * m * m * (side - 1.0); }

__global__ void __launch_bounds__(RW_TMAX) k_rd_final(RdModel M, double *__restrict__ out16, int64_t *__restrict__ sums) {
  __shared__ RdLds T;
  const RdSums R = rd_tile_tree(T, M);
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  rm_write_out8(M.meta, R.s1, R.ap, out16);
  const int status = M.meta[5];
  if (status != 0) {
    for (int j = 8; j < 15; ++j) out16[j] = nan;
    for (int j = 0; j < 12; ++j) sums[j] = 0;
    out16[15] = (double)status;
    return;
  }
  const int64_t m = M.meta[4], n = (int64_t)M.meta[1] + M.meta[3];
  const rd_u128 sq = (rd_u128)(uint64_t)R.s1 * (uint64_t)R.s1;
  const rd_u128 n10 = (rd_u128)(uint64_t)m * R.s2 - sq, n01 = (rd_u128)(uint64_t)n * R.t2 - sq;      // >= 0 (Cauchy-Schwarz)
  rd_store_limbs(sums, 0, (rd_u128)(uint64_t)R.s1);  rd_store_limbs(sums, 1, R.s2);  rd_store_limbs(sums, 2, R.t2);
  rd_store_limbs(sums, 3, n10);  rd_store_limbs(sums, 4, n01);
  sums[10] = 0;  sums[11] = 0;
  out16[12] = 0.0;  out16[13] = 0.0;  out16[14] = 0.0;
  if (m < 2 || n < 2) {                                           // no unbiased variance of one placement
    for (int j = 8; j < 12; ++j) out16[j] = nan;
    out16[15] = 6.0;
    return;
  }
  const double v10 = rd_to_double(n10) / rd_den((double)m, (double)n, (double)m);
  const double v01 = rd_to_double(n01) / rd_den((double)m, (double)n, (double)n);
  const double var = v10 + v01;
  out16[8] = var;  out16[9] = v10;  out16[10] = v01;  out16[11] = sqrt(var);
  out16[15] = 0.0;
}

__global__ void __launch_bounds__(RD_XG) k_rd_pair_final(RdModel A, RdModel B, const uint64_t *__restrict__ part_x, int xg,
                                                         double *__restrict__ out24, int64_t *__restrict__ sums) {
  __shared__ RdLds T;
  const int t = threadIdx.x;
  const RdSums Ra = rd_tile_tree(T, A);
  const RdSums Rb = rd_tile_tree(T, B);
  const int sa = A.meta[5], sb = B.meta[5];
  const bool both = sa == 0 && sb == 0;                           // else k_rd_cross wrote nothing
  __syncthreads();
  {
    const bool in = both && t < xg;
    const uint64_t *q = part_x + (int64_t)t * RD_XP;
    T.x[t] = in ? ((rd_u128)q[1] << 64) | q[0] : (rd_u128)0;
    T.y[t] = in ? ((rd_u128)q[3] << 64) | q[2] : (rd_u128)0;
  }
  __syncthreads();
  for (int d = RD_XG / 2; d > 0; d >>= 1) {
    if (t < d) { T.x[t] += T.x[t + d];  T.y[t] += T.y[t + d]; }
    __syncthreads();
  }
  if (t != 0) return;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  rm_write_out8(A.meta, Ra.s1, Ra.ap, out24);
  rm_write_out8(B.meta, Rb.s1, Rb.ap, out24 + 8);
  if (!both) {
    for (int j = 16; j < 23; ++j) out24[j] = nan;
    for (int j = 0; j < 24; ++j) sums[j] = 0;
    out24[23] = (double)(sa != 0 ? sa : sb);
    return;
  }
  const rd_u128 c10 = T.x[0], c01 = T.y[0];
  const int64_t m = A.meta[4], n = (int64_t)A.meta[1] + A.meta[3];
  const rd_u128 um = (rd_u128)(uint64_t)m, un = (rd_u128)(uint64_t)n;
  const rd_i128 d = (rd_i128)Ra.s1 - (rd_i128)Rb.s1;
  const rd_u128 dd = (rd_u128)(d * d);
  const rd_u128 nd10 = um * (Ra.s2 + Rb.s2 - 2 * c10) - dd, nd01 = un * (Ra.t2 + Rb.t2 - 2 * c01) - dd;   // >= 0 (Cauchy-Schwarz)
  rd_store_limbs(sums, 0, (rd_u128)(uint64_t)Ra.s1);  rd_store_limbs(sums, 1, (rd_u128)(uint64_t)Rb.s1);
  rd_store_limbs(sums, 2, Ra.s2);  rd_store_limbs(sums, 3, Rb.s2);  rd_store_limbs(sums, 4, c10);
  rd_store_limbs(sums, 5, Ra.t2);  rd_store_limbs(sums, 6, Rb.t2);  rd_store_limbs(sums, 7, c01);
  rd_store_limbs(sums, 8, nd10);  rd_store_limbs(sums, 9, nd01);
  for (int j = 20; j < 24; ++j) sums[j] = 0;
  out24[22] = 0.0;
  if (m < 2 || n < 2) {
    for (int j = 16; j < 22; ++j) out24[j] = nan;
    out24[23] = 6.0;
    return;
  }
  const double den10 = rd_den((double)m, (double)n, (double)m), den01 = rd_den((double)m, (double)n, (double)n);
  const rd_u128 qa = (rd_u128)(uint64_t)Ra.s1 * (uint64_t)Ra.s1, qb = (rd_u128)(uint64_t)Rb.s1 * (uint64_t)Rb.s1;
  const rd_i128 ab = (rd_i128)Ra.s1 * (rd_i128)Rb.s1;
  out24[16] = rd_to_double(um * Ra.s2 - qa) / den10 + rd_to_double(un * Ra.t2 - qa) / den01;
  out24[17] = rd_to_double(um * Rb.s2 - qb) / den10 + rd_to_double(un * Rb.t2 - qb) / den01;
  out24[18] = rd_to_double_signed((rd_i128)(um * c10) - ab) / den10 + rd_to_double_signed((rd_i128)(un * c01) - ab) / den01;
  const double vd = rd_to_double(nd10) / den10 + rd_to_double(nd01) / den01;
  const double diff = (double)(Ra.s1 - Rb.s1) / (double)(2 * m * n);
  out24[19] = vd;
  out24[20] = diff;
  const bool same = nd10 == 0 && nd01 == 0;                       // the two rankings induce the same placements
  out24[21] = same ? nan : diff / sqrt(vd);
  out24[23] = same ? 7.0 : 0.0;
}

// the launches behind rw_front of one model: its terms kernel; M names what the cross kernel and the finals read
int rd_model(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, int32_t *workspace,
             ggad_stream_t stream, const RdLayout &D, bool pair, RdModel &M, hipStream_t &st) {
  RwFront F;
  const int rc = rw_front(score, label, n, pos_cap, thres, workspace, stream, F);
  if (rc != GGAD_OK) return rc;
  uint64_t *part_sq = reinterpret_cast<uint64_t *>(workspace + D.o_sq());
  int32_t *lt = workspace + D.o_lt();
  if (pair) k_rd_terms_lt<<<dim3(F.L.tc), dim3(RW_T), 0, F.st>>>(F.meta, F.keys, (int)F.L.pc, F.hist, F.part_ap, F.part_num, part_sq, lt);
  else k_rd_terms<<<dim3(F.L.tc), dim3(RW_T), 0, F.st>>>(F.meta, F.keys, (int)F.L.pc, F.hist, F.part_ap, F.part_num, part_sq);
  GGAD_CHECK_LAUNCH("rank_delong terms");
  M.meta = F.meta;  M.hist = F.hist;  M.keys = F.keys;  M.lt = lt;  M.part_ap = F.part_ap;  M.part_num = F.part_num;  M.part_sq = part_sq;
  st = F.st;
  return GGAD_OK;
}

// ---- Stratified bootstrap of AP and AUROC from the chain's bins (ggad_rank_bootstrap_f32).  A replicate redraws P positives among
// the P sorted ranks (w[k] = how often rank k was drawn) and Nn negatives among the Nn negatives; a negative is known by its bin only:
// bin b of histU (the negatives with exactly b positives at or below them), and inside the bin whether it is one of the histE[b - 1]
// that tie the positive run ending at b - 1 (the first histE[b - 1] places of the bin, by convention).  So a replicate is three
// integer histograms, w[P], cU[P + 1], cE[P + 1], and never touches the n elements:
//     L*_k  = prefix of cU through k       TP*_k = sum of w from the start s of k's run of equal keys
//     AP*   = (1 / P) sum_k w_k TP*_k / (TP*_k + Nn - L*_k)        num* = sum_k w_k (2 L*_k + cE[e]), e the run's end (exact int64)
// Draws are Philox4x32-10 (Random123; the constants of rocrand_philox4x32_10.h), key (seed lo, seed hi), counter (j lo, j hi,
// replicate, stream): call j gives draws 2j and 2j + 1 as x = c0 | c1 << 32 and c2 | c3 << 32, a draw over m outcomes is
// mulhi64(x, m).  Stream 0 the positives, 1 the negatives.  Which thread makes which draw does not matter: LDS integer atomics only.
constexpr int RB_MAXP = 9216;             // four int32 arrays of P + 1 entries (147,472 bytes) beside the tree and scan scratch
constexpr int RB_MAXREPS = 4096;
constexpr int RB_TOO_FEW = 8, RB_TOO_MANY = 9;      // statuses behind the chain's 1 .. 4 (5: operating point, 6 and 7: DeLong)
constexpr int RB_LDS_MAX = 4 * (RB_MAXP + 1) * 4;

static_assert(RB_LDS_MAX + RW_T * 8 + (int)sizeof(RkScan) <= 160 * 1024, "k_rb_boot's arrays, its tree and its scan share one CU's LDS");

__device__ __forceinline__ void rb_philox(uint32_t k0, uint32_t k1, uint64_t j, uint32_t rep, uint32_t stream, uint64_t &x0, uint64_t &x1) {
  uint32_t c0 = (uint32_t)j, c1 = (uint32_t)(j >> 32), c2 = rep, c3 = stream;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0;  c1 = l1;  c2 = n2;  c3 = l0;
    k0 += 0x9E3779B9u;  k1 += 0xBB67AE85u;
  }
  x0 = (uint64_t)c0 | ((uint64_t)c1 << 32);
  x1 = (uint64_t)c2 | ((uint64_t)c3 << 32);
}

// a[0, len) in LDS replaced by its inclusive (EXCL: exclusive) prefix sums: `chunk` consecutive entries per thread, a scan of the
// threads' totals between two passes.  Whole workgroup; the caller's stores to a[] need a barrier before it, the sums none after it.
template <bool EXCL>
__device__ __forceinline__ void rb_prefix(RkScan &S, int32_t *a, int len, int chunk) {
  const int lo = threadIdx.x * chunk, hi = lo + chunk < len ? lo + chunk : len;
  int32_t tot = 0;
  for (int i = lo; i < hi; ++i) tot += a[i];
  int32_t run = rk_block_scan(S, tot, nullptr) - tot;
  for (int i = lo; i < hi; ++i) {
    const int32_t v = a[i];
    a[i] = EXCL ? run : run + v;
    run += v;
  }
  __syncthreads();
}

union RbRed { double d[RW_T]; int64_t i[RW_T]; };                // the tree of rb_terms: the AP sum, then the numerator

// The two formulas from a replicate's histograms in LDS, for k_rb_boot and k_rp_boot alike: a0 = w (a0[P] = 0), cu, ce; a1 is
// scratch of P + 1 ints.  Consecutive ranks per thread, then the halving tree: ap_sum (before the division by P) and num, both valid
// in thread 0.  Whole workgroup; the caller's stores to the histograms need a barrier before it, red none after it.
__device__ __forceinline__ void rb_terms(RkScan &S, RbRed &red, const int32_t *a0, int32_t *a1, const int32_t *cu, const int32_t *ce,
                                         const uint32_t *__restrict__ keys, int P, int64_t Nn, int chunk, double &ap_sum, int64_t &num_sum) {
  const int t = threadIdx.x;
  for (int i = t; i <= P; i += RW_T) a1[i] = a0[i];
  __syncthreads();
  rb_prefix<true>(S, a1, P + 1, chunk);                           // a1[k]: draws of ranks below k; P - a1[s] = TP* of a run from s
  const int lo = t * chunk, hi = lo + chunk < P ? lo + chunk : P;
  int32_t tot = 0;
  for (int k = lo; k < hi; ++k) tot += cu[k];
  int64_t L = (int64_t)(rk_block_scan(S, tot, nullptr) - tot);    // cU before this thread's ranks (every prefix <= Nn <= INT32_MAX)
  double ap = 0.0;
  int64_t num = 0;
  for (int k = lo; k < hi; ++k) {
    L += cu[k];
    const uint32_t key = keys[k];
    int s = k, e = k;                                             // the run of equal keys that holds k: [s, e]
    if (k > 0 && keys[k - 1] == key) s = rk_lower(keys, 0, k - 1, key);
    if (k + 1 < P && keys[k + 1] == key) e = rk_upper(keys, k + 2, P, key) - 1;
    const int64_t w = a0[k], tp = P - a1[s];
    // w == 0: nothing, by a select and not by a branch around the running sums (the note above ro_better).  The quotient may then
    // be 0 / 0: the top positive above every negative, and not drawn
    const double q = (double)(w * tp) / (double)(tp + Nn - L);
    ap += w != 0 ? q : 0.0;
    num += w * (2 * L + ce[e]);
  }
  red.d[t] = ap;
  __syncthreads();
  for (int d = RW_T / 2; d > 0; d >>= 1) {
    if (t < d) red.d[t] += red.d[t + d];
    __syncthreads();
  }
  ap_sum = red.d[0];
  __syncthreads();
  red.i[t] = num;
  __syncthreads();
  for (int d = RW_T / 2; d > 0; d >>= 1) {
    if (t < d) red.i[t] += red.i[t + d];
    __syncthreads();
  }
  num_sum = red.i[0];
}

// One workgroup = one replicate.  LDS: four arrays of ls >= P + 1 ints.  While the negatives are drawn they hold cum (the inclusive
// prefix of histU), histE, cU and cE; then cum's place takes w, and histE's the exclusive prefix of w.
__global__ void __launch_bounds__(RW_T) k_rb_boot(const int32_t *__restrict__ meta, const uint32_t *__restrict__ keys, int pc,
                                                  const int32_t *__restrict__ hist, uint32_t seed_lo, uint32_t seed_hi, int reps, int ls,
                                                  double *__restrict__ out16, double *__restrict__ rep_ap,
                                                  int64_t *__restrict__ rep_num, int32_t *__restrict__ hist_out, int64_t hstride) {
  extern __shared__ __attribute__((aligned(16))) int32_t rb_lds[];
  __shared__ RkScan S;
  __shared__ RbRed red;
  const int t = threadIdx.x;
  const uint32_t r = blockIdx.x;
  const int status = meta[5];
  const int P = meta[4];
  const int64_t Nn = (int64_t)meta[1] + meta[3];
  const int code = status != 0 ? status : (P > RB_MAXP ? RB_TOO_MANY : ((P < 2 || Nn < 2) ? RB_TOO_FEW : 0));
  if (r == 0 && t == 0) {
    out16[8] = (double)reps;  out16[9] = (double)P;  out16[10] = (double)Nn;
    out16[11] = 0.0;  out16[12] = 0.0;  out16[13] = 0.0;  out16[14] = 0.0;
    out16[15] = (double)code;
  }
  int32_t *ho = hist_out ? hist_out + (int64_t)r * hstride : nullptr;
  if (code != 0) {                                                // (uniform over the launch)
    if (t == 0) { rep_ap[r] = __longlong_as_double(0x7FF8000000000000ll);  rep_num[r] = 0; }
    if (ho) for (int64_t i = t; i < hstride; i += RW_T) ho[i] = 0;
    return;
  }
  int32_t *a0 = rb_lds, *a1 = a0 + ls, *cu = a1 + ls, *ce = cu + ls;       // P + 1 <= ls
  const int32_t *hu = hist, *he = hist + (pc + 1);
  const int chunk = (P + 1 + RW_T - 1) / RW_T;
  for (int i = t; i <= P; i += RW_T) { a0[i] = hu[i];  a1[i] = he[i];  cu[i] = 0;  ce[i] = 0; }
  __syncthreads();
  rb_prefix<false>(S, a0, P + 1, chunk);                          // cum[b]: negatives of bins 0 .. b; cum[P] = Nn
  {
    const uint64_t m = (uint64_t)Nn, calls = (m + 1) >> 1;
    for (uint64_t j = t; j < calls; j += RW_T) {
      uint64_t x[2];
      rb_philox(seed_lo, seed_hi, j, r, 1u, x[0], x[1]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (2 * j + h >= m) continue;                             // (an odd count: the last call is half used)
        const int32_t u = (int32_t)__umul64hi(x[h], m);           // < Nn <= INT32_MAX
        int b = rk_upper(a0, 0, P + 1, u);                        // entries of cum that are <= u
        b = b < P ? b : P;                                        // (cum[P] = Nn > u: never taken)
        atomicAdd(&cu[b], 1);
        if (b >= 1 && u - a0[b - 1] < a1[b - 1]) atomicAdd(&ce[b - 1], 1);     // one of the bin's first histE[b - 1] places
      }
    }
  }
  __syncthreads();
  for (int i = t; i <= P; i += RW_T) a0[i] = 0;                   // w (w[P] stays 0)
  __syncthreads();
  {
    const uint64_t m = (uint64_t)P, calls = (m + 1) >> 1;
    for (uint64_t j = t; j < calls; j += RW_T) {
      uint64_t x[2];
      rb_philox(seed_lo, seed_hi, j, r, 0u, x[0], x[1]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (2 * j + h >= m) continue;
        int k = (int)__umul64hi(x[h], m);
        k = k < P ? k : P - 1;                                    // (never taken)
        atomicAdd(&a0[k], 1);
      }
    }
  }
  __syncthreads();
  if (ho) {                                                       // tests only: w, cU, cE of this replicate, the rest of the row zero
    const int64_t third = hstride / 3;
    for (int64_t i = t; i < third; i += RW_T) {
      const bool in = i <= P;
      ho[i] = in ? a0[i] : 0;  ho[third + i] = in ? cu[i] : 0;  ho[2 * third + i] = in ? ce[i] : 0;
    }
  }
  double ap_sum;
  int64_t num;
  rb_terms(S, red, a0, a1, cu, ce, keys, P, Nn, chunk, ap_sum, num);
  if (t == 0) { rep_ap[r] = ap_sum / (double)P;  rep_num[r] = num; }
}

// ---- Paired stratified bootstrap of two models on the same labels (ggad_rank_bootstrap_pair_f32).  A replicate draws ELEMENTS, and
// every drawn element is counted at its own bin under A and under B.  An element is named by its number in position order --
// positive j: the j-th element with label 1; negative u: the u-th with label 0 -- which is the same thing under both models; the
// sorted ranks of k_rb_boot are not.  Replicate r draws P positive numbers on Philox stream 0 and Nn negative numbers on stream 1
// (rb_philox, its key, counter layout and draw rule) and, per model M,
//     w_M[rank_M(j)] += 1       rank_M(j): lower bound of the positive's key in M's sorted positives (a run of equal keys is counted
//                               at its first rank: the bins strictly inside a run are empty, so TP*, L* and cE[e] there are the run's)
//     cU_M[ub_M(u)] += 1        and cE_M[ub_M(u) - 1] += 1 when the negative ties the positive at ub_M(u) - 1
// then rb_terms.  k_rp_cells makes the per-element tables once per call: uint16 cells ub | tie << 15 per negative number and uint16
// ranks per positive number, one array per model, so that a replicate's pass over one model gathers 2 bytes per draw.
struct RpLayout {                         // two halves of the run-merge chain's words, then the four uint16 tables
  RwLayout L;
  int64_t n;
  int64_t half() const { return (L.total() + 3) & ~(int64_t)3; }
  int64_t cell_words() const { return ((n + 1) / 2 + 3) & ~(int64_t)3; }          // uint16 per negative number (Nn <= n)
  int64_t rank_words() const { return ((L.pc + 1) / 2 + 3) & ~(int64_t)3; }       // uint16 per positive number (P <= pc)
  int64_t o_cell(int m) const { return 2 * half() + m * cell_words(); }
  int64_t o_rank(int m) const { return 2 * half() + 2 * cell_words() + m * rank_words(); }
  int64_t total() const { return o_rank(2); }
};

static_assert(RB_MAXP < (1 << 15), "a cell holds ub <= P in 15 bits beside the tie bit; a rank is below P");

struct RpModel {                          // one model's words for k_rp_cells and k_rp_boot
  const int32_t *meta;
  const uint32_t *keys;
  uint16_t *cell, *rank;
};

// the call's status (out24[23]) from the two summaries: the first non-zero chain status, 8, 9, else 0 (the same labels: P and Nn of A)
__device__ __forceinline__ int rp_code(const int32_t *__restrict__ ma, const int32_t *__restrict__ mb) {
  const int sa = ma[5], sb = mb[5], P = ma[4];
  const int64_t Nn = (int64_t)ma[1] + ma[3];
  if (sa != 0) return sa;
  if (sb != 0) return sb;
  if (P < 2 || Nn < 2) return RB_TOO_FEW;
  return P > RB_MAXP ? RB_TOO_MANY : 0;
}

// One pass over the n elements in k_rw_scan's block ranges.  The numbering does not depend on the grid's schedule: a block's first
// positive and negative numbers are sums over the headers k_rw_scan left for the blocks before it (A's: the labels are shared), and
// inside a block every chunk of RW_T elements is numbered by a workgroup scan (both counts in one int: at most 1,024 each).
__global__ void __launch_bounds__(RW_T) k_rp_cells(const float *__restrict__ score_a, const float *__restrict__ score_b,
                                                   const uint8_t *__restrict__ label, int64_t n, int64_t per_block,
                                                   const int32_t *__restrict__ hdr, RpModel A, RpModel B) {
  __shared__ RkScan S;
  if (rp_code(A.meta, B.meta) != 0) return;                       // (uniform over the launch; with 0, P <= pc and P <= RB_MAXP)
  const int t = threadIdx.x, b = blockIdx.x;
  const int P = A.meta[4];
  const bool before = t < b;                                      // (b < RW_G <= RW_T: one thread per earlier header)
  int neg0 = rk_block_sum(S.wsum, before ? hdr[t * RW_HDR + 1] + hdr[t * RW_HDR + 3] : 0);
  int pos0 = rk_block_sum(S.wsum, before ? hdr[t * RW_HDR + 4] : 0);
  const int64_t lo = (int64_t)b * per_block;
  const int64_t hi = lo + per_block < n ? lo + per_block : n;
  for (int64_t base = lo; base < hi; base += RW_T) {              // (whole workgroup: the scan needs every thread)
    const int64_t i = base + t;
    const int y = i < hi ? label[i] : 2;
    const bool is_neg = y == 0, is_pos = y == 1;
    int total;
    const int incl = rk_block_scan(S, (is_neg ? 1 : 0) | (is_pos ? 1 << 16 : 0), &total);
    if (is_neg) {
      const int64_t u = (int64_t)neg0 + (incl & 0xFFFF) - 1;      // < Nn <= n
      const uint32_t ka = rk_key(score_a[i]), kb = rk_key(score_b[i]);
      const int ua = rk_upper(A.keys, 0, P, ka), ub = rk_upper(B.keys, 0, P, kb);
      A.cell[u] = (uint16_t)(ua | ((ua > 0 && A.keys[ua - 1] == ka) ? 1 << 15 : 0));
      B.cell[u] = (uint16_t)(ub | ((ub > 0 && B.keys[ub - 1] == kb) ? 1 << 15 : 0));
    } else if (is_pos) {
      const int j = pos0 + (incl >> 16) - 1;                      // < P
      A.rank[j] = (uint16_t)rk_lower(A.keys, 0, P, rk_key(score_a[i]));
      B.rank[j] = (uint16_t)rk_lower(B.keys, 0, P, rk_key(score_b[i]));
    }
    neg0 += total & 0xFFFF;
    pos0 += total >> 16;
  }
}

constexpr int RP_BATCH = 4;               // Philox calls of one thread whose 2 RP_BATCH gathers are in flight together
constexpr uint32_t RP_NONE = 0xFFFFu;     // no draw (ub = 32,767 cannot be)

// One workgroup = one replicate: model A completely, then model B from the same draws (counter-based: regenerated, not stored).
// LDS: k_rb_boot's four arrays of ls >= P + 1 ints -- w, rb_terms' scratch, cU, cE.  LDS integer atomics only.
__global__ void __launch_bounds__(RW_T) k_rp_boot(RpModel A, RpModel B, uint32_t seed_lo, uint32_t seed_hi, int reps, int ls,
                                                  double *__restrict__ out24, double *__restrict__ rep_ap,
                                                  int64_t *__restrict__ rep_num, int32_t *__restrict__ hist_out, int64_t hstride) {
  extern __shared__ __attribute__((aligned(16))) int32_t rb_lds[];
  __shared__ RkScan S;
  __shared__ RbRed red;
  const int t = threadIdx.x;
  const uint32_t r = blockIdx.x;
  const int P = A.meta[4];
  const int64_t Nn = (int64_t)A.meta[1] + A.meta[3];
  const int code = rp_code(A.meta, B.meta);
  if (r == 0 && t == 0) {
    out24[16] = (double)reps;  out24[17] = (double)P;  out24[18] = (double)Nn;
    out24[19] = 0.0;  out24[20] = 0.0;  out24[21] = 0.0;  out24[22] = 0.0;
    out24[23] = (double)code;
  }
  int32_t *ho = hist_out ? hist_out + (int64_t)r * hstride : nullptr;
  if (code != 0) {                                                // (uniform over the launch)
    if (t < 2) { rep_ap[t * reps + r] = __longlong_as_double(0x7FF8000000000000ll);  rep_num[t * reps + r] = 0; }
    if (ho) for (int64_t i = t; i < hstride; i += RW_T) ho[i] = 0;
    return;
  }
  int32_t *a0 = rb_lds, *a1 = a0 + ls, *cu = a1 + ls, *ce = cu + ls;       // P + 1 <= ls
  const int chunk = (P + 1 + RW_T - 1) / RW_T;
  const int64_t third = hstride / 6;
#pragma unroll 1
  for (int model = 0; model < 2; ++model) {
    const RpModel &M = model ? B : A;
    const uint16_t *__restrict__ cell = M.cell, *__restrict__ rank = M.rank;
    __syncthreads();                                              // (the model before has read its histograms)
    for (int i = t; i <= P; i += RW_T) { a0[i] = 0;  cu[i] = 0;  ce[i] = 0; }
    __syncthreads();
    {
      const uint64_t m = (uint64_t)Nn, calls = (m + 1) >> 1;
      for (uint64_t j0 = t; j0 < calls; j0 += (uint64_t)RP_BATCH * RW_T) {
        uint32_t c[2 * RP_BATCH];
#pragma unroll
        for (int q = 0; q < RP_BATCH; ++q) {
          const uint64_t j = j0 + (uint64_t)q * RW_T;
          uint64_t x[2] = {0, 0};
          if (j < calls) rb_philox(seed_lo, seed_hi, j, r, 1u, x[0], x[1]);
#pragma unroll
          for (int h = 0; h < 2; ++h)                             // (an odd count: the last call is half used)
            c[2 * q + h] = 2 * j + h < m ? (uint32_t)cell[__umul64hi(x[h], m)] : RP_NONE;      // negative number < Nn
        }
#pragma unroll
        for (int q = 0; q < 2 * RP_BATCH; ++q) {
          if (c[q] == RP_NONE) continue;
          const int bin = (int)(c[q] & 0x7FFFu);                  // <= P
          atomicAdd(&cu[bin], 1);
          if ((c[q] >> 15) && bin >= 1) atomicAdd(&ce[bin - 1], 1);
        }
      }
    }
    {
      const uint64_t m = (uint64_t)P, calls = (m + 1) >> 1;
      for (uint64_t j = t; j < calls; j += RW_T) {
        uint64_t x[2];
        rb_philox(seed_lo, seed_hi, j, r, 0u, x[0], x[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (2 * j + h >= m) continue;
          int k = (int)rank[__umul64hi(x[h], m)];                 // positive number < P
          k = k < P ? k : P - 1;                                  // (never taken)
          atomicAdd(&a0[k], 1);
        }
      }
    }
    __syncthreads();
    if (ho) {                                                     // tests only: w, cU, cE of this model, the rest of the row zero
      int32_t *hm = ho + 3 * third * model;
      for (int64_t i = t; i < third; i += RW_T) {
        const bool in = i <= P;
        hm[i] = in ? a0[i] : 0;  hm[third + i] = in ? cu[i] : 0;  hm[2 * third + i] = in ? ce[i] : 0;
      }
    }
    double ap_sum;
    int64_t num;
    rb_terms(S, red, a0, a1, cu, ce, M.keys, P, Nn, chunk, ap_sum, num);
    if (t == 0) { rep_ap[model * reps + r] = ap_sum / (double)P;  rep_num[model * reps + r] = num; }
  }
}

}  // namespace

extern "C" {

int32_t ggad_rank_metrics_max_pos(void) { return RM_CAP; }
int32_t ggad_rank_wide_max_pos(void) { return RW_MAX; }

int64_t ggad_rank_metrics_workspace_elems(int64_t n) {
  if (n < 0 || n > INT32_MAX) return 0;
  return rm_layout(n).total();
}

int64_t ggad_rank_wide_workspace_elems(int64_t n, int64_t pos_cap) {
  if (!rw_args_ok(n, pos_cap)) return 0;
  return rw_layout(n, pos_cap).total();
}

int ggad_rank_metrics_f32(const float *score, const uint8_t *label, int64_t n, float thres, double *out8, int32_t *workspace,
                          ggad_stream_t stream) {
  GGAD_REQUIRE(out8 && workspace && n >= 0 && n <= INT32_MAX && (n == 0 || (score && label)));
  const RmLayout L = rm_layout(n);
  static ggad_lds_optin lds;
  const int ready = ggad_lds_opt_in(lds, RW_BUCKET_LDS, k_rm_bucket);
  if (ready == 0) return GGAD_E_INVALID;
  if (ready != 1) { ggad_set_error(hipErrorInvalidValue, "rank_metrics: this device cannot give k_rm_bucket its LDS"); return GGAD_E_LAUNCH; }
  hipStream_t st = as_stream(stream);
  int32_t *hdr = workspace + L.o_hdr(), *meta = workspace + L.o_meta(), *hist = workspace + L.o_hist();
  uint32_t *keys = reinterpret_cast<uint32_t *>(workspace + L.o_keys()), *seg = reinterpret_cast<uint32_t *>(workspace + L.o_seg());
  k_rm_scan<<<dim3(L.g), dim3(RW_T), 0, st>>>(score, label, n, thres, L.per_block, (int)L.seg_cap, hdr, seg, hist);
  GGAD_CHECK_LAUNCH("rank_metrics scan");
  k_rm_sort<<<dim3(1), dim3(RW_T), 0, st>>>(hdr, L.g, (int)L.seg_cap, seg, meta, keys);
  GGAD_CHECK_LAUNCH("rank_metrics sort");
  int64_t gb = (n + 16 * RW_T - 1) / (16 * RW_T);
  gb = gb < 1 ? 1 : (gb > RM_GB ? RM_GB : gb);
  k_rm_bucket<<<dim3((unsigned)gb), dim3(RW_T), RW_BUCKET_LDS, st>>>(score, label, n, meta, keys, hist);
  GGAD_CHECK_LAUNCH("rank_metrics bucket");
  k_rm_finish<<<dim3(1), dim3(RW_T), 0, st>>>(meta, keys, hist, out8);
  GGAD_CHECK_LAUNCH("rank_metrics finish");
  return GGAD_OK;
}

int ggad_rank_wide_f32(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, double *out8,
                       int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(out8 && workspace && ((uintptr_t)workspace & 15) == 0 && rw_args_ok(n, pos_cap) && (n == 0 || (score && label)));
  RwFront F;
  const int rc = rw_front(score, label, n, pos_cap, thres, workspace, stream, F);
  if (rc != GGAD_OK) return rc;
  k_rw_terms<<<dim3(F.L.tc), dim3(RW_T), 0, F.st>>>(F.meta, F.keys, (int)F.L.pc, F.hist, F.part_ap, F.part_num);
  GGAD_CHECK_LAUNCH("rank_wide terms");
  k_rw_final<<<dim3(1), dim3(RW_TMAX), 0, F.st>>>(F.meta, F.part_ap, F.part_num, out8);
  GGAD_CHECK_LAUNCH("rank_wide final");
  return GGAD_OK;
}

int32_t ggad_rank_operating_criteria(void) { return RO_CRITERIA; }

int64_t ggad_rank_operating_workspace_elems(int64_t n, int64_t pos_cap) {
  if (!rw_args_ok(n, pos_cap)) return 0;
  return rw_layout(n, pos_cap).total_op();
}

int ggad_rank_operating_f32(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, int32_t criterion,
                            double param, double *out16, float *curve_thres, int32_t *curve_tp, int32_t *curve_fp, int32_t *workspace,
                            ggad_stream_t stream) {
  GGAD_REQUIRE(out16 && workspace && ((uintptr_t)workspace & 15) == 0 && rw_args_ok(n, pos_cap) && (n == 0 || (score && label)));
  GGAD_REQUIRE(criterion >= 0 && criterion < RO_CRITERIA && (criterion < 3 || (param >= 0.0 && param <= 1.0)));
  GGAD_REQUIRE((curve_thres != nullptr) == (curve_tp != nullptr) && (curve_tp != nullptr) == (curve_fp != nullptr));
  RwFront F;
  const int rc = rw_front(score, label, n, pos_cap, thres, workspace, stream, F);
  if (rc != GGAD_OK) return rc;
  const RoArgs A = {criterion, criterion < 3 ? 0.0 : param, curve_thres, curve_tp, curve_fp, workspace + F.L.o_op()};
  k_ro_terms<<<dim3(F.L.tc), dim3(RW_T), 0, F.st>>>(F.meta, F.keys, (int)F.L.pc, F.hist, F.part_ap, F.part_num, A);
  GGAD_CHECK_LAUNCH("rank_operating terms");
  k_ro_final<<<dim3(1), dim3(RW_TMAX), 0, F.st>>>(F.meta, F.part_ap, F.part_num, A.part, criterion, out16);
  GGAD_CHECK_LAUNCH("rank_operating final");
  return GGAD_OK;
}

int64_t ggad_rank_delong_workspace_elems(int64_t n, int64_t pos_cap) {
  if (!rw_args_ok(n, pos_cap)) return 0;
  return RdLayout{rw_layout(n, pos_cap)}.total();
}

int64_t ggad_rank_delong_pair_workspace_elems(int64_t n, int64_t pos_cap) {
  if (!rw_args_ok(n, pos_cap)) return 0;
  return RdLayout{rw_layout(n, pos_cap)}.total_pair();
}

int ggad_rank_delong_f32(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, double *out16,
                         int64_t *sums, int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(out16 && sums && workspace && ((uintptr_t)workspace & 15) == 0 && rw_args_ok(n, pos_cap) && (n == 0 || (score && label)));
  const RdLayout D{rw_layout(n, pos_cap)};
  RdModel M;
  hipStream_t st;
  const int rc = rd_model(score, label, n, pos_cap, thres, workspace, stream, D, false, M, st);
  if (rc != GGAD_OK) return rc;
  k_rd_final<<<dim3(1), dim3(RW_TMAX), 0, st>>>(M, out16, sums);
  GGAD_CHECK_LAUNCH("rank_delong final");
  return GGAD_OK;
}

int ggad_rank_delong_pair_f32(const float *score_a, const float *score_b, const uint8_t *label, int64_t n, int64_t pos_cap, float thres,
                              double *out24, int64_t *sums, int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(out24 && sums && workspace && ((uintptr_t)workspace & 15) == 0 && rw_args_ok(n, pos_cap) &&
               (n == 0 || (score_a && score_b && label)));
  const RdLayout D{rw_layout(n, pos_cap)};
  RdModel A, B;
  hipStream_t st;
  int rc = rd_model(score_a, label, n, pos_cap, thres, workspace, stream, D, true, A, st);
  if (rc != GGAD_OK) return rc;
  rc = rd_model(score_b, label, n, pos_cap, thres, workspace + D.half(), stream, D, true, B, st);
  if (rc != GGAD_OK) return rc;
  uint64_t *part_x = reinterpret_cast<uint64_t *>(workspace + D.o_cross());
  int64_t xg = (n + 4 * RW_T - 1) / (4 * RW_T);
  xg = xg < 1 ? 1 : (xg > RD_XG ? RD_XG : xg);
  k_rd_cross<<<dim3((unsigned)xg), dim3(RW_T), 0, st>>>(score_a, score_b, label, n, (int)D.L.pc, A, B, part_x);
  GGAD_CHECK_LAUNCH("rank_delong cross");
  k_rd_pair_final<<<dim3(1), dim3(RD_XG), 0, st>>>(A, B, part_x, (int)xg, out24, sums);
  GGAD_CHECK_LAUNCH("rank_delong pair final");
  return GGAD_OK;
}

int32_t ggad_rank_bootstrap_max_pos(void) { return RB_MAXP; }
int32_t ggad_rank_bootstrap_max_reps(void) { return RB_MAXREPS; }

int64_t ggad_rank_bootstrap_workspace_elems(int64_t n, int64_t pos_cap) {
  if (!rw_args_ok(n, pos_cap)) return 0;
  return rw_layout(n, pos_cap).total();
}

int ggad_rank_bootstrap_f32(const float *score, const uint8_t *label, int64_t n, int64_t pos_cap, float thres, uint64_t seed,
                            int32_t reps, double *out16, double *rep_ap, int64_t *rep_auc_num, int32_t *hist_out, int32_t *workspace,
                            ggad_stream_t stream) {
  GGAD_REQUIRE(out16 && rep_ap && rep_auc_num && workspace && ((uintptr_t)workspace & 15) == 0 && rw_args_ok(n, pos_cap) &&
               (n == 0 || (score && label)));
  GGAD_REQUIRE(reps >= 1 && reps <= RB_MAXREPS);
  static ggad_lds_optin lds;
  const int ready = ggad_lds_opt_in(lds, RB_LDS_MAX, k_rb_boot);
  if (ready == 0) return GGAD_E_INVALID;
  if (ready != 1) { ggad_set_error(hipErrorInvalidValue, "rank_bootstrap: this device cannot give k_rb_boot its LDS"); return GGAD_E_LAUNCH; }
  RwFront F;
  const int rc = rw_front(score, label, n, pos_cap, thres, workspace, stream, F);
  if (rc != GGAD_OK) return rc;
  k_rw_terms<<<dim3(F.L.tc), dim3(RW_T), 0, F.st>>>(F.meta, F.keys, (int)F.L.pc, F.hist, F.part_ap, F.part_num);
  GGAD_CHECK_LAUNCH("rank_bootstrap terms");
  k_rw_final<<<dim3(1), dim3(RW_TMAX), 0, F.st>>>(F.meta, F.part_ap, F.part_num, out16);
  GGAD_CHECK_LAUNCH("rank_bootstrap final");
  const int ls = (int)(F.L.pc < RB_MAXP ? F.L.pc : RB_MAXP) + 1;  // the LDS follows from (n, pos_cap) alone, like every grid here
  k_rb_boot<<<dim3((unsigned)reps), dim3(RW_T), (size_t)4 * ls * 4, F.st>>>(F.meta, F.keys, (int)F.L.pc, F.hist, (uint32_t)seed,
                                                                            (uint32_t)(seed >> 32), reps, ls, out16, rep_ap, rep_auc_num,
                                                                            hist_out, 3 * (pos_cap + 1));
  GGAD_CHECK_LAUNCH("rank_bootstrap replicates");
  return GGAD_OK;
}

int64_t ggad_rank_bootstrap_pair_workspace_elems(int64_t n, int64_t pos_cap) {
  if (!rw_args_ok(n, pos_cap)) return 0;
  return RpLayout{rw_layout(n, pos_cap), n}.total();
}

int ggad_rank_bootstrap_pair_f32(const float *score_a, const float *score_b, const uint8_t *label, int64_t n, int64_t pos_cap,
                                 float thres, uint64_t seed, int32_t reps, double *out24, double *rep_ap, int64_t *rep_auc_num,
                                 int32_t *hist_out, int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(out24 && rep_ap && rep_auc_num && workspace && ((uintptr_t)workspace & 15) == 0 && rw_args_ok(n, pos_cap) &&
               (n == 0 || (score_a && score_b && label)));
  GGAD_REQUIRE(reps >= 1 && reps <= RB_MAXREPS);
  static ggad_lds_optin lds;
  const int ready = ggad_lds_opt_in(lds, RB_LDS_MAX, k_rp_boot);
  if (ready == 0) return GGAD_E_INVALID;
  if (ready != 1) { ggad_set_error(hipErrorInvalidValue, "rank_bootstrap_pair: this device cannot give k_rp_boot its LDS"); return GGAD_E_LAUNCH; }
  const RpLayout D{rw_layout(n, pos_cap), n};
  RpModel M[2];
  RwFront F;
  for (int m = 0; m < 2; ++m) {
    const int rc = rw_front(m ? score_b : score_a, label, n, pos_cap, thres, workspace + m * D.half(), stream, F);
    if (rc != GGAD_OK) return rc;
    k_rw_terms<<<dim3(F.L.tc), dim3(RW_T), 0, F.st>>>(F.meta, F.keys, (int)F.L.pc, F.hist, F.part_ap, F.part_num);
    GGAD_CHECK_LAUNCH("rank_bootstrap_pair terms");
    k_rw_final<<<dim3(1), dim3(RW_TMAX), 0, F.st>>>(F.meta, F.part_ap, F.part_num, out24 + 8 * m);
    GGAD_CHECK_LAUNCH("rank_bootstrap_pair final");
    M[m] = {F.meta, F.keys, reinterpret_cast<uint16_t *>(workspace + D.o_cell(m)), reinterpret_cast<uint16_t *>(workspace + D.o_rank(m))};
  }
  k_rp_cells<<<dim3(D.L.g), dim3(RW_T), 0, F.st>>>(score_a, score_b, label, n, D.L.per_block, workspace + D.L.o_hdr(), M[0], M[1]);
  GGAD_CHECK_LAUNCH("rank_bootstrap_pair cells");
  const int ls = (int)(D.L.pc < RB_MAXP ? D.L.pc : RB_MAXP) + 1;
  k_rp_boot<<<dim3((unsigned)reps), dim3(RW_T), (size_t)4 * ls * 4, F.st>>>(M[0], M[1], (uint32_t)seed, (uint32_t)(seed >> 32), reps, ls, out24,
                                                                            rep_ap, rep_auc_num, hist_out, 6 * (pos_cap + 1));
  GGAD_CHECK_LAUNCH("rank_bootstrap_pair replicates");
  return GGAD_OK;
}

}  // extern "C"
