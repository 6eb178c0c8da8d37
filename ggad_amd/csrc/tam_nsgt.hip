// TAM's truncation round (`graph_nsgt` + `normalize_adj_tensor`, reference utils_tam.py:222-240 / :45-53) on the device.
//
// The current graph is a byte mask `alive` over the CSR entries of raw = A + I (sorted columns, symmetric pattern): a round never
// needs an entry outside raw's pattern and removes about 1 % of the entries, so it is a few streaming passes over nnz entries:
//
//   k_transpose_map   once per run: tpos[e] = CSR position of (j, i) for e = (i, j)          (binary search of row j)
//   k_rowstat         per row over the live entries: count, max distance, count of non-zero distances
//   k_compact         per row, ascending columns: the live non-zero distances (mode 0) or (col, r_i r_j) of the live entries (mode 1)
//                     at the offsets of an exclusive scan of the row counts (ggad_exclusive_scan_i32, plan.hip)
//   k_cut_keep        keep[e]  = alive[e] && !(dis[e] > thr[row])
//   k_cut_sym         alive[e] = keep[e] | keep[tpos[e]]                                      (adj + adj.T of the reference)
//
// One wave per row, lanes striding the row: the loads of a wave are consecutive, the per-row value (threshold, offset) is uniform.
// Rows of tens of thousands of entries are walked by one wave too (a few hundred iterations): this is bandwidth over nnz once per
// round, not a latency-critical path.  No floating-point atomics, no grid-wide waiting; the only atomic is an integer OR on the
// status word of the transpose map.
#include "common.h"

namespace {

constexpr int NSGT_T = 256;                          // threads per block
constexpr int NSGT_ROWS = NSGT_T / GGAD_WAVE;        // rows (waves) per block

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, GGAD_WAVE));
  return v;
}

__global__ void __launch_bounds__(NSGT_T) k_transpose_map(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int n,
                                                          int32_t *__restrict__ tpos, int32_t *__restrict__ status) {
  const int i = blockIdx.x * NSGT_ROWS + (int)(threadIdx.x / GGAD_WAVE);
  if (i >= n) return;
  const int beg = rowptr[i], end = rowptr[i + 1];
  for (int e = beg + lane_id(); e < end; e += GGAD_WAVE) {
    const int j = col[e];
    int p = e, bad = 2;                               // 2: a column outside the matrix (nothing is read through it)
    if (j >= 0 && j < n) {
      const int jb = rowptr[j], je = rowptr[j + 1];
      const int q = lower_bound_i32(col, jb, je, i);
      if (q < je && col[q] == i) { p = q; bad = 0; } else bad = 1;      // 1: entry (j, i) is missing
    }
    tpos[e] = p;
    if (bad) atomicOr(status, bad);
  }
}

__global__ void __launch_bounds__(NSGT_T) k_rowstat(const int32_t *__restrict__ rowptr, const float *__restrict__ dis,
                                                    const uint8_t *__restrict__ alive, int n, int32_t *__restrict__ cnt,
                                                    float *__restrict__ mx, int32_t *__restrict__ nzcnt) {
  const int i = blockIdx.x * NSGT_ROWS + (int)(threadIdx.x / GGAD_WAVE);
  if (i >= n) return;
  const int beg = rowptr[i], end = rowptr[i + 1];
  int c = 0, z = 0;
  float m = -INFINITY;
  for (int e = beg + lane_id(); e < end; e += GGAD_WAVE) {
    if (alive[e]) {
      const float d = dis[e];
      ++c;
      z += (d != 0.0f) ? 1 : 0;
      m = fmaxf(m, d);
    }
  }
  c = wave_sum_i(c);
  z = wave_sum_i(z);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, GGAD_WAVE));
  if (lane_id() == 0) { cnt[i] = c; mx[i] = m; nzcnt[i] = z; }
}

// MODE 0: out_val = the non-zero distances of the live entries; MODE 1: (out_col, out_val) = (j, r_i * r_j) of the live entries.
// A wave walks its row in chunks of 64 consecutive entries and places the selected ones of a chunk by their rank in the ballot, so the
// output keeps the row's ascending column order.  Nothing is written at or past out_rowptr[i + 1]: counts that disagree with the mask
// lose entries, they never write outside the row's range.
template <int MODE>
__global__ void __launch_bounds__(NSGT_T) k_compact(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const float *__restrict__ dis, const uint8_t *__restrict__ alive, int n,
                                                    const float *__restrict__ r, const int32_t *__restrict__ out_rowptr,
                                                    int32_t *__restrict__ out_col, float *__restrict__ out_val) {
  const int i = blockIdx.x * NSGT_ROWS + (int)(threadIdx.x / GGAD_WAVE);
  if (i >= n) return;
  const int beg = rowptr[i], end = rowptr[i + 1], lane = lane_id();
  const int obeg = out_rowptr[i], oend = out_rowptr[i + 1];
  float ri = 0.0f;
  if (MODE == 1) ri = r[i];
  int off = obeg;
  for (int base = beg; base < end; base += GGAD_WAVE) {
    const int e = base + lane;
    bool sel = false;
    float d = 0.0f;
    if (e < end && alive[e]) {
      if (MODE == 0) { d = dis[e]; sel = (d != 0.0f); } else sel = true;
    }
    const unsigned long long bal = __ballot(sel);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
    const int pos = off + rank;
    if (sel && pos < oend) {
      if (MODE == 0) {
        out_val[pos] = d;
      } else {
        const int j = col[e];
        out_col[pos] = j;
        out_val[pos] = __fmul_rn(ri, r[j]);            // ONE rounded fp32 product, never part of an fma
      }
    }
    off += __popcll(bal);
  }
}

__global__ void __launch_bounds__(NSGT_T) k_cut_keep(const int32_t *__restrict__ rowptr, const float *__restrict__ dis,
                                                     const uint8_t *__restrict__ alive, const float *__restrict__ thr, int n,
                                                     uint8_t *__restrict__ keep) {
  const int i = blockIdx.x * NSGT_ROWS + (int)(threadIdx.x / GGAD_WAVE);
  if (i >= n) return;
  const int beg = rowptr[i], end = rowptr[i + 1];
  const float t = thr[i];
  for (int e = beg + lane_id(); e < end; e += GGAD_WAVE) keep[e] = (alive[e] && !(dis[e] > t)) ? 1 : 0;
}

__global__ void __launch_bounds__(NSGT_T) k_cut_sym(const uint8_t *__restrict__ keep, const int32_t *__restrict__ tpos, int64_t nnz,
                                                    uint8_t *__restrict__ alive) {
  const int64_t e = (int64_t)blockIdx.x * NSGT_T + threadIdx.x;
  if (e >= nnz) return;
  alive[e] = keep[e] | keep[tpos[e]];
}

inline unsigned row_blocks(int32_t n) { return (unsigned)((n + NSGT_ROWS - 1) / NSGT_ROWS); }

}  // namespace

extern "C" {

int ggad_tam_nsgt_transpose_map(const int32_t *rowptr, const int32_t *col, int32_t n, int32_t *tpos, int32_t *status,
                                ggad_stream_t stream) {
  GGAD_REQUIRE(rowptr && col && tpos && status && n >= 0);
  hipStream_t st = as_stream(stream);
  (void)hipMemsetAsync(status, 0, sizeof(int32_t), st);
  GGAD_CHECK_LAUNCH("tam_nsgt_transpose_map memset");
  if (n == 0) return GGAD_OK;
  k_transpose_map<<<dim3(row_blocks(n)), dim3(NSGT_T), 0, st>>>(rowptr, col, n, tpos, status);
  GGAD_CHECK_LAUNCH("tam_nsgt_transpose_map");
  return GGAD_OK;
}

int ggad_tam_nsgt_rowstat(const int32_t *rowptr, const float *dis, const uint8_t *alive, int32_t n, int32_t *cnt, float *mx,
                          int32_t *nzcnt, ggad_stream_t stream) {
  GGAD_REQUIRE(rowptr && dis && alive && cnt && mx && nzcnt && n >= 0);
  if (n == 0) return GGAD_OK;
  k_rowstat<<<dim3(row_blocks(n)), dim3(NSGT_T), 0, as_stream(stream)>>>(rowptr, dis, alive, n, cnt, mx, nzcnt);
  GGAD_CHECK_LAUNCH("tam_nsgt_rowstat");
  return GGAD_OK;
}

int ggad_tam_nsgt_compact(const int32_t *rowptr, const int32_t *col, const float *dis, const uint8_t *alive, int32_t n, int32_t mode,
                          const int32_t *counts, const float *r, int32_t *out_rowptr, int32_t *out_col, float *out_val,
                          int32_t *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(rowptr && col && dis && alive && counts && out_rowptr && out_val && workspace && n >= 0);
  GGAD_REQUIRE(mode == 0 || (mode == 1 && r && out_col));
  const int rc = ggad_exclusive_scan_i32(counts, out_rowptr, n, workspace, stream);      // out_rowptr[n] = the total
  if (rc != GGAD_OK) return rc;
  if (n == 0) return GGAD_OK;
  hipStream_t st = as_stream(stream);
  if (mode == 0)
    k_compact<0><<<dim3(row_blocks(n)), dim3(NSGT_T), 0, st>>>(rowptr, col, dis, alive, n, r, out_rowptr, out_col, out_val);
  else
    k_compact<1><<<dim3(row_blocks(n)), dim3(NSGT_T), 0, st>>>(rowptr, col, dis, alive, n, r, out_rowptr, out_col, out_val);
  GGAD_CHECK_LAUNCH("tam_nsgt_compact");
  return GGAD_OK;
}

int ggad_tam_nsgt_cut(const int32_t *rowptr, const float *dis, const int32_t *tpos, const float *thr, int32_t n, int64_t nnz,
                      uint8_t *alive, uint8_t *keep, ggad_stream_t stream) {
  GGAD_REQUIRE(rowptr && dis && tpos && thr && alive && keep && n >= 0 && nnz >= 0 && nnz < ((int64_t)1 << 31));
  GGAD_REQUIRE((const void *)alive != (const void *)keep);
  if (n == 0 || nnz == 0) return GGAD_OK;
  hipStream_t st = as_stream(stream);
  k_cut_keep<<<dim3(row_blocks(n)), dim3(NSGT_T), 0, st>>>(rowptr, dis, alive, thr, n, keep);
  GGAD_CHECK_LAUNCH("tam_nsgt_cut keep");
  k_cut_sym<<<dim3((unsigned)((nnz + NSGT_T - 1) / NSGT_T)), dim3(NSGT_T), 0, st>>>(keep, tpos, nnz, alive);      // reads keep at other rows
  GGAD_CHECK_LAUNCH("tam_nsgt_cut sym");
  return GGAD_OK;
}

}  // extern "C"
