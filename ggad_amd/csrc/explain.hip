// Exact attribution of the GGAD inference logit (ggad_explain_f32): why is this node in the ranked list?
//
// The score of row i of a sweep has no bias and one ReLU (k_score, step.hip):
//   a = W x1_i,   z = sum_d w_d relu(a[d]),   score = sigmoid(z),   x1_i = sum_{j in N(i)+{i}} omega_ij feat[j],
//   omega_ij = (1 / sqrt(r_i)) / sqrt(c_j):  r_i the size of the closed row, c_j the rows -- with multiplicity -- of row i's slice of
//   batch_size ids whose closed row holds j (quirk 2: the aggregation normalises per slice).
// With g[f] = sum_d w_d [a[d] > 0] W[d, f] the logit is linear where the ReLU pattern holds:  z = sum_f g[f] x1[f] (per feature)
// = sum_j omega_ij (g . feat[j]) (per neighbour).  Both are complete: no baseline, no sampling.
//
// One workgroup of 256 threads per explained position; everything is recomputed from the CSR graph, the feature table, the scored id
// list and the parameter block (no plan, no cached row):
//   1. the closed row: the sorted columns of i with i merged in (ids ascending)
//   2. c_j: every closed row of the slice -- one wave per row, a lane per entry -- is looked up in row i's list by binary search and
//      bumps an int32 counter (LDS / device atomics on INTEGERS: the result does not depend on their order)
//   3. x1[f]: the list is cut into NG contiguous pieces (NG depends on F alone), each summed with fma in ascending j, the pieces added
//      in ascending order; a[d]: k_score's fma chain over f ascending, channel d = lane + 64 j of the wide convention owned by lane
//      `lane` of wave j; z over d ascending; g[f] over d ascending
//   4. t_j = omega_ij * (g . feat[j]), the dot over f ascending, one thread per j
//   5. the m greatest t_j (signed; equal values by ascending id) by m arg-max rounds over 64-bit keys; `rest` = the others, 256
//      contiguous pieces in ascending j, the pieces added in ascending order
// Every float sum has one fixed order: equal inputs give equal bits.  No float atomic anywhere.
//
// Two branches by closed-row size, chosen per row at the kernel's entry: up to EX_LDS_ROWS entries the ids, counters and contributions
// stay in LDS (the launch asks for the LDS of min(n_rows_max_closed, EX_LDS_ROWS) entries; the contributions and counters are copied
// to the workspace at the end: the dump the tests read); longer rows (hubs) keep all three in the caller's workspace, the counters
// read and written with device-scope atomics.
#include "rank_common.h"
#include "step_common.h"

namespace {

constexpr int EX_T = 256;                 // threads of a workgroup: thread t owns channel t (D <= 256)
constexpr int EX_MAX_M = 32;              // listed neighbours per row
constexpr int EX_MAX_F = GGAD_MAX_F;      // 1024
constexpr int EX_LDS_ROWS = 12288;        // closed-row entries of the LDS branch: 12 bytes each
// LDS, in 4-byte words: x1[F] | g[F] (before it: the NG partial sums of x1, NG * F <= 1024) | w_d [a_d > 0] | 256 scratch | 64 misc
// | ids, counters, contributions of the row.  (2,624 + 3 * 12,288) * 4 = 157,952 of the 163,840 bytes of a workgroup.
constexpr int EX_O_X1 = 0, EX_O_G = EX_MAX_F, EX_O_GW = 2 * EX_MAX_F, EX_O_RED = EX_O_GW + EX_T, EX_O_MISC = EX_O_RED + EX_T,
              EX_O_ROWS = EX_O_MISC + 64;
constexpr int EX_LDS = (EX_O_ROWS + 3 * EX_LDS_ROWS) * 4;
static_assert(EX_LDS <= 160 * 1024, "explain: LDS of one workgroup");

enum { EX_ST_OK = 0, EX_ST_CAPACITY = 2, EX_ST_NAN = 3, EX_ST_POSITION = 5 };

struct ExOut {
  float *logit, *feature;
  int32_t *closed_size;
  int64_t *nbr_id;
  float *nbr_contrib;
  int32_t *nbr_colcount;
  float *rest;
  int64_t *meta;
};

template <bool WS>
__device__ __forceinline__ int ex_cnt(const int32_t *c, int j) {
  if (WS) return __hip_atomic_load(c + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return c[j];
}
template <bool WS>
__device__ __forceinline__ void ex_cnt_zero(int32_t *c, int j) {
  if (WS) __hip_atomic_store(c + j, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else c[j] = 0;
}
template <bool WS>
__device__ __forceinline__ void ex_cnt_bump(int32_t *c, int j) {
  if (WS) __hip_atomic_fetch_add(c + j, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else __hip_atomic_fetch_add(c + j, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// u in the sorted list: bump its counter
template <bool WS>
__device__ __forceinline__ void ex_hit(const int32_t *lst, int32_t *cnt, int r, int u) {
  int lo = 0, hi = r;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (lst[mid] < u) lo = mid + 1; else hi = mid; }
  if (lo < r && lst[lo] == u) ex_cnt_bump<WS>(cnt, lo);
}

__device__ __forceinline__ void ex_status(int64_t *meta, int st) {
  atomicMax(reinterpret_cast<unsigned long long *>(meta), (unsigned long long)st);
}

// the key of contribution t at list index q: greater = listed earlier (t descending, -0.0 ties with +0.0; then q ascending)
__device__ __forceinline__ unsigned long long ex_key(float t, int q) {
  return ((unsigned long long)rk_key(t) << 32) | (unsigned long long)(~(uint32_t)q);
}

__device__ __forceinline__ unsigned long long ex_block_max(unsigned long long v, unsigned long long *w4) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, GGAD_WAVE);
    v = o > v ? o : v;
  }
  if (lane_id() == 0) w4[threadIdx.x / GGAD_WAVE] = v;
  __syncthreads();
  unsigned long long b = w4[0];
#pragma unroll
  for (int w = 1; w < EX_T / GGAD_WAVE; ++w) b = w4[w] > b ? w4[w] : b;
  __syncthreads();
  return b;
}

// a row that is not explained (its status is already set): every output of slot k holds its padding
__device__ void ex_blank(const ExOut &O, int k, int F, int m, int closed) {
  const int tid = threadIdx.x;
  for (int f = tid; f < F; f += EX_T) O.feature[(int64_t)k * F + f] = 0.0f;
  if (tid < m) {
    O.nbr_id[(int64_t)k * m + tid] = -1;
    O.nbr_contrib[(int64_t)k * m + tid] = 0.0f;
    O.nbr_colcount[(int64_t)k * m + tid] = 0;
  }
  if (tid == 0) { O.logit[k] = 0.0f; O.rest[k] = 0.0f; O.closed_size[k] = closed; }
}

template <bool WS>
__device__ void ex_row(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int n_nodes, const float *__restrict__ feat,
                       const float *__restrict__ params, ParamLayout L, const int64_t *__restrict__ ids, int s0, int s1, int k, int m,
                       int i, int lo, int self_at, bool has_self, int r, float *lds, int32_t *lst, int32_t *cnt, float *tt,
                       int32_t *dump_c, float *dump_t, const ExOut &O) {
  const int tid = threadIdx.x, lane = lane_id(), wave = tid / GGAD_WAVE;
  const int D = L.D, F = L.F;
  float *x1 = lds + EX_O_X1, *g = lds + EX_O_G, *gw = lds + EX_O_GW, *red = lds + EX_O_RED;
  unsigned long long *w4 = reinterpret_cast<unsigned long long *>(lds + EX_O_MISC);
  float *zs = lds + EX_O_MISC + 16;
  bool nan = false;

  // 1. the closed row, ids ascending
  for (int q = tid; q < r; q += EX_T) {
    int v;
    if (has_self) v = col[lo + q];
    else v = q < self_at ? col[lo + q] : (q == self_at ? i : col[lo + q - 1]);
    lst[q] = v;
    ex_cnt_zero<WS>(cnt, q);
  }
  __syncthreads();

  // 2. c_j over the closed rows of the slice (row i's own among them; an id that stands twice in the slice counts twice)
  const int first = lst[0], last = lst[r - 1];
  for (int s = s0 + wave; s < s1; s += EX_T / GGAD_WAVE) {
    const int64_t v64 = ids[s];
    if (v64 < 0 || v64 >= n_nodes) {                                    // (wave-uniform) not a node: the slice cannot be counted
      if (lane == 0) ex_status(O.meta, EX_ST_POSITION);
      continue;
    }
    const int v = (int)v64, vlo = rowptr[v], vhi = rowptr[v + 1];
    for (int e = vlo + lane; e < vhi; e += GGAD_WAVE) {
      const int u = col[e];
      if (u >= first && u <= last) ex_hit<WS>(lst, cnt, r, u);
    }
    if (lane == 0 && v >= first && v <= last) {                         // v itself, unless it is a column of its own row
      const int p = lower_bound_i32(col, vlo, vhi, v);
      if (!(p < vhi && col[p] == v)) ex_hit<WS>(lst, cnt, r, v);
    }
  }
  __syncthreads();

  // 3. x1: NG contiguous pieces of the list (NG from F alone), fma in ascending j, then the pieces in ascending order
  const float rinv = 1.0f / sqrtf((float)r);
  int GS = 1;
  while (GS < F && GS < GGAD_WAVE) GS <<= 1;
  int NG = EX_T / GS;
  if (NG > EX_MAX_F / F) NG = EX_MAX_F / F;
  {
    const int gi = tid / GS, sl = tid - gi * GS;
    const int piece = (r + NG - 1) / NG;
    if (gi < NG) {
      const int j0 = gi * piece, j1 = min(r, j0 + piece);
      for (int f = sl; f < F; f += GS) {
        float acc = 0.0f;
        for (int j = j0; j < j1; ++j) {
          const float om = rinv / sqrtf((float)ex_cnt<WS>(cnt, j));
          acc = fmaf(om, feat[(int64_t)lst[j] * F + f], acc);
        }
        g[gi * F + f] = acc;
      }
    }
  }
  __syncthreads();
  for (int f = tid; f < F; f += EX_T) {
    float s = g[f];
    for (int gi = 1; gi < NG; ++gi) s += g[gi * F + f];
    x1[f] = s;
    nan |= s != s;
  }
  __syncthreads();

  //    a = W x1 (k_score's order), the mask, z and g
  if (tid < D) {
    const float *Wt = params + L.o_Wt();
    float a = 0.0f;
    for (int f = 0; f < F; ++f) a = fmaf(Wt[(int64_t)f * D + tid], x1[f], a);
    const float wd = params[L.o_w() + tid];
    gw[tid] = a > 0.0f ? wd : 0.0f;
    red[tid] = wd * fmaxf(a, 0.0f);
    nan |= a != a || wd != wd;
  }
  __syncthreads();
  if (tid == 0) {
    float z = 0.0f;
    for (int d = 0; d < D; ++d) z += red[d];
    zs[0] = z;
    O.logit[k] = z;
  }
  {
    const float *W = params + L.o_W();
    for (int f = tid; f < F; f += EX_T) {
      float acc = 0.0f;
      for (int d = 0; d < D; ++d) acc = fmaf(gw[d], W[(int64_t)d * F + f], acc);
      g[f] = acc;
      O.feature[(int64_t)k * F + f] = acc * x1[f];
      nan |= acc != acc;
    }
  }
  __syncthreads();

  // 4. t_j
  for (int j = tid; j < r; j += EX_T) {
    const float *row = feat + (int64_t)lst[j] * F;
    float dot = 0.0f;
    for (int f = 0; f < F; ++f) dot = fmaf(g[f], row[f], dot);
    const float om = rinv / sqrtf((float)ex_cnt<WS>(cnt, j));
    const float t = om * dot;
    tt[j] = t;
    nan |= t != t;
  }
  __syncthreads();

  // 5. the m greatest, one arg-max round each: a round takes the greatest key under the one taken before it
  unsigned long long prev = 0;
  bool more = true;
  for (int c = 0; c < m; ++c) {
    unsigned long long best = 0;                                        // (no key of an entry is 0)
    if (more)
      for (int j = tid; j < r; j += EX_T) {
        const unsigned long long key = ex_key(tt[j], j);
        if ((c == 0 || key < prev) && key > best) best = key;
      }
    best = ex_block_max(best, w4);
    more = best != 0;
    if (tid == 0) {
      const int64_t o = (int64_t)k * m + c;
      if (more) {
        const int q = (int)(~(uint32_t)best);
        O.nbr_id[o] = lst[q];
        O.nbr_contrib[o] = tt[q];
        O.nbr_colcount[o] = ex_cnt<WS>(cnt, q);
      } else {
        O.nbr_id[o] = -1;
        O.nbr_contrib[o] = 0.0f;
        O.nbr_colcount[o] = 0;
      }
    }
    prev = best;
  }
  //    rest: the entries under the last listed key
  {
    float part = 0.0f;
    if (more && r > m) {
      const int piece = (r + EX_T - 1) / EX_T;
      const int j0 = tid * piece, j1 = min(r, j0 + piece);
      for (int j = j0; j < j1; ++j) {
        const float t = tt[j];
        if (ex_key(t, j) < prev) part += t;
      }
    }
    red[tid] = part;
    __syncthreads();
    if (tid == 0) {
      float s = 0.0f;
      for (int w = 0; w < EX_T; ++w) s += red[w];
      O.rest[k] = s;
      O.closed_size[k] = r;
      atomicAdd(reinterpret_cast<unsigned long long *>(O.meta) + 1, 1ull);
      if (WS) atomicAdd(reinterpret_cast<unsigned long long *>(O.meta) + 2, 1ull);
    }
  }
  // the dump: every t_j and c_j of the row, in row order (the workspace branch computed them in place)
  if (!WS)
    for (int j = tid; j < r; j += EX_T) { dump_t[j] = tt[j]; dump_c[j] = cnt[j]; }
  if (nan) ex_status(O.meta, EX_ST_NAN);
}

__global__ void __launch_bounds__(EX_T) k_explain(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int n_nodes,
                                                  const float *__restrict__ feat, const float *__restrict__ params, ParamLayout L,
                                                  const int64_t *__restrict__ ids, int n, int batch_size,
                                                  const int32_t *__restrict__ positions, int m, int stride, int lds_rows, ExOut O,
                                                  int32_t *__restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int k = blockIdx.x, K = gridDim.x;
  const int p = positions[k];
  int64_t i64 = -1;
  if (p >= 0 && p < n) i64 = ids[p];
  if (i64 < 0 || i64 >= n_nodes) {                                      // (uniform over the workgroup)
    if (threadIdx.x == 0) ex_status(O.meta, EX_ST_POSITION);
    ex_blank(O, k, L.F, m, 0);
    return;
  }
  const int i = (int)i64, lo = rowptr[i], hi = rowptr[i + 1];
  const int self_at = lower_bound_i32(col, lo, hi, i) - lo;             // where i stands, or would stand, among its columns
  const bool has_self = lo + self_at < hi && col[lo + self_at] == i;
  const int r = hi - lo + (has_self ? 0 : 1);
  if (r > stride) {                                                     // the caller's bound on the closed rows does not hold
    if (threadIdx.x == 0) ex_status(O.meta, EX_ST_CAPACITY);
    ex_blank(O, k, L.F, m, r);
    return;
  }
  const int s0 = p - p % batch_size;
  const int s1 = (int)min((int64_t)n, (int64_t)s0 + batch_size);
  // the workspace: contributions [K][stride] | counters [K][stride] | ids [K][stride] (the last: rows of the workspace branch only)
  const int64_t base = (int64_t)k * stride, plane = (int64_t)K * stride;
  float *dump_t = reinterpret_cast<float *>(ws) + base;
  int32_t *dump_c = ws + plane + base;
  if (r <= lds_rows) {                                                  // lds_rows = min(stride, EX_LDS_ROWS): r <= stride here
    int32_t *rows = reinterpret_cast<int32_t *>(lds + EX_O_ROWS);
    ex_row<false>(rowptr, col, n_nodes, feat, params, L, ids, s0, s1, k, m, i, lo, self_at, has_self, r, lds, rows, rows + lds_rows,
                  lds + EX_O_ROWS + 2 * lds_rows, dump_c, dump_t, O);
  } else {
    ex_row<true>(rowptr, col, n_nodes, feat, params, L, ids, s0, s1, k, m, i, lo, self_at, has_self, r, lds, ws + 2 * plane + base, dump_c,
                 dump_t, dump_c, dump_t, O);
  }
}

}  // namespace

extern "C" {

int32_t ggad_explain_max_nbrs(void) { return EX_MAX_M; }
int32_t ggad_explain_lds_rows(void) { return EX_LDS_ROWS; }

int64_t ggad_explain_workspace_elems(int64_t n_rows_max_closed, int64_t K, int32_t m) {
  if (n_rows_max_closed < 1 || n_rows_max_closed > INT32_MAX || K < 0 || K > INT32_MAX || m < 1 || m > EX_MAX_M) return 0;
  return 3 * K * n_rows_max_closed;
}

int ggad_explain_f32(const int32_t *rowptr, const int32_t *col, int32_t n_nodes, const float *feat, const float *params, int32_t D,
                     int32_t F, const int64_t *ids, int64_t n, int32_t batch_size, const int32_t *positions, int32_t K, int32_t m,
                     int32_t n_rows_max_closed, float *out_logit, float *out_feature, int32_t *out_closed_size, int64_t *out_nbr_id,
                     float *out_nbr_contrib, int32_t *out_nbr_colcount, float *out_rest, int64_t *out_meta, int32_t *workspace,
                     ggad_stream_t stream) {
  if (!ggad_int_wide_ok(D, F) || m < 1 || m > EX_MAX_M) return GGAD_E_UNSUPPORTED;
  GGAD_REQUIRE(rowptr && feat && params && ids && out_meta && n_nodes >= 1 && n >= 0 && n <= INT32_MAX && batch_size >= 1 && K >= 0 &&
               n_rows_max_closed >= 1);
  GGAD_REQUIRE(K == 0 || (col && positions && out_logit && out_feature && out_closed_size && out_nbr_id && out_nbr_contrib &&
                          out_nbr_colcount && out_rest && workspace));
  static ggad_lds_optin lds;
  const int ready = ggad_lds_opt_in(lds, EX_LDS, k_explain);
  if (ready == 0) return GGAD_E_INVALID;
  if (ready != 1) { ggad_set_error(hipErrorInvalidValue, "explain: this device cannot give k_explain its LDS"); return GGAD_E_LAUNCH; }
  hipStream_t st = as_stream(stream);
  const hipError_t e = hipMemsetAsync(out_meta, 0, 4 * sizeof(int64_t), st);
  if (e != hipSuccess) { ggad_set_error(e, "explain meta"); return GGAD_E_LAUNCH; }
  if (K == 0) return GGAD_OK;
  ParamLayout L{D, F};
  ExOut O{out_logit, out_feature, out_closed_size, out_nbr_id, out_nbr_contrib, out_nbr_colcount, out_rest, out_meta};
  // the LDS of a launch holds min(n_rows_max_closed, EX_LDS_ROWS) entries: a list of short rows (the usual ranked list: the longest of
  // the top 8,192 of the DGraph-size sweep has 115) leaves room for eight workgroups per CU instead of one; no result depends on it
  const int lds_rows = n_rows_max_closed < EX_LDS_ROWS ? n_rows_max_closed : EX_LDS_ROWS;
  k_explain<<<dim3(K), dim3(EX_T), (size_t)(EX_O_ROWS + 3 * lds_rows) * 4, st>>>(rowptr, col, n_nodes, feat, params, L, ids, (int)n,
                                                                                 batch_size, positions, m, n_rows_max_closed, lds_rows, O,
                                                                                 workspace);
  GGAD_CHECK_LAUNCH("explain");
  return GGAD_OK;
}

}  // extern "C"
