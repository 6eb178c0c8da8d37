// Device path of the PC-GNN comparison model (reference src/layers.py:62-153,179-244): for ONE relation graph kept as CSR in HBM and
// one batch b_0 .. b_{B-1}
//   plan   U = union of the rows N(b_i) in ascending id order, pos[v] = index of v in U, c_v = |{u in U : v in N(u)}|  (integers only)
//   hop    A1[i] = mean_{v in N(b_i)} X[v],                         T1 = relu(A1 W)
//          A2[p] = sum_{v in N(u_p)} X[v] (1/sqrt r_u)/sqrt c_v,      T2 = relu(A2 W)      (one kernel, two weightings)
//   nb     NB[i] = mean_{u in N(b_i)} T2[pos[u]]  and its transpose  dT2[p] = sum_{i : u_p in N(b_i)} dNB[i] / |N(b_i)|
// No floating-point atomics: every sum has one owner (a wave, or the four waves of a workgroup combined in wave order), so the same
// input gives the same bits.  |U| never leaves the device: buffers have the host-known capacity `cap`, the kernels read |U| from
// memory and write the rows [|U|, cap) as zeros.  The N-sized scratch (bitmap, pos, cnt) is put back by walking the same entries.
#include "common.h"

#define PC_THREADS 256
#define PC_WAVES (PC_THREADS / GGAD_WAVE)
#define PC_SCAN_WORDS 1024      // bitmap words of one scan workgroup (4 per thread)
#define PC_SPLIT 256            // a row with more entries is gathered by the four waves of the workgroup, a quarter each
#define PC_MAX_F 64             // feature width: one wave holds a row, lane = column
#define PC_MAX_D GGAD_MAX_D
#define PC_MAX_GRID 2048

namespace {

// ------------------------------------------------------------------ plan
// bitmap bit v = 1 for every v in a batch row.  atomicOr on integers: the result does not depend on the order.
__global__ __launch_bounds__(PC_THREADS) void k_pc_mark(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        const int32_t *__restrict__ batch, uint32_t *__restrict__ bitmap) {
  const int b = batch[blockIdx.x];
  const int e1 = rowptr[b + 1];
  for (int e = rowptr[b] + threadIdx.x; e < e1; e += PC_THREADS) {
    const int v = col[e];
    atomicOr(&bitmap[v >> 5], 1u << (v & 31));
  }
}

__device__ __forceinline__ int block_sum_i(int v, int *s_part) {      // every thread gets the sum
  v = wave_sum_i(v);
  if (lane_id() == 0) s_part[threadIdx.x / GGAD_WAVE] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < PC_WAVES; ++w) t += s_part[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(PC_THREADS) void k_pc_blocksum(const uint32_t *__restrict__ bitmap, int32_t *__restrict__ bsum) {
  __shared__ int s_part[PC_WAVES];
  const uint4 w = reinterpret_cast<const uint4 *>(bitmap)[(size_t)blockIdx.x * PC_THREADS + threadIdx.x];
  const int t = block_sum_i(__popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w), s_part);
  if (threadIdx.x == 0) bsum[blockIdx.x] = t;
}

// Emits the set bits in ascending id order: unique[p] = v, pos[v] = p, row_count[p] = |N(v)|; clears the words it read.
__global__ __launch_bounds__(PC_THREADS) void k_pc_emit(uint32_t *__restrict__ bitmap, const int32_t *__restrict__ bsum,
                                                        const int32_t *__restrict__ rowptr, int cap, int32_t *__restrict__ unique,
                                                        int32_t *__restrict__ pos, int32_t *__restrict__ row_count,
                                                        int32_t *__restrict__ n_unique) {
  __shared__ int s_part[PC_WAVES];
  __shared__ int s_wave[PC_WAVES];
  int before = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += PC_THREADS) before += bsum[j];
  const int base = block_sum_i(before, s_part);
  const size_t slot = (size_t)blockIdx.x * PC_THREADS + threadIdx.x;
  const uint4 w4 = reinterpret_cast<const uint4 *>(bitmap)[slot];
  const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
  const int mine = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
  if (mine) reinterpret_cast<uint4 *>(bitmap)[slot] = make_uint4(0u, 0u, 0u, 0u);
  const int lane = lane_id(), wave = threadIdx.x / GGAD_WAVE;
  int incl = mine;                                           // inclusive scan over the wave
#pragma unroll
  for (int off = 1; off < GGAD_WAVE; off <<= 1) {
    const int up = __shfl_up(incl, off, GGAD_WAVE);
    if (lane >= off) incl += up;
  }
  if (lane == GGAD_WAVE - 1) s_wave[wave] = incl;
  __syncthreads();
  int p = base + incl - mine;
  for (int k = 0; k < wave; ++k) p += s_wave[k];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == PC_THREADS - 1) n_unique[0] = p + mine;
  for (int k = 0; k < 4; ++k) {
    uint32_t bits = w[k];
    while (bits) {
      const int v = (int)((slot * 4 + k) * 32) + (__ffs(bits) - 1);
      bits &= bits - 1;
      if (p < cap) {
        unique[p] = v;
        pos[v] = p;
        row_count[p] = rowptr[v + 1] - rowptr[v];
      }
      ++p;
    }
  }
}

// One wave per row of U: cnt[v] += 1 over its entries (RESET: cnt[v] = 0, pos[u] = -1).  The rows [|U|, cap) of unique / row_count
// get their padding values.
template <bool RESET>
__global__ __launch_bounds__(PC_THREADS) void k_pc_count(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                         int32_t *__restrict__ unique, const int32_t *__restrict__ n_unique,
                                                         int cap, int32_t *__restrict__ cnt, int32_t *__restrict__ pos,
                                                         int32_t *__restrict__ row_count) {
  const int nu = min(n_unique[0], cap), lane = lane_id();
  const int nw = gridDim.x * PC_WAVES;
  for (int p = blockIdx.x * PC_WAVES + threadIdx.x / GGAD_WAVE; p < cap; p += nw) {
    if (p < nu) {
      const int u = unique[p];
      const int e1 = rowptr[u + 1];
      for (int e = rowptr[u] + lane; e < e1; e += GGAD_WAVE) {
        if (RESET) cnt[col[e]] = 0; else atomicAdd(&cnt[col[e]], 1);
      }
      if (RESET && lane == 0) pos[u] = -1;
    } else if (!RESET && lane == 0) {
      unique[p] = -1;
      row_count[p] = 0;
    }
  }
}

// ------------------------------------------------------------------ gathers
// sum_{e in [a, b)} w_e tab[idx_e][0..W) for lanes < W.  The wave is cut into 64 / W lane groups that take every (64 / W)-th entry;
// the group sums are added in group order.
//   MODE 0: idx = col[e], w = rw.   MODE 1: idx = col[e], w = rw / sqrt(aux[col[e]]).   MODE 2: idx = aux[col[e]], w = rw.
template <int MODE>
__device__ __forceinline__ float pc_gather(const float *__restrict__ tab, int W, const int32_t *__restrict__ col,
                                           const int32_t *__restrict__ aux, int a, int b, float rw, int lane) {
  const int rpi = GGAD_WAVE / W, g = lane / W, f = lane - g * W;
  float acc = 0.f;
  if (g < rpi) {
#pragma unroll 4
    for (int e = a + g; e < b; e += rpi) {
      const int v = col[e];
      float w = rw;
      int idx = v;
      if (MODE == 1) w = rw / sqrtf((float)aux[v]);
      if (MODE == 2) idx = aux[v];
      acc = fmaf(w, tab[(size_t)idx * W + f], acc);
    }
  }
  const int src = lane < W ? lane : 0;
  float tot = 0.f;
  for (int k = 0; k < rpi; ++k) tot += __shfl(acc, k * W + src, GGAD_WAVE);
  return tot;
}

// Fused hop: A[r] = weighted sum of the feature rows of CSR row rows[r], T[r] = relu(A[r] W).  W (F x D, row-major) sits in LDS for
// the life of the workgroup, which strides over groups of four rows (one per wave; longer rows by all four waves).
// TWO = false: w = 1 / |N|  (the mean of hop 1).   TWO = true: w = (1 / sqrt |N(u)|) / sqrt c_v, rows past *n_rows are zeros.
template <bool TWO>
__global__ __launch_bounds__(PC_THREADS) void k_pc_hop(const float *__restrict__ feat, int F, const int32_t *__restrict__ rowptr,
                                                       const int32_t *__restrict__ col, const int32_t *__restrict__ rows,
                                                       const int32_t *__restrict__ n_rows, int cap, const int32_t *__restrict__ cnt,
                                                       const float *__restrict__ W, int D, float *__restrict__ A,
                                                       float *__restrict__ T) {
  __shared__ float s_w[PC_MAX_F * PC_MAX_D];
  __shared__ float s_a[PC_WAVES * PC_MAX_F];
  __shared__ float s_part[PC_WAVES * PC_MAX_F];
  __shared__ int s_e0[PC_WAVES], s_e1[PC_WAVES];
  const int tid = threadIdx.x, lane = lane_id(), wave = tid / GGAD_WAVE;
  for (int i = tid; i < F * D; i += PC_THREADS) s_w[i] = W[i];
  const int n_valid = n_rows ? min(n_rows[0], cap) : cap;
  const int n_groups = (cap + PC_WAVES - 1) / PC_WAVES;
  for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
    __syncthreads();                                         // s_w is loaded; the last group's s_a has been read
    const int row = g * PC_WAVES + wave;
    int e0 = 0, e1 = 0;
    if (row < n_valid) {
      const int u = rows[row];
      e0 = rowptr[u];
      e1 = rowptr[u + 1];
    }
    const int deg = e1 - e0;
    float tot = 0.f;
    if (deg > 0 && deg <= PC_SPLIT) {
      const float rw = TWO ? 1.0f / sqrtf((float)deg) : 1.0f / (float)deg;
      tot = pc_gather<TWO ? 1 : 0>(feat, F, col, cnt, e0, e1, rw, lane);
    }
    if (lane < F) s_a[wave * F + lane] = tot;
    if (lane == 0) {
      s_e0[wave] = e0;
      s_e1[wave] = e1;
    }
    __syncthreads();
    for (int r = 0; r < PC_WAVES; ++r) {
      const int re0 = s_e0[r], rdeg = s_e1[r] - re0;
      if (rdeg <= PC_SPLIT) continue;                        // the same for every thread of the workgroup
      const int per = (rdeg + PC_WAVES - 1) / PC_WAVES;
      const int a = re0 + wave * per, b = min(a + per, re0 + rdeg);
      const float rw = TWO ? 1.0f / sqrtf((float)rdeg) : 1.0f / (float)rdeg;
      const float part = pc_gather<TWO ? 1 : 0>(feat, F, col, cnt, a, b, rw, lane);
      if (lane < F) s_part[wave * F + lane] = part;
      __syncthreads();
      if (tid < F) s_a[r * F + tid] = ((s_part[tid] + s_part[F + tid]) + s_part[2 * F + tid]) + s_part[3 * F + tid];
      __syncthreads();
    }
    for (int i = tid; i < PC_WAVES * F; i += PC_THREADS) {
      const int r = g * PC_WAVES + i / F;
      if (r < cap) A[(size_t)r * F + (i - (i / F) * F)] = s_a[i];
    }
    if (row < cap && lane < D) {
      float z = 0.f;
      for (int f = 0; f < F; ++f) z = fmaf(s_a[wave * F + f], s_w[f * D + lane], z);
      T[(size_t)row * D + lane] = z < 0.f ? 0.f : z;
    }
  }
}

// NB[i] = sum_{u in N(b_i)} (1 / |N(b_i)|) T2[pos[u]]: one workgroup per batch row, a contiguous quarter of the row per wave.
__global__ __launch_bounds__(PC_THREADS) void k_pc_nb_fwd(const float *__restrict__ T2, int D, const int32_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ col, const int32_t *__restrict__ batch,
                                                          const int32_t *__restrict__ pos, float *__restrict__ NB) {
  __shared__ float s_part[PC_WAVES * PC_MAX_D];
  const int lane = lane_id(), wave = threadIdx.x / GGAD_WAVE;
  const int b = batch[blockIdx.x];
  const int e0 = rowptr[b], e1 = rowptr[b + 1], deg = e1 - e0;
  const int per = (deg + PC_WAVES - 1) / PC_WAVES;
  const int a = e0 + wave * per, bnd = min(a + per, e1);
  const float part = pc_gather<2>(T2, D, col, pos, a, bnd, 1.0f / (float)deg, lane);
  if (lane < D) s_part[wave * D + lane] = part;
  __syncthreads();
  const int d = threadIdx.x;
  if (d < D) NB[(size_t)blockIdx.x * D + d] = ((s_part[d] + s_part[D + d]) + s_part[2 * D + d]) + s_part[3 * D + d];
}

// dZ2[p] = [T2[p] > 0] sum_{i : u_p in N(b_i)} dNB[i] / |N(b_i)|, i ascending: one wave per row of U looks u_p up in the sorted
// batch rows (64 at a time, one per lane), then adds the rows that hold it with lane = column.  Rows past |U| are zeros.
__global__ __launch_bounds__(PC_THREADS) void k_pc_nb_bwd(const float *__restrict__ dNB, const float *__restrict__ T2, int D,
                                                          const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                          const int32_t *__restrict__ batch, int B,
                                                          const int32_t *__restrict__ unique, const int32_t *__restrict__ n_unique,
                                                          int cap, float *__restrict__ dZ2) {
  const int nu = min(n_unique[0], cap), lane = lane_id();
  const int nw = gridDim.x * PC_WAVES;
  for (int p = blockIdx.x * PC_WAVES + threadIdx.x / GGAD_WAVE; p < cap; p += nw) {
    float acc = 0.f;
    if (p < nu) {
      const int u = unique[p];
      for (int i0 = 0; i0 < B; i0 += GGAD_WAVE) {
        const int i = i0 + lane;
        bool hit = false;
        float inv = 0.f;
        if (i < B) {
          const int b = batch[i];
          const int e0 = rowptr[b], e1 = rowptr[b + 1];
          if (e1 > e0 && col[e0] <= u && col[e1 - 1] >= u) {
            const int k = lower_bound_i32(col, e0, e1, u);
            hit = k < e1 && col[k] == u;
          }
          inv = 1.0f / (float)(e1 - e0);
        }
        unsigned long long m = __ballot(hit);
        while (m) {                                          // the same for every lane
          const int j = __ffsll(m) - 1;
          m &= m - 1;
          const float w = __shfl(inv, j, GGAD_WAVE);
          if (lane < D) acc = fmaf(w, dNB[(size_t)(i0 + j) * D + lane], acc);
        }
      }
      if (lane < D && !(T2[(size_t)p * D + lane] > 0.f)) acc = 0.f;
    }
    if (lane < D) dZ2[(size_t)p * D + lane] = acc;
  }
}

inline unsigned pc_wave_grid(int rows) {
  const int blocks = (rows + PC_WAVES - 1) / PC_WAVES;
  return (unsigned)(blocks < 1 ? 1 : blocks > PC_MAX_GRID ? PC_MAX_GRID : blocks);
}
inline int64_t pc_scan_blocks(int64_t n_nodes) { return ((n_nodes + 31) / 32 + PC_SCAN_WORDS - 1) / PC_SCAN_WORDS; }

}  // namespace

extern "C" {

int32_t ggad_pcgnn_supported(int32_t feat_dim, int32_t embed_dim) {
  return feat_dim >= 1 && feat_dim <= PC_MAX_F && embed_dim >= 1 && embed_dim <= PC_MAX_D;
}
int32_t ggad_pcgnn_max_feat_dim(void) { return PC_MAX_F; }

int64_t ggad_pcgnn_scan_elems(int64_t n_nodes) {
  if (n_nodes < 1) return 0;
  const int64_t blocks = pc_scan_blocks(n_nodes);
  return blocks * PC_SCAN_WORDS + blocks;
}

int ggad_pcgnn_plan(const int32_t *rowptr, const int32_t *col, int64_t n_nodes, const int32_t *batch, int32_t n_batch, int32_t cap,
                    int32_t *scan, int32_t *pos, int32_t *cnt, int32_t *unique, int32_t *row_count, int32_t *n_unique,
                    ggad_stream_t stream) {
  GGAD_REQUIRE(rowptr && col && batch && scan && pos && cnt && unique && row_count && n_unique);
  GGAD_REQUIRE(n_nodes >= 1 && n_nodes < (1ll << 31) && n_batch >= 1 && cap >= 1 && cap <= n_nodes);
  hipStream_t st = as_stream(stream);
  const int64_t blocks = pc_scan_blocks(n_nodes);
  uint32_t *bitmap = reinterpret_cast<uint32_t *>(scan);
  int32_t *bsum = scan + blocks * PC_SCAN_WORDS;
  k_pc_mark<<<dim3((unsigned)n_batch), dim3(PC_THREADS), 0, st>>>(rowptr, col, batch, bitmap);
  k_pc_blocksum<<<dim3((unsigned)blocks), dim3(PC_THREADS), 0, st>>>(bitmap, bsum);
  k_pc_emit<<<dim3((unsigned)blocks), dim3(PC_THREADS), 0, st>>>(bitmap, bsum, rowptr, cap, unique, pos, row_count, n_unique);
  k_pc_count<false><<<dim3(pc_wave_grid(cap)), dim3(PC_THREADS), 0, st>>>(rowptr, col, unique, n_unique, cap, cnt, pos, row_count);
  GGAD_CHECK_LAUNCH("pcgnn_plan");
  return GGAD_OK;
}

int ggad_pcgnn_plan_reset(const int32_t *rowptr, const int32_t *col, int32_t *unique, const int32_t *n_unique, int32_t cap,
                          int32_t *pos, int32_t *cnt, ggad_stream_t stream) {
  GGAD_REQUIRE(rowptr && col && unique && n_unique && pos && cnt && cap >= 1);
  k_pc_count<true><<<dim3(pc_wave_grid(cap)), dim3(PC_THREADS), 0, as_stream(stream)>>>(rowptr, col, unique, n_unique, cap, cnt, pos,
                                                                                        nullptr);
  GGAD_CHECK_LAUNCH("pcgnn_plan_reset");
  return GGAD_OK;
}

int ggad_pcgnn_hop_f32(const float *feat, int32_t feat_dim, const int32_t *rowptr, const int32_t *col, const int32_t *rows,
                       const int32_t *n_rows, int32_t cap, const int32_t *cnt, const float *w, int32_t embed_dim, float *a, float *t,
                       ggad_stream_t stream) {
  GGAD_REQUIRE(feat && rowptr && col && rows && w && a && t && cap >= 1);
  if (!ggad_pcgnn_supported(feat_dim, embed_dim)) return GGAD_E_UNSUPPORTED;
  const dim3 grid(pc_wave_grid(cap)), block(PC_THREADS);
  if (cnt)
    k_pc_hop<true><<<grid, block, 0, as_stream(stream)>>>(feat, feat_dim, rowptr, col, rows, n_rows, cap, cnt, w, embed_dim, a, t);
  else
    k_pc_hop<false><<<grid, block, 0, as_stream(stream)>>>(feat, feat_dim, rowptr, col, rows, n_rows, cap, nullptr, w, embed_dim, a, t);
  GGAD_CHECK_LAUNCH("pcgnn_hop");
  return GGAD_OK;
}

int ggad_pcgnn_nb_fwd_f32(const float *t2, int32_t embed_dim, const int32_t *rowptr, const int32_t *col, const int32_t *batch,
                          int32_t n_batch, const int32_t *pos, float *nb, ggad_stream_t stream) {
  GGAD_REQUIRE(t2 && rowptr && col && batch && pos && nb && n_batch >= 1 && embed_dim >= 1 && embed_dim <= PC_MAX_D);
  k_pc_nb_fwd<<<dim3((unsigned)n_batch), dim3(PC_THREADS), 0, as_stream(stream)>>>(t2, embed_dim, rowptr, col, batch, pos, nb);
  GGAD_CHECK_LAUNCH("pcgnn_nb_fwd");
  return GGAD_OK;
}

int ggad_pcgnn_nb_bwd_f32(const float *dnb, const float *t2, int32_t embed_dim, const int32_t *rowptr, const int32_t *col,
                          const int32_t *batch, int32_t n_batch, const int32_t *unique, const int32_t *n_unique, int32_t cap,
                          float *dz2, ggad_stream_t stream) {
  GGAD_REQUIRE(dnb && t2 && rowptr && col && batch && unique && n_unique && dz2);
  GGAD_REQUIRE(n_batch >= 1 && cap >= 1 && embed_dim >= 1 && embed_dim <= PC_MAX_D);
  k_pc_nb_bwd<<<dim3(pc_wave_grid(cap)), dim3(PC_THREADS), 0, as_stream(stream)>>>(dnb, t2, embed_dim, rowptr, col, batch, n_batch,
                                                                                  unique, n_unique, cap, dz2);
  GGAD_CHECK_LAUNCH("pcgnn_nb_bwd");
  return GGAD_OK;
}

}  // extern "C"
