// Full-graph AnomalyDAE comparison model (reference model_AnomalyDAE.py / anomalyDAE.py): the GAT layer (GATConv of
// torch_geometric 2.1 with its defaults: one head, slope 0.2, self loops removed then one added per node, bias) forward and
// backward, and the fused structure / attribute reconstruction loss `double_recon_loss` on the rows R without the N x N matrix
// s_ = sigmoid(z z^T) (model_AnomalyDAE.py:258,283-299):
//
//   stru_i^2 = sum_j s_ij^2  +  sum_{j : A_ij != 0} (A_ij^2 - 2 A_ij s_ij)          (dense MFMA tiles + an edge pass)
//
// The dense tiles recompute x_ij = z_i . z_j on v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain, so the edge pass,
// which runs the same chain on one lane, gets the same s_ij) and never write an s or G element: the forward writes one partial
// sum per (row, column block), the backward recomputes the tile, forms G in registers, stages it in LDS and multiplies it by
// the walked rows of z on the same matrix cores, flash-attention style.  No float atomics anywhere: every sum runs in a fixed
// order and split partials are combined in index order, so a replayed hipGraph equals the eager epoch bit for bit.
#include "common.h"

#define ADAE_MAX_F 768          // output-tile budget of the backward (12 x 16 columns per wave)
#define ADAE_BWD_TILES 12
#define ADAE_COLSUM_PARTS 128
#define ADAE_FWD_COLS 256       // columns of one forward workgroup (4 waves x 64)
#define ADAE_SLOPE 0.2f

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float leaky_(float x) { return x > 0.f ? x : ADAE_SLOPE * x; }
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, GGAD_WAVE));
  return v;
}
__device__ __forceinline__ long row_of(const int64_t *__restrict__ rows, long i) { return rows ? (long)rows[i] : i; }

// ------------------------------------------------------------------------------------------------ GAT layer
// alpha_src_r = y_r . a_s, alpha_dst_r = y_r . a_d (GATConv: (x * att).sum(-1)).  One wave per node.
__global__ __launch_bounds__(256) void k_gat_alpha(const float *__restrict__ y, const float *__restrict__ a_s,
                                                   const float *__restrict__ a_d, int n, int F, float *__restrict__ als,
                                                   float *__restrict__ ald) {
  const long r = (long)blockIdx.x * 4 + threadIdx.x / GGAD_WAVE;
  if (r >= n) return;
  const int lane = lane_id();
  float s = 0.f, d = 0.f;
  for (int f = lane; f < F; f += GGAD_WAVE) {
    const float v = y[r * F + f];
    s += v * a_s[f];
    d += v * a_d[f];
  }
  s = wave_sum(s);
  d = wave_sum(d);
  if (lane == 0) {
    als[r] = s;
    ald[r] = d;
  }
}

// Edge k of target i (row i of A_hat^T, whose columns are the sources r with A_hat[r, i] != 0): k < deg walks the stored
// entries, k == deg is the one self loop GATConv adds after removing the stored ones.  Entries that are not edges of the
// reference's `adj > 0` list (a stored zero) or that are raw self loops are skipped.
__device__ __forceinline__ bool gat_edge(const int32_t *__restrict__ tcol, const float *__restrict__ tval, int beg, int deg, int i,
                                         int k, int &r) {
  if (k == deg) {
    r = i;
    return true;
  }
  r = tcol[beg + k];
  return r != i && tval[beg + k] > 0.f;
}

// z_i = sum_r p_ri y_r + b,  p_ri = softmax_r(leaky(alpha_src_r + alpha_dst_i)) over the incoming edges.  One wave per target
// row: the max and the denominator over the row's edges (lanes over edges), then the weighted sum (lanes over features).
// Saves the row max and denominator for the backward.
__global__ __launch_bounds__(256) void k_gat_fwd(const int32_t *__restrict__ tptr, const int32_t *__restrict__ tcol,
                                                 const float *__restrict__ tval, const float *__restrict__ y,
                                                 const float *__restrict__ als, const float *__restrict__ ald,
                                                 const float *__restrict__ bias, int n, int F, float *__restrict__ z,
                                                 float *__restrict__ rmax, float *__restrict__ rsum) {
  const int i = blockIdx.x * 4 + threadIdx.x / GGAD_WAVE;
  if (i >= n) return;
  const int lane = lane_id(), beg = tptr[i], deg = tptr[i + 1] - beg;
  const float di = ald[i];
  float m = -INFINITY;
  for (int k = lane; k <= deg; k += GGAD_WAVE) {
    int r;
    if (gat_edge(tcol, tval, beg, deg, i, k, r)) m = fmaxf(m, leaky_(als[r] + di));
  }
  m = wave_max(m);
  float l = 0.f;
  for (int k = lane; k <= deg; k += GGAD_WAVE) {
    int r;
    if (gat_edge(tcol, tval, beg, deg, i, k, r)) l += expf(leaky_(als[r] + di) - m);
  }
  l = wave_sum(l);
  const float inv = 1.f / (l + 1e-16f);
  for (int f0 = 0; f0 < F; f0 += GGAD_WAVE) {
    const int f = f0 + lane;
    float acc = 0.f;
    for (int k = 0; k <= deg; ++k) {
      int r;
      if (!gat_edge(tcol, tval, beg, deg, i, k, r)) continue;
      const float p = expf(leaky_(als[r] + di) - m) * inv;
      if (f < F) acc += p * y[(long)r * F + f];
    }
    if (f < F) z[(long)i * F + f] = acc + (bias ? bias[f] : 0.f);
  }
  if (lane == 0) {
    rmax[i] = m;
    rsum[i] = l;
  }
}

// Backward, target side.  Slot of edge k of target i: tptr[i] + i + k (one extra slot per row: the added self loop).
//   q_ri = g_i . y_r,  dpre_ri = p_ri (q_ri - sum_r' p_r'i q_r'i) * leaky'(pre_ri),  dalpha_dst_i = sum_r dpre_ri
__global__ __launch_bounds__(256) void k_gat_bwd_tgt(const int32_t *__restrict__ tptr, const int32_t *__restrict__ tcol,
                                                     const float *__restrict__ tval, const float *__restrict__ y,
                                                     const float *__restrict__ als, const float *__restrict__ ald,
                                                     const float *__restrict__ rmax, const float *__restrict__ rsum,
                                                     const float *__restrict__ g, int n, int F, float *__restrict__ dpre,
                                                     float *__restrict__ dald) {
  const int i = blockIdx.x * 4 + threadIdx.x / GGAD_WAVE;
  if (i >= n) return;
  const int lane = lane_id(), beg = tptr[i], deg = tptr[i + 1] - beg;
  const long slot0 = (long)beg + i;
  const float di = ald[i], m = rmax[i], inv = 1.f / (rsum[i] + 1e-16f);
  const float *gi = g + (long)i * F;
  float S = 0.f;
  for (int k = lane; k <= deg; k += GGAD_WAVE) {        // each lane re-reads only the slots it wrote itself
    int r;
    float q = 0.f;
    if (gat_edge(tcol, tval, beg, deg, i, k, r)) {
      const float *yr = y + (long)r * F;
      for (int f = 0; f < F; ++f) q += gi[f] * yr[f];
      S += expf(leaky_(als[r] + di) - m) * inv * q;
    }
    dpre[slot0 + k] = q;
  }
  S = wave_sum(S);
  float D = 0.f;
  for (int k = lane; k <= deg; k += GGAD_WAVE) {
    int r;
    float v = 0.f;
    if (gat_edge(tcol, tval, beg, deg, i, k, r)) {
      const float pre = als[r] + di;
      const float p = expf(leaky_(pre) - m) * inv;
      v = p * (dpre[slot0 + k] - S) * (pre > 0.f ? 1.f : ADAE_SLOPE);
    }
    dpre[slot0 + k] = v;
    D += v;
  }
  D = wave_sum(D);
  if (lane == 0) dald[i] = D;
}

// Backward, source side: walk row r of A_hat (targets i with A_hat[r, i] != 0) plus the self loop; tmap[e] = position of entry
// e of A_hat in A_hat^T, so the slot of edge (r -> i) is tmap[e] + i.
//   dalpha_src_r = sum_i dpre_ri,  dy_r = sum_i p_ri g_i + dalpha_src_r a_s + dalpha_dst_r a_d
__global__ __launch_bounds__(256) void k_gat_bwd_src(const int32_t *__restrict__ aptr, const int32_t *__restrict__ acol,
                                                     const float *__restrict__ aval, const int32_t *__restrict__ tmap,
                                                     const int32_t *__restrict__ tptr, const float *__restrict__ als,
                                                     const float *__restrict__ ald, const float *__restrict__ rmax,
                                                     const float *__restrict__ rsum, const float *__restrict__ a_s,
                                                     const float *__restrict__ a_d, const float *__restrict__ g,
                                                     const float *__restrict__ dpre, const float *__restrict__ dald, int n, int F,
                                                     float *__restrict__ dals, float *__restrict__ dy) {
  const int r = blockIdx.x * 4 + threadIdx.x / GGAD_WAVE;
  if (r >= n) return;
  const int lane = lane_id(), beg = aptr[r], deg = aptr[r + 1] - beg;
  float S = 0.f;
  for (int k = lane; k <= deg; k += GGAD_WAVE) {
    int i;
    if (!gat_edge(acol, aval, beg, deg, r, k, i)) continue;
    S += dpre[k == deg ? (long)tptr[r + 1] + r : (long)tmap[beg + k] + i];
  }
  S = wave_sum(S);
  const float sr = als[r], dr = dald[r];
  for (int f0 = 0; f0 < F; f0 += GGAD_WAVE) {
    const int f = f0 + lane;
    float acc = 0.f;
    for (int k = 0; k <= deg; ++k) {
      int i;
      if (!gat_edge(acol, aval, beg, deg, r, k, i)) continue;
      const float p = expf(leaky_(sr + ald[i]) - rmax[i]) * (1.f / (rsum[i] + 1e-16f));
      if (f < F) acc += p * g[(long)i * F + f];
    }
    if (f < F) dy[(long)r * F + f] = acc + S * a_s[f] + dr * a_d[f];
  }
  if (lane == 0) dals[r] = S;
}

// out[f] = sum_r w_r M[r, f] (w = NULL: 1): fixed row ranges per part, parts combined in order.
__global__ __launch_bounds__(64) void k_colsum_part(const float *__restrict__ M, const float *__restrict__ w, long n, int F,
                                                    float *__restrict__ ws) {
  const int f = blockIdx.x * 64 + threadIdx.x, p = blockIdx.y;
  if (f >= F) return;
  const long lo = n * p / ADAE_COLSUM_PARTS, hi = n * (p + 1) / ADAE_COLSUM_PARTS;
  float acc = 0.f;
  for (long r = lo; r < hi; ++r) acc += (w ? w[r] : 1.f) * M[r * F + f];
  ws[(long)p * F + f] = acc;
}
__global__ __launch_bounds__(256) void k_colsum_fin(const float *__restrict__ ws, int F, float *__restrict__ out) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  float acc = 0.f;
  for (int p = 0; p < ADAE_COLSUM_PARTS; ++p) acc += ws[(long)p * F + f];
  out[f] = acc;
}

// ------------------------------------------------------------------------------------------------ structure loss
// One 16 x 16 tile of x = Z_a Z_b^T on the matrix cores.  Lane l supplies A[l & 15][k] = z[ra][k] and B[k][l & 15] = z[rb][k],
// k = k0 + l / 16, zero past F (K padded to a multiple of 4); the result register j holds row 4 (l / 16) + j, column l & 15.
__device__ __forceinline__ f32x4 gram_tile(const float *__restrict__ z, int F, long ra, bool va, long rb, bool vb) {
  const int kq = lane_id() >> 4;
  const float *za = z + ra * F, *zb = z + rb * F;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < F; k0 += 4) {
    const int k = k0 + kq;
    const float a = (va && k < F) ? za[k] : 0.f;
    const float b = (vb && k < F) ? zb[k] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// Forward dense part: part[i * n_cb + cb] = sum_{j in column block cb, j < N} s_ij^2 for the rows i of the list.  Workgroup =
// 16 rows x 256 columns, wave w the columns 64 w .. 64 w + 63 as four 16-column tiles.
__global__ __launch_bounds__(256) void k_stru_fwd_dense(const float *__restrict__ z, int n, int F, const int64_t *__restrict__ rows,
                                                        int n_rows, int n_cb, float *__restrict__ part) {
  __shared__ float s_part[4][16];
  const int wave = threadIdx.x / GGAD_WAVE, lane = lane_id();
  const int rb = blockIdx.y, cb = blockIdx.x;
  const int il = rb * 16 + (lane & 15);
  const bool va = il < n_rows;
  const long ra = va ? row_of(rows, il) : 0;
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const long j = (long)cb * ADAE_FWD_COLS + wave * 64 + t * 16 + (lane & 15);
    const bool vb = j < n;
    const f32x4 x = gram_tile(z, F, ra, va, vb ? j : 0, vb);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float s = sigmoidf_(x[q]);
      rs[q] += vb ? s * s : 0.f;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v = rs[q];
    for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, GGAD_WAVE);      // the 16 columns of a row
    if ((lane & 15) == 0) s_part[wave][(lane >> 4) * 4 + q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int row = rb * 16 + threadIdx.x;
    if (row < n_rows)
      part[(long)row * n_cb + cb] = ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
  }
}

// Forward edge pass, one wave per listed row i (compact CSR of A_hat[rows, :]): the correction sum_e (A^2 - 2 A s) with s_ij from
// the same k-ordered fmaf chain as the tiles (one lane per edge), the dense partials, the attribute error ||X_i - X^_i||, and
//   stru_i = sqrt(dense + correction), score_i = 0.5 attr_i + 0.5 stru_i.  s_edge (may be NULL) keeps s per edge for the backward.
__global__ __launch_bounds__(256) void k_stru_fwd_rows(const float *__restrict__ z, int F, const int64_t *__restrict__ rows, int n_rows,
                                                       const int32_t *__restrict__ rptr, const int32_t *__restrict__ rcol,
                                                       const float *__restrict__ rval, const float *__restrict__ part, int n_cb,
                                                       const float *__restrict__ x, const float *__restrict__ xhat,
                                                       float *__restrict__ s_edge, float *__restrict__ attr,
                                                       float *__restrict__ stru, float *__restrict__ score) {
  const int il = blockIdx.x * 4 + threadIdx.x / GGAD_WAVE;
  if (il >= n_rows) return;
  const int lane = lane_id();
  const long i = row_of(rows, il);
  const float *zi = z + i * F;
  float corr = 0.f;
  for (int e = rptr[il] + lane; e < rptr[il + 1]; e += GGAD_WAVE) {
    const float *zj = z + (long)rcol[e] * F;
    float acc = 0.f;
    for (int k = 0; k < F; ++k) acc = fmaf(zi[k], zj[k], acc);
    const float s = sigmoidf_(acc), a = rval[e];
    corr += a * a - 2.f * a * s;
    if (s_edge) s_edge[e] = s;
  }
  corr = wave_sum(corr);
  float dense = 0.f;
  for (int c = lane; c < n_cb; c += GGAD_WAVE) dense += part[(long)il * n_cb + c];
  dense = wave_sum(dense);
  float ae = 0.f;
  for (int f = lane; f < F; f += GGAD_WAVE) {
    const float d = x[i * F + f] - xhat[i * F + f];
    ae += d * d;
  }
  ae = sqrtf(wave_sum(ae));
  if (lane == 0) {
    const float se = sqrtf(fmaxf(dense + corr, 0.f));
    attr[il] = ae;
    stru[il] = se;
    score[il] = 0.5f * ae + 0.5f * se;
  }
}

__global__ __launch_bounds__(1024) void k_mean(const float *__restrict__ v, long n, float *__restrict__ out) {
  __shared__ float part[16];
  const long per = (n + 1023) / 1024;
  const long lo = (long)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  float s = 0.f;
  for (long i = lo; i < hi; ++i) s += v[i];
  s = wave_sum(s);
  if (lane_id() == 0) part[threadIdx.x / GGAD_WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int w = 0; w < 16; ++w) acc += part[w];
    out[0] = acc / (float)n;
  }
}

// c_i = g 0.5 / (|R| stru_i): d loss / d s_ij = c_i (s_ij - A_ij).
__global__ __launch_bounds__(256) void k_stru_coef(const float *__restrict__ stru, int n_rows, const float *__restrict__ gloss,
                                                   float *__restrict__ c) {
  const int il = blockIdx.x * 256 + threadIdx.x;
  if (il < n_rows) c[il] = gloss[0] * (0.5f / (float)n_rows) / stru[il];
}

// Backward dense part, one recompute pass: for the owner rows o (a list, or all N) and the walked rows w (all N, or a list) in
// this split's range of 64-row blocks,  part[split][o][:] = sum_w G_ow z_w,  G_ow = c s^2 (1 - s),  s = sigmoid(z_o . z_w),
// c = c[o] (owners are the loss rows) or c[w] (walked rows are).  Workgroup = 16 owners: per block of 64 walked rows each wave
// forms a 16 x 16 G tile, the 16 x 64 tile goes through LDS, and each wave multiplies it into its output columns (16-column
// tiles w, w + 4, ... of F), K = 64 on the matrix cores.
__global__ __launch_bounds__(256) void k_stru_bwd_dense(const float *__restrict__ z, int F, const int64_t *__restrict__ own,
                                                        int n_own, const int64_t *__restrict__ walk, int n_walk,
                                                        const float *__restrict__ c, int c_of_walk, int n_split,
                                                        float *__restrict__ part) {
  __shared__ float sG[16][64 + 4];
  const int wave = threadIdx.x / GGAD_WAVE, lane = lane_id(), kq = lane >> 4, col = lane & 15;
  const int ob = blockIdx.x, split = blockIdx.y;
  const int n_wb = (n_walk + 63) / 64;
  const int wb0 = (int)((long)n_wb * split / n_split), wb1 = (int)((long)n_wb * (split + 1) / n_split);
  const int ol = ob * 16 + col;
  const bool vo = ol < n_own;
  const long ro = vo ? row_of(own, ol) : 0;
  const int n_ft = (F + 15) / 16;
  f32x4 O[ADAE_BWD_TILES];
#pragma unroll
  for (int t = 0; t < ADAE_BWD_TILES; ++t) O[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int wb = wb0; wb < wb1; ++wb) {
    {
      const int wl = wb * 64 + wave * 16 + col;
      const bool vw = wl < n_walk;
      const f32x4 x = gram_tile(z, F, ro, vo, vw ? row_of(walk, wl) : 0, vw);
      // register q: owner row 4 kq + q, walked column wave * 16 + col
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int orow = ob * 16 + kq * 4 + q;
        float gq = 0.f;
        if (vw && orow < n_own) {
          const float s = sigmoidf_(x[q]);
          gq = (c_of_walk ? c[wl] : c[orow]) * (s * s * (1.f - s));
        }
        sG[kq * 4 + q][wave * 16 + col] = gq;
      }
    }
    __syncthreads();
    for (int kk = 0; kk < 64; kk += 4) {
      const int wl = wb * 64 + kk + kq;
      const bool vw = wl < n_walk;
      const float *zw = z + (vw ? row_of(walk, wl) : 0) * F;
      const float a = sG[col][kk + kq];
#pragma unroll
      for (int t = 0; t < ADAE_BWD_TILES; ++t) {
        const int ft = t * 4 + wave;
        if (ft < n_ft) {
          const int f = ft * 16 + col;
          const float b = (vw && f < F) ? zw[f] : 0.f;
          O[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, O[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < ADAE_BWD_TILES; ++t) {
    const int ft = t * 4 + wave;
    const int f = ft * 16 + col;
    if (ft >= n_ft || f >= F) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int orow = ob * 16 + kq * 4 + q;
      if (orow < n_own) part[((long)split * n_own + orow) * F + f] = O[t][q];
    }
  }
}

// dZ_j = sum_s colpart[s][j] + sum_{i in R, A_ij != 0} dG_ij z_i  (+ for j = R[il]: sum_s rowpart[s][il] + sum_e dG_je z_col(e)),
// dG = -c_i A_ij s_ij (1 - s_ij).  One wave per node, fixed order.  tptr / trow / tedge: the entries of A_hat[R, :] grouped by
// column (row position in R, edge index), pos[j] = position of j in R or -1.
__global__ __launch_bounds__(256) void k_stru_bwd_combine(const float *__restrict__ z, int n, int F, const int64_t *__restrict__ rows,
                                                          int n_rows, const int32_t *__restrict__ rptr, const int32_t *__restrict__ rcol,
                                                          const float *__restrict__ rval, const float *__restrict__ s_edge,
                                                          const int32_t *__restrict__ pos, const int32_t *__restrict__ tptr,
                                                          const int32_t *__restrict__ trow, const int32_t *__restrict__ tedge,
                                                          const float *__restrict__ c, const float *__restrict__ rowpart, int s_row,
                                                          const float *__restrict__ colpart, int s_col, float *__restrict__ dz) {
  const int j = blockIdx.x * 4 + threadIdx.x / GGAD_WAVE;
  if (j >= n) return;
  const int lane = lane_id(), il = pos[j];
  for (int f0 = 0; f0 < F; f0 += GGAD_WAVE) {
    const int f = f0 + lane;
    const bool vf = f < F;
    float d = 0.f;
    for (int s = 0; s < s_col; ++s) d += vf ? colpart[((long)s * n + j) * F + f] : 0.f;
    for (int e = tptr[j]; e < tptr[j + 1]; ++e) {
      const int ir = trow[e], ed = tedge[e];
      const float s = s_edge[ed];
      const float gq = -c[ir] * rval[ed] * (s * (1.f - s));
      if (vf) d += gq * z[row_of(rows, ir) * F + f];
    }
    if (il >= 0) {
      for (int s = 0; s < s_row; ++s) d += vf ? rowpart[((long)s * n_rows + il) * F + f] : 0.f;
      for (int e = rptr[il]; e < rptr[il + 1]; ++e) {
        const float s = s_edge[e];
        const float gq = -c[il] * rval[e] * (s * (1.f - s));
        if (vf) d += gq * z[(long)rcol[e] * F + f];
      }
    }
    if (vf) dz[(long)j * F + f] = d;
  }
}

// d loss / d X^_i = g (0.5 / |R|) (X^_i - X_i) / attr_i on the listed rows (the other rows of dxhat are left as they are).
__global__ __launch_bounds__(256) void k_attr_bwd(const float *__restrict__ x, const float *__restrict__ xhat, const int64_t *__restrict__ rows,
                                                  int n_rows, int F, const float *__restrict__ attr, const float *__restrict__ gloss,
                                                  float *__restrict__ dxhat) {
  const int il = blockIdx.x * 4 + threadIdx.x / GGAD_WAVE;
  if (il >= n_rows) return;
  const long i = row_of(rows, il);
  const float sc = gloss[0] * (0.5f / (float)n_rows) / attr[il];
  for (int f = lane_id(); f < F; f += GGAD_WAVE) dxhat[i * F + f] = sc * (xhat[i * F + f] - x[i * F + f]);
}

// ------------------------------------------------------------------------------------------------ host side
static int stru_cb(int64_t n) { return (int)((n + ADAE_FWD_COLS - 1) / ADAE_FWD_COLS); }

// column splits of the backward recompute passes: enough workgroups to cover the CUs twice at least
static int bwd_split(int64_t n_own, int64_t n_walk) {
  const int64_t blocks = (n_own + 15) / 16, wb = (n_walk + 63) / 64;
  int64_t s = (1024 + blocks - 1) / blocks;
  if (s > wb) s = wb;
  if (s < 1) s = 1;
  return (int)s;
}

extern "C" {

int ggad_adae_gat_alpha_f32(const float *y, const float *a_s, const float *a_d, int32_t n, int32_t F, float *als, float *ald,
                            ggad_stream_t stream) {
  GGAD_REQUIRE(y && a_s && a_d && als && ald && n >= 1 && F >= 1);
  k_gat_alpha<<<dim3((n + 3) / 4), dim3(256), 0, as_stream(stream)>>>(y, a_s, a_d, n, F, als, ald);
  GGAD_CHECK_LAUNCH("adae_gat_alpha");
  return GGAD_OK;
}

int ggad_adae_gat_fwd_f32(const int32_t *tptr, const int32_t *tcol, const float *tval, const float *y, const float *als,
                          const float *ald, const float *bias, int32_t n, int32_t F, float *z, float *rmax, float *rsum,
                          ggad_stream_t stream) {
  GGAD_REQUIRE(tptr && tcol && tval && y && als && ald && z && rmax && rsum && n >= 1 && F >= 1);
  k_gat_fwd<<<dim3((n + 3) / 4), dim3(256), 0, as_stream(stream)>>>(tptr, tcol, tval, y, als, ald, bias, n, F, z, rmax, rsum);
  GGAD_CHECK_LAUNCH("adae_gat_fwd");
  return GGAD_OK;
}

int ggad_adae_gat_bwd_f32(const int32_t *tptr, const int32_t *tcol, const float *tval, const int32_t *aptr, const int32_t *acol,
                          const float *aval, const int32_t *tmap, const float *y, const float *als, const float *ald,
                          const float *rmax, const float *rsum, const float *a_s, const float *a_d, const float *g, int32_t n,
                          int32_t F, float *dpre, float *dals, float *dald, float *dy, ggad_stream_t stream) {
  GGAD_REQUIRE(tptr && tcol && tval && aptr && acol && aval && tmap && y && als && ald && rmax && rsum && a_s && a_d && g && dpre &&
               dals && dald && dy && n >= 1 && F >= 1);
  k_gat_bwd_tgt<<<dim3((n + 3) / 4), dim3(256), 0, as_stream(stream)>>>(tptr, tcol, tval, y, als, ald, rmax, rsum, g, n, F, dpre,
                                                                        dald);
  GGAD_CHECK_LAUNCH("adae_gat_bwd_tgt");
  k_gat_bwd_src<<<dim3((n + 3) / 4), dim3(256), 0, as_stream(stream)>>>(aptr, acol, aval, tmap, tptr, als, ald, rmax, rsum, a_s,
                                                                        a_d, g, dpre, dald, n, F, dals, dy);
  GGAD_CHECK_LAUNCH("adae_gat_bwd_src");
  return GGAD_OK;
}

int64_t ggad_adae_colsum_workspace_elems(int32_t F) { return (int64_t)ADAE_COLSUM_PARTS * (F > 0 ? F : 0); }

int ggad_adae_colsum_f32(const float *M, const float *w, int64_t n, int32_t F, float *out, float *ws, ggad_stream_t stream) {
  GGAD_REQUIRE(M && out && ws && n >= 0 && F >= 1);
  k_colsum_part<<<dim3((F + 63) / 64, ADAE_COLSUM_PARTS), dim3(64), 0, as_stream(stream)>>>(M, w, (long)n, F, ws);
  GGAD_CHECK_LAUNCH("adae_colsum_part");
  k_colsum_fin<<<dim3((F + 255) / 256), dim3(256), 0, as_stream(stream)>>>(ws, F, out);
  GGAD_CHECK_LAUNCH("adae_colsum_fin");
  return GGAD_OK;
}

int64_t ggad_adae_stru_fwd_workspace_elems(int32_t n_rows, int32_t n) { return (int64_t)n_rows * stru_cb(n); }

int ggad_adae_stru_fwd_f32(const float *z, int32_t n, int32_t F, const int64_t *rows, int32_t n_rows, const int32_t *rptr,
                           const int32_t *rcol, const float *rval, const float *x, const float *xhat, float *ws, float *s_edge,
                           float *attr, float *stru, float *score, float *loss, ggad_stream_t stream) {
  GGAD_REQUIRE(z && rows && rptr && rcol && rval && x && xhat && ws && attr && stru && score && n >= 1 && F >= 1 && n_rows >= 1 &&
               n_rows <= n);
  const int n_cb = stru_cb(n);
  k_stru_fwd_dense<<<dim3(n_cb, (n_rows + 15) / 16), dim3(256), 0, as_stream(stream)>>>(z, n, F, rows, n_rows, n_cb, ws);
  GGAD_CHECK_LAUNCH("adae_stru_fwd_dense");
  k_stru_fwd_rows<<<dim3((n_rows + 3) / 4), dim3(256), 0, as_stream(stream)>>>(z, F, rows, n_rows, rptr, rcol, rval, ws, n_cb, x,
                                                                               xhat, s_edge, attr, stru, score);
  GGAD_CHECK_LAUNCH("adae_stru_fwd_rows");
  if (loss) {
    k_mean<<<dim3(1), dim3(1024), 0, as_stream(stream)>>>(score, (long)n_rows, loss);
    GGAD_CHECK_LAUNCH("adae_mean");
  }
  return GGAD_OK;
}

int64_t ggad_adae_stru_bwd_workspace_elems(int32_t n_rows, int32_t n, int32_t F) {
  if (n_rows < 1 || n < 1 || F < 1) return 0;
  return (int64_t)bwd_split(n_rows, n) * n_rows * F + (int64_t)bwd_split(n, n_rows) * n * F + n_rows;
}

int ggad_adae_stru_bwd_f32(const float *z, int32_t n, int32_t F, const int64_t *rows, int32_t n_rows, const int32_t *rptr,
                           const int32_t *rcol, const float *rval, const float *s_edge, const int32_t *pos, const int32_t *tptr,
                           const int32_t *trow, const int32_t *tedge, const float *stru, const float *gloss, float *ws, float *dz,
                           ggad_stream_t stream) {
  GGAD_REQUIRE(z && rows && rptr && rcol && rval && s_edge && pos && tptr && trow && tedge && stru && gloss && ws && dz && n >= 1 &&
               F >= 1 && F <= ADAE_MAX_F && n_rows >= 1 && n_rows <= n);
  const int s_row = bwd_split(n_rows, n), s_col = bwd_split(n, n_rows);
  float *rowpart = ws, *colpart = ws + (int64_t)s_row * n_rows * F, *c = colpart + (int64_t)s_col * n * F;
  k_stru_coef<<<dim3((n_rows + 255) / 256), dim3(256), 0, as_stream(stream)>>>(stru, n_rows, gloss, c);
  GGAD_CHECK_LAUNCH("adae_stru_coef");
  k_stru_bwd_dense<<<dim3((n_rows + 15) / 16, s_row), dim3(256), 0, as_stream(stream)>>>(z, F, rows, n_rows, nullptr, n, c, 0, s_row,
                                                                                         rowpart);
  GGAD_CHECK_LAUNCH("adae_stru_bwd_rows");
  k_stru_bwd_dense<<<dim3((n + 15) / 16, s_col), dim3(256), 0, as_stream(stream)>>>(z, F, nullptr, n, rows, n_rows, c, 1, s_col,
                                                                                    colpart);
  GGAD_CHECK_LAUNCH("adae_stru_bwd_cols");
  k_stru_bwd_combine<<<dim3((n + 3) / 4), dim3(256), 0, as_stream(stream)>>>(z, n, F, rows, n_rows, rptr, rcol, rval, s_edge, pos,
                                                                             tptr, trow, tedge, c, rowpart, s_row, colpart, s_col,
                                                                             dz);
  GGAD_CHECK_LAUNCH("adae_stru_bwd_combine");
  return GGAD_OK;
}

int ggad_adae_attr_bwd_f32(const float *x, const float *xhat, const int64_t *rows, int32_t n_rows, int32_t F, const float *attr,
                           const float *gloss, float *dxhat, ggad_stream_t stream) {
  GGAD_REQUIRE(x && xhat && rows && attr && gloss && dxhat && n_rows >= 1 && F >= 1);
  k_attr_bwd<<<dim3((n_rows + 3) / 4), dim3(256), 0, as_stream(stream)>>>(x, xhat, rows, n_rows, F, attr, gloss, dxhat);
  GGAD_CHECK_LAUNCH("adae_attr_bwd");
  return GGAD_OK;
}

}  // extern "C"
