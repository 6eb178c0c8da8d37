// Head and loss of the PC-GNN comparison model behind its relation kernels (pcgnn.hip): what InterAgg.forward does after the three
// relations and what PCALayer.loss does with it (reference src/layers.py:125-153, src/model.py:25-48), forward and backward.
//   fwd   combined = relu([T1_0 T1_1 T1_2] W),  neigh = relu([NB_0 NB_1 NB_2] W),  cn / nn = rows over their norm (0 / 0 -> 0),
//         affinity_i = <cn_i, nn_i>,  scores = combined W_cls^T,  row loss = CE(scores_i, y_i),  dscores = (softmax - onehot) / B
//   rows  a0 / a1 = mean affinity of the label-0 / label-1 rows,  constraint = max(0, 1 - (a0 - a1)),  total = mean CE + 5 constraint;
//         dZc, dZn (through the cross entropy, the hinge, both normalisations and both ReLUs),  dT1_r = dZc W_r^T,  dNB_r = dZn W_r^T
//   dW    dW = [T1]^T dZc + [NB]^T dZn,  dW_cls = dscores^T combined
// No floating-point atomics and no workgroup waits on another: a0 and a1 need every row, so the forward ends at a launch boundary
// and every workgroup of the row kernel adds the B affinities again in the same order (lane l of one wave over rows l, l + 64, ...,
// then the butterfly).  Every other sum has one owner and a fixed order as well (a lane over the 3D inputs in two interleaved
// chains; a thread over the rows of its range, then the PH_PARTS ranges in range order), so equal inputs give equal bits.
// W (3D x D, at most 48 KiB) is staged in LDS with an odd row stride: the forward reads it with lane = column, the backward with
// lane = row, and both are free of bank conflicts.  At B ~ 200 every launch is bound by launch and load latency.
#include "common.h"

#define PH_THREADS 256
#define PH_WAVES (PH_THREADS / GGAD_WAVE)
#define PH_MAX_D GGAD_MAX_D
#define PH_MAX_GRID 1024
#define PH_PARTS 8              // row ranges of the weight gradient; their partial sums are added in range order
#define PH_ROWS 16              // rows of a range staged in LDS at a time
#define PH_TILE (4 * PH_THREADS)          // entries of dW per workgroup, four per thread

namespace {

struct ph_in { const float *t1[3]; const float *nb[3]; };
struct ph_out { float *t1[3]; float *nb[3]; };

__device__ __forceinline__ int ph_stride(int D) { return D | 1; }

// W (3D x D, row-major) into s_w with rows ph_stride(D) apart.
__device__ __forceinline__ void ph_stage_w(const float *__restrict__ W, int D, float *__restrict__ s_w) {
  const int ws = ph_stride(D), n = 3 * D * D;
  for (int i = threadIdx.x; i < n; i += PH_THREADS) {
    const int k = i / D, j = i - k * D;
    s_w[k * ws + j] = W[i];
  }
}

// One wave per batch row, lane = output channel; the workgroup strides over groups of four rows.  combined == nullptr: forward only,
// scores and affinity are the only stores.
__global__ __launch_bounds__(PH_THREADS) void k_ph_fwd(ph_in in, const float *__restrict__ W, const float *__restrict__ Wcls,
                                                       const int64_t *__restrict__ labels, int B, int D, float *__restrict__ scores,
                                                       float *__restrict__ affinity, float *__restrict__ combined,
                                                       float *__restrict__ neigh, float *__restrict__ rowloss,
                                                       float *__restrict__ dscores) {
  __shared__ float s_w[3 * PH_MAX_D * (PH_MAX_D + 1)];
  __shared__ float s_x[PH_WAVES * 6 * PH_MAX_D];
  const int tid = threadIdx.x, lane = lane_id(), wave = tid / GGAD_WAVE;
  const int C3 = 3 * D, ws = ph_stride(D);
  ph_stage_w(W, D, s_w);
  const float wc0 = lane < D ? Wcls[lane] : 0.f, wc1 = lane < D ? Wcls[D + lane] : 0.f;
  float *sx = s_x + wave * 6 * PH_MAX_D;
  const int n_groups = (B + PH_WAVES - 1) / PH_WAVES;
  for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int row = g * PH_WAVES + wave;
    if (row < B && lane < D) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        sx[r * D + lane] = in.t1[r][(size_t)row * D + lane];
        sx[C3 + r * D + lane] = in.nb[r][(size_t)row * D + lane];
      }
    }
    __syncthreads();                                           // s_w is loaded, this group's s_x is written
    if (row < B) {
      float c = 0.f, m = 0.f;
      if (lane < D) {
        const float *__restrict__ w = s_w + lane;
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
        int k = 0;
        for (; k + 2 <= C3; k += 2) {
          const float w0 = w[k * ws], w1 = w[(k + 1) * ws];
          a0 = fmaf(sx[k], w0, a0);
          a1 = fmaf(sx[k + 1], w1, a1);
          b0 = fmaf(sx[C3 + k], w0, b0);
          b1 = fmaf(sx[C3 + k + 1], w1, b1);
        }
        if (k < C3) {
          a0 = fmaf(sx[k], w[k * ws], a0);
          b0 = fmaf(sx[C3 + k], w[k * ws], b0);
        }
        const float zc = a0 + a1, zn = b0 + b1;
        c = zc < 0.f ? 0.f : zc;
        m = zn < 0.f ? 0.f : zn;
      }
      const float nc = sqrtf(wave_sum(c * c)), nq = sqrtf(wave_sum(m * m));
      float cn = c / nc, mn = m / nq;                          // 0 / 0 = NaN -> 0, as the reference replaces it   layers.py:139-145
      cn = cn != cn ? 0.f : cn;
      mn = mn != mn ? 0.f : mn;
      const float aff = wave_sum(cn * mn);
      const float s0 = wave_sum(c * wc0), s1 = wave_sum(c * wc1);
      if (lane == 0) {
        scores[2 * (size_t)row] = s0;
        scores[2 * (size_t)row + 1] = s1;
        affinity[row] = aff;
      }
      if (combined) {
        if (lane < D) {
          combined[(size_t)row * D + lane] = c;
          neigh[(size_t)row * D + lane] = m;
        }
        if (lane == 0) {
          const float mx = s0 > s1 ? s0 : s1;
          const float lse = logf(expf(s0 - mx) + expf(s1 - mx));
          const float l0 = (s0 - mx) - lse, l1 = (s1 - mx) - lse;  // log softmax
          const bool y = labels[row] != 0;
          rowloss[row] = -(y ? l1 : l0);
          dscores[2 * (size_t)row] = (expf(l0) - (y ? 0.f : 1.f)) / (float)B;
          dscores[2 * (size_t)row + 1] = (expf(l1) - (y ? 1.f : 0.f)) / (float)B;
        }
      }
    }
    __syncthreads();                                           // s_x has been read
  }
}

// The loss pair and the row gradients.  Wave 0 of EVERY workgroup adds the row losses and the two classes' affinities in the same
// order; workgroup 0 stores (total, constraint).  A class without a row makes its mean 0 / 0: total and constraint are NaN and the
// hinge passes no gradient (NaN >= 0 is false), as torch's clamp_min does.  A row whose combined or neigh has norm 0 gets no
// gradient from the affinity on either side: the reference's replacement selects 0 there and its ReLU backward selects 0 again.
__global__ __launch_bounds__(PH_THREADS) void k_ph_bwd_rows(const float *__restrict__ W, const float *__restrict__ Wcls,
                                                            const int64_t *__restrict__ labels, int B, int D,
                                                            const float *__restrict__ affinity, const float *__restrict__ combined,
                                                            const float *__restrict__ neigh, const float *__restrict__ rowloss,
                                                            const float *__restrict__ dscores, float *__restrict__ dzc,
                                                            float *__restrict__ dzn, ph_out out, float *__restrict__ loss) {
  __shared__ float s_w[3 * PH_MAX_D * (PH_MAX_D + 1)];
  __shared__ float s_dz[PH_WAVES * 2 * PH_MAX_D];
  __shared__ float s_g[2];
  const int tid = threadIdx.x, lane = lane_id(), wave = tid / GGAD_WAVE;
  const int ws = ph_stride(D);
  ph_stage_w(W, D, s_w);
  if (wave == 0) {
    int n0 = 0, n1 = 0;
    float t0 = 0.f, t1 = 0.f, tl = 0.f;
    for (int i = lane; i < B; i += GGAD_WAVE) {
      const int64_t y = labels[i];
      const float a = affinity[i];
      if (y == 0) { ++n0; t0 += a; }
      if (y == 1) { ++n1; t1 += a; }
      tl += rowloss[i];
    }
    n0 = wave_sum_i(n0);
    n1 = wave_sum_i(n1);
    t0 = wave_sum(t0);
    t1 = wave_sum(t1);
    tl = wave_sum(tl);
    if (lane == 0) {
      const float a0 = t0 / (float)n0, a1 = t1 / (float)n1;
      const float diff = 1.0f - (a0 - a1);
      const float con = diff < 0.f ? 0.f : diff;               // clamp_min: NaN stays NaN                    model.py:36-41
      const bool pass = diff >= 0.f;
      s_g[0] = pass ? -5.0f / (float)n0 : 0.f;
      s_g[1] = pass ? 5.0f / (float)n1 : 0.f;
      if (blockIdx.x == 0) {
        loss[0] = tl / (float)B + 5.0f * con;
        loss[1] = con;
      }
    }
  }
  const float wc0 = lane < D ? Wcls[lane] : 0.f, wc1 = lane < D ? Wcls[D + lane] : 0.f;
  float *sd = s_dz + wave * 2 * PH_MAX_D;
  const int n_groups = (B + PH_WAVES - 1) / PH_WAVES;
  for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int row = g * PH_WAVES + wave;
    __syncthreads();                                           // s_w and s_g are written, the last group's s_dz has been read
    if (row < B) {
      const float c = lane < D ? combined[(size_t)row * D + lane] : 0.f;
      const float m = lane < D ? neigh[(size_t)row * D + lane] : 0.f;
      const int64_t y = labels[row];
      const float ga = y == 0 ? s_g[0] : (y == 1 ? s_g[1] : 0.f);
      const float nc = sqrtf(wave_sum(c * c)), nq = sqrtf(wave_sum(m * m));
      float dc = fmaf(dscores[2 * (size_t)row + 1], wc1, dscores[2 * (size_t)row] * wc0);
      float dm = 0.f;
      if (nc > 0.f && nq > 0.f) {
        // d affinity / d c = (nn - affinity cn) / |c|: what autograd's x / n and norm nodes add up to, with one rounding where
        // the two parts cancel
        const float cn = c / nc, mn = m / nq, aff = affinity[row];
        dc += (ga / nc) * fmaf(-aff, cn, mn);
        dm = (ga / nq) * fmaf(-aff, mn, cn);
      }
      dc = c > 0.f ? dc : 0.f;
      dm = m > 0.f ? dm : 0.f;
      if (lane < D) {
        dzc[(size_t)row * D + lane] = dc;
        dzn[(size_t)row * D + lane] = dm;
        sd[lane] = dc;
        sd[PH_MAX_D + lane] = dm;
      }
    }
    __syncthreads();                                           // this group's s_dz is written
    if (row < B && lane < D) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float *__restrict__ w = s_w + (r * D + lane) * ws;
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
        int j = 0;
        for (; j + 2 <= D; j += 2) {
          const float w0 = w[j], w1 = w[j + 1];
          a0 = fmaf(sd[j], w0, a0);
          a1 = fmaf(sd[j + 1], w1, a1);
          b0 = fmaf(sd[PH_MAX_D + j], w0, b0);
          b1 = fmaf(sd[PH_MAX_D + j + 1], w1, b1);
        }
        if (j < D) {
          a0 = fmaf(sd[j], w[j], a0);
          b0 = fmaf(sd[PH_MAX_D + j], w[j], b0);
        }
        out.t1[r][(size_t)row * D + lane] = a0 + a1;
        out.nb[r][(size_t)row * D + lane] = b0 + b1;
      }
    }
  }
}

// Partial weight gradients of row range blockIdx.x: thread t of tile blockIdx.y owns the entries tile * PH_TILE + t + 256 u (u < 4)
// of dW (flattened k * D + j); the threads t < 2 D of tile 0 own dW_cls as well.  The rows of the range pass through LDS, PH_ROWS
// at a time.
__global__ __launch_bounds__(PH_THREADS) void k_ph_dw_part(ph_in in, const float *__restrict__ combined,
                                                           const float *__restrict__ dscores, const float *__restrict__ dzc,
                                                           const float *__restrict__ dzn, int B, int D, float *__restrict__ part) {
  __shared__ float s_t[PH_ROWS * 3 * PH_MAX_D];
  __shared__ float s_n[PH_ROWS * 3 * PH_MAX_D];
  __shared__ float s_zc[PH_ROWS * PH_MAX_D];
  __shared__ float s_zn[PH_ROWS * PH_MAX_D];
  __shared__ float s_cb[PH_ROWS * PH_MAX_D];
  __shared__ float s_ds[PH_ROWS * 2];
  const int tid = threadIdx.x;
  const int C3 = 3 * D, n_out = C3 * D, stride = n_out + 2 * D;
  const int per = (B + PH_PARTS - 1) / PH_PARTS;
  const long long r0l = (long long)blockIdx.x * per;
  const int r0 = r0l < B ? (int)r0l : B, r1 = (long long)r0 + per < B ? r0 + per : B;
  int orow[4], ocol[4];
  bool ok[4];
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = (int)blockIdx.y * PH_TILE + tid + u * PH_THREADS;
    ok[u] = o < n_out;
    orow[u] = ok[u] ? o / D : 0;
    ocol[u] = ok[u] ? o - orow[u] * D : 0;
  }
  const bool cls = blockIdx.y == 0 && tid < 2 * D;
  const int wc = cls ? tid / D : 0, wd = cls ? tid - wc * D : 0;
  float accw = 0.f;
  for (int rb = r0; rb < r1; rb += PH_ROWS) {
    const int nr = min(PH_ROWS, r1 - rb);
    __syncthreads();                                           // the last chunk has been read
    for (int i = tid; i < nr * C3; i += PH_THREADS) {
      const int r = i / C3, k = i - r * C3, rel = k / D, kk = k - rel * D;
      s_t[i] = in.t1[rel][(size_t)(rb + r) * D + kk];
      s_n[i] = in.nb[rel][(size_t)(rb + r) * D + kk];
    }
    for (int i = tid; i < nr * D; i += PH_THREADS) {
      s_zc[i] = dzc[(size_t)rb * D + i];
      s_zn[i] = dzn[(size_t)rb * D + i];
      s_cb[i] = combined[(size_t)rb * D + i];
    }
    for (int i = tid; i < nr * 2; i += PH_THREADS) s_ds[i] = dscores[(size_t)rb * 2 + i];
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = fmaf(s_t[r * C3 + orow[u]], s_zc[r * D + ocol[u]], acc[u]);
        acc[u] = fmaf(s_n[r * C3 + orow[u]], s_zn[r * D + ocol[u]], acc[u]);
      }
    }
    if (cls)
      for (int r = 0; r < nr; ++r) accw = fmaf(s_ds[2 * r + wc], s_cb[r * D + wd], accw);
  }
  float *__restrict__ o = part + (size_t)blockIdx.x * stride;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (ok[u]) o[(int)blockIdx.y * PH_TILE + tid + u * PH_THREADS] = acc[u];
  if (cls) o[n_out + tid] = accw;
}

// dW / dW_cls = the PH_PARTS partial sums added in range order.
__global__ __launch_bounds__(PH_THREADS) void k_ph_dw_sum(const float *__restrict__ part, int n_out, int n_cls, float *__restrict__ d_w,
                                                          float *__restrict__ d_cls) {
  const int o = blockIdx.x * PH_THREADS + threadIdx.x, stride = n_out + n_cls;
  if (o >= stride) return;
  float t = part[o];
#pragma unroll
  for (int p = 1; p < PH_PARTS; ++p) t += part[(size_t)p * stride + o];
  if (o < n_out) d_w[o] = t; else d_cls[o - n_out] = t;
}

}  // namespace

extern "C" {

int32_t ggad_pcgnn_head_supported(int32_t n_batch, int32_t embed_dim) {
  return n_batch >= 1 && embed_dim >= 1 && embed_dim <= PH_MAX_D;
}
int32_t ggad_pcgnn_head_parts(void) { return PH_PARTS; }
int64_t ggad_pcgnn_head_workspace_elems(int32_t n_batch, int32_t embed_dim) {
  if (!ggad_pcgnn_head_supported(n_batch, embed_dim)) return 0;
  const int64_t b = n_batch, d = embed_dim;
  return 4 * b * d + 3 * b + (int64_t)PH_PARTS * (3 * d * d + 2 * d);
}

int ggad_pcgnn_head_f32(const float *t1_0, const float *t1_1, const float *t1_2, const float *nb_0, const float *nb_1, const float *nb_2,
                        const float *w, const float *w_cls, const int64_t *labels, int32_t n_batch, int32_t embed_dim, float *scores,
                        float *affinity, float *loss, float *d_t1_0, float *d_t1_1, float *d_t1_2, float *d_nb_0, float *d_nb_1,
                        float *d_nb_2, float *d_w, float *d_cls, float *ws, ggad_stream_t stream) {
  GGAD_REQUIRE(t1_0 && t1_1 && t1_2 && nb_0 && nb_1 && nb_2 && w && w_cls && scores && affinity);
  GGAD_REQUIRE(!loss || (labels && d_t1_0 && d_t1_1 && d_t1_2 && d_nb_0 && d_nb_1 && d_nb_2 && d_w && d_cls && ws));
  if (!ggad_pcgnn_head_supported(n_batch, embed_dim)) return GGAD_E_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const int64_t b = n_batch, d = embed_dim;
  const int n_out = 3 * embed_dim * embed_dim, n_cls = 2 * embed_dim;
  float *combined = nullptr, *neigh = nullptr, *dzc = nullptr, *dzn = nullptr, *rowloss = nullptr, *dscores = nullptr, *part = nullptr;
  if (loss) {
    combined = ws;
    neigh = combined + b * d;
    dzc = neigh + b * d;
    dzn = dzc + b * d;
    rowloss = dzn + b * d;
    dscores = rowloss + b;
    part = dscores + 2 * b;
  }
  const ph_in in = {{t1_0, t1_1, t1_2}, {nb_0, nb_1, nb_2}};
  const int groups = (n_batch + PH_WAVES - 1) / PH_WAVES;
  const dim3 rows_grid((unsigned)(groups > PH_MAX_GRID ? PH_MAX_GRID : groups));
  k_ph_fwd<<<rows_grid, dim3(PH_THREADS), 0, st>>>(in, w, w_cls, labels, n_batch, embed_dim, scores, affinity, combined, neigh, rowloss,
                                                   dscores);
  if (loss) {
    const ph_out out = {{d_t1_0, d_t1_1, d_t1_2}, {d_nb_0, d_nb_1, d_nb_2}};
    k_ph_bwd_rows<<<rows_grid, dim3(PH_THREADS), 0, st>>>(w, w_cls, labels, n_batch, embed_dim, affinity, combined, neigh, rowloss,
                                                          dscores, dzc, dzn, out, loss);
    const dim3 grid(PH_PARTS, (unsigned)((n_out + PH_TILE - 1) / PH_TILE));
    k_ph_dw_part<<<grid, dim3(PH_THREADS), 0, st>>>(in, combined, dscores, dzc, dzn, n_batch, embed_dim, part);
    k_ph_dw_sum<<<dim3((unsigned)((n_out + n_cls + PH_THREADS - 1) / PH_THREADS)), dim3(PH_THREADS), 0, st>>>(part, n_out, n_cls, d_w,
                                                                                                          d_cls);
  }
  GGAD_CHECK_LAUNCH("pcgnn_head");
  return GGAD_OK;
}

}  // extern "C"
