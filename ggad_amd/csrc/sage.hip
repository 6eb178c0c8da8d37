// Device path of the GraphSAGE comparison model (reference src/graphsage.py:19-154): one optimiser step on a batch whose neighbour
// samples were drawn on the host (sampler.cpp, ggad_mt_sample_rows) and arrive as a B x k table of node ids with row lengths.
//   fwd   combined[i] = [X[v_i] || sum_j X[nbr[i][j]] (1 / cnt_i)],  emb = relu(combined W_enc^T),  scores = emb W_cls^T,
//         and with labels  loss = mean_i CE(scores_i, y_i),  dscores = (softmax(scores) - onehot(y)) / B
//   bwd   dW_cls = dscores^T emb,  dZ = (dscores W_cls) * [emb > 0],  dW_enc = dZ^T combined
// No floating-point atomics: every sum has one owner and a fixed order (a lane over a row's sample in table order; a lane over the
// columns of `combined` in four interleaved chains; the 64 lanes of a wave in butterfly order; a thread over the rows of its row
// range, then the SG_BWD_PARTS ranges in range order), so equal inputs give equal bits.  Entries of `nbr` at or past cnt_i are never
// read.  At B ~ 200 both entry points are bound by launch and gather latency, not by bandwidth or arithmetic.
// The epoch path (ggad_sage_epoch_f32, sage_epoch.py) enqueues the steps of an epoch on one stream from a table sampled in one
// host call (sampler.cpp, ggad_sage_sched_epoch): per step k_sage_fwd, k_sage_bwd_part and k_sage_sum_adam, which adds the partial
// gradients in range order, applies Adam in place (weights, moments, step counters) and stores the step's mean loss -- one
// workgroup, the same orders of summation as k_sage_bwd_sum and k_sage_loss, so the bits equal the step path's.
#include "common.h"

#define SG_THREADS 256
#define SG_WAVES (SG_THREADS / GGAD_WAVE)
#define SG_MAX_F 64             // feature width: one wave holds a row, lane = column
#define SG_MAX_D GGAD_MAX_D     // embedding width: lane = channel
#define SG_MAX_GRID 1024
#define SG_BWD_PARTS 8          // row ranges of the backward; their partial sums are added in range order
#define SG_BWD_ROWS 32          // rows of a range staged in LDS at a time
#define SG_BWD_TILE (4 * SG_THREADS)      // entries of dW_enc per workgroup, four per thread
#define SG_SA_THREADS 1024      // the one workgroup of k_sage_sum_adam
#define SG_SA_PER ((SG_MAX_D * 2 * SG_MAX_F + 2 * SG_MAX_D + SG_SA_THREADS - 1) / SG_SA_THREADS)      // parameters per thread at most (9)

namespace {

// One wave per batch row; the workgroup keeps W_enc in LDS (transposed: s_w[c * D + d], so that lane = d reads consecutive words)
// and strides over groups of four rows.
__global__ __launch_bounds__(SG_THREADS) void k_sage_fwd(const float *__restrict__ feat, int F, const int32_t *__restrict__ nodes,
                                                         const int32_t *__restrict__ nbr, const int32_t *__restrict__ cnt, int B,
                                                         int K, const float *__restrict__ Wenc, int D,
                                                         const float *__restrict__ Wcls, const int32_t *__restrict__ labels,
                                                         float *__restrict__ combined, float *__restrict__ emb,
                                                         float *__restrict__ scores, float *__restrict__ rowloss,
                                                         float *__restrict__ dscores) {
  __shared__ float s_w[2 * SG_MAX_F * SG_MAX_D];
  __shared__ float s_c[SG_WAVES * 2 * SG_MAX_F];
  const int tid = threadIdx.x, lane = lane_id(), wave = tid / GGAD_WAVE;
  const int C2 = 2 * F;
  for (int i = tid; i < D * C2; i += SG_THREADS) {
    const int d = i / C2, c = i - d * C2;
    s_w[c * D + d] = Wenc[i];
  }
  const float wc0 = lane < D ? Wcls[lane] : 0.f, wc1 = lane < D ? Wcls[D + lane] : 0.f;
  float *sc = s_c + wave * 2 * SG_MAX_F;
  const int n_groups = (B + SG_WAVES - 1) / SG_WAVES;
  for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int row = g * SG_WAVES + wave;
    if (row < B && lane < F) {
      const int v = nodes[row];
      int n = cnt[row];
      n = n < 0 ? 0 : (n > K ? K : n);
      const float inv = 1.0f / (float)n;                       // mask.div(num_neigh)            graphsage.py:92-93
      const int32_t *__restrict__ nb = nbr + (size_t)row * K;
      const float self = feat[(size_t)v * F + lane];
      float acc = 0.f;
      int j = 0;
      for (; j + 4 <= n; j += 4) {                             // four rows in flight; added in table order
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = feat[(size_t)nb[j + u] * F + lane];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fmaf(inv, x[u], acc);
      }
      for (; j < n; ++j) acc = fmaf(inv, feat[(size_t)nb[j] * F + lane], acc);
      if (n == 0) acc = inv * 0.0f;                            // empty sample: the dense 0 / 0 mask row -> NaN, as k_seg_mean
      sc[lane] = self;
      sc[F + lane] = acc;
      combined[(size_t)row * C2 + lane] = self;
      combined[(size_t)row * C2 + F + lane] = acc;
    }
    __syncthreads();                                           // s_w is loaded, this group's s_c is written
    if (row < B) {
      float e = 0.f;
      if (lane < D) {
        const float *__restrict__ w = s_w + lane;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int c = 0;
        for (; c + 4 <= C2; c += 4) {
          a0 = fmaf(sc[c], w[c * D], a0);
          a1 = fmaf(sc[c + 1], w[(c + 1) * D], a1);
          a2 = fmaf(sc[c + 2], w[(c + 2) * D], a2);
          a3 = fmaf(sc[c + 3], w[(c + 3) * D], a3);
        }
        if (c < C2) {                                          // 2F is even: a tail of two
          a0 = fmaf(sc[c], w[c * D], a0);
          a1 = fmaf(sc[c + 1], w[(c + 1) * D], a1);
        }
        const float z = (a0 + a1) + (a2 + a3);
        e = z < 0.f ? 0.f : z;
        emb[(size_t)row * D + lane] = e;
      }
      const float s0 = wave_sum(e * wc0), s1 = wave_sum(e * wc1);
      if (lane == 0) {
        scores[2 * (size_t)row] = s0;
        scores[2 * (size_t)row + 1] = s1;
        if (labels) {
          const float m = s0 > s1 ? s0 : s1;
          const float lse = logf(expf(s0 - m) + expf(s1 - m));
          const float l0 = (s0 - m) - lse, l1 = (s1 - m) - lse;    // log softmax
          const int y = labels[row];
          rowloss[row] = -(y ? l1 : l0);
          dscores[2 * (size_t)row] = (expf(l0) - (y ? 0.f : 1.f)) / (float)B;
          dscores[2 * (size_t)row + 1] = (expf(l1) - (y ? 1.f : 0.f)) / (float)B;
        }
      }
    }
    __syncthreads();                                           // s_c has been read
  }
}

// loss[0] = (sum of the row losses) / B: lane l adds rows l, l + 64, ... in order, the lanes are added in butterfly order.
__global__ __launch_bounds__(GGAD_WAVE) void k_sage_loss(const float *__restrict__ rowloss, int B, float *__restrict__ loss) {
  float t = 0.f;
  for (int i = threadIdx.x; i < B; i += GGAD_WAVE) t += rowloss[i];
  t = wave_sum(t);
  if (threadIdx.x == 0) loss[0] = t / (float)B;
}

// Partial gradients of row range blockIdx.x: thread t of tile blockIdx.y owns the entries tile * SG_BWD_TILE + t + 256 u (u < 4) of
// dW_enc (flattened d * 2F + c); the threads t < 2 D of tile 0 own dW_cls as well.  The rows of the range pass through LDS,
// SG_BWD_ROWS at a time: dscores, combined, emb and dZ, which every workgroup computes again for its rows.
__global__ __launch_bounds__(SG_THREADS) void k_sage_bwd_part(const float *__restrict__ combined, const float *__restrict__ emb,
                                                              const float *__restrict__ dscores, const float *__restrict__ Wcls,
                                                              int B, int F, int D, float *__restrict__ ws) {
  __shared__ float s_dz[SG_BWD_ROWS * SG_MAX_D];
  __shared__ float s_em[SG_BWD_ROWS * SG_MAX_D];
  __shared__ float s_cb[SG_BWD_ROWS * 2 * SG_MAX_F];
  __shared__ float s_ds[SG_BWD_ROWS * 2];
  const int tid = threadIdx.x;
  const int C2 = 2 * F, n_out = D * C2, stride = n_out + 2 * D;
  const int per = (B + SG_BWD_PARTS - 1) / SG_BWD_PARTS;
  const int r0 = (int)blockIdx.x * per, r1 = min(B, r0 + per);
  int od[4], oc[4];
  bool ok[4];
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = (int)blockIdx.y * SG_BWD_TILE + tid + u * SG_THREADS;
    ok[u] = o < n_out;
    od[u] = ok[u] ? o / C2 : 0;
    oc[u] = ok[u] ? o - od[u] * C2 : 0;
  }
  const bool cls = blockIdx.y == 0 && tid < 2 * D;
  const int wc = cls ? tid / D : 0, wd = cls ? tid - wc * D : 0;
  float accw = 0.f;
  for (int rb = r0; rb < r1; rb += SG_BWD_ROWS) {
    const int nr = min(SG_BWD_ROWS, r1 - rb);
    __syncthreads();                                           // the last chunk has been read
    for (int i = tid; i < nr * 2; i += SG_THREADS) s_ds[i] = dscores[(size_t)rb * 2 + i];
    for (int i = tid; i < nr * C2; i += SG_THREADS) s_cb[i] = combined[(size_t)rb * C2 + i];
    for (int i = tid; i < nr * D; i += SG_THREADS) s_em[i] = emb[(size_t)rb * D + i];
    __syncthreads();
    for (int i = tid; i < nr * D; i += SG_THREADS) {
      const int r = i / D, d = i - r * D;
      const float gz = fmaf(s_ds[2 * r + 1], Wcls[D + d], s_ds[2 * r] * Wcls[d]);
      s_dz[i] = s_em[i] > 0.f ? gz : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fmaf(s_dz[r * D + od[u]], s_cb[r * C2 + oc[u]], acc[u]);
    }
    if (cls)
      for (int r = 0; r < nr; ++r) accw = fmaf(s_ds[2 * r + wc], s_em[r * D + wd], accw);
  }
  float *__restrict__ out = ws + (size_t)blockIdx.x * stride;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (ok[u]) out[(int)blockIdx.y * SG_BWD_TILE + tid + u * SG_THREADS] = acc[u];
  if (cls) out[n_out + tid] = accw;
}

// d_enc / d_cls = the SG_BWD_PARTS partial sums added in range order.
__global__ __launch_bounds__(SG_THREADS) void k_sage_bwd_sum(const float *__restrict__ ws, int n_out, int n_cls,
                                                             float *__restrict__ d_enc, float *__restrict__ d_cls) {
  const int o = blockIdx.x * SG_THREADS + threadIdx.x, stride = n_out + n_cls;
  if (o >= stride) return;
  float t = ws[o];
#pragma unroll
  for (int p = 1; p < SG_BWD_PARTS; ++p) t += ws[(size_t)p * stride + o];
  if (o < n_out) d_enc[o] = t; else d_cls[o - n_out] = t;
}

// The tail of a step in ONE workgroup (at most 64 * 128 + 128 = 8,320 parameters: up to nine per thread): thread t owns the entries
// t, t + 1024, ... of [d_enc | d_cls].  Each is the sum of its SG_BWD_PARTS partials in range order (k_sage_bwd_sum), then
// k_adam_multi's update in place (ggad_adam_elem; the bias corrections of the two tensors are formed in double by four threads of
// four waves side by side).  Wave 0 adds the row losses as k_sage_loss does.  Both step counters are read before the first barrier
// and advanced by thread 0 behind the second: no other workgroup exists that could still want the old values.
__global__ __launch_bounds__(SG_SA_THREADS) void k_sage_sum_adam(const float *__restrict__ ws, const float *__restrict__ rowloss, int B,
                                                                 int n_out, int n_cls, float *__restrict__ Wenc,
                                                                 float *__restrict__ mEnc, float *__restrict__ vEnc,
                                                                 int32_t *__restrict__ ctrEnc, float *__restrict__ Wcls,
                                                                 float *__restrict__ mCls, float *__restrict__ vCls,
                                                                 int32_t *__restrict__ ctrCls, float lr, float wd,
                                                                 float *__restrict__ loss) {
  __shared__ float sc[4];                                      // enc: lr / (1 - .9^t), sqrt(1 - .999^t); then cls
  const int tid = threadIdx.x, stride = n_out + n_cls;
  if ((tid & (GGAD_WAVE - 1)) == 0 && tid < 4 * GGAD_WAVE) {
    const int which = tid / GGAD_WAVE;
    const double t = (double)((which < 2 ? *ctrEnc : *ctrCls) + 1);
    sc[which] = (which & 1) ? (float)sqrt(1.0 - pow(0.999, t)) : (float)((double)lr / (1.0 - pow(0.9, t)));
  }
  float g[SG_SA_PER];
#pragma unroll
  for (int u = 0; u < SG_SA_PER; ++u) {                        // the gradients do not need the corrections: summed while they form
    const int o = tid + u * SG_SA_THREADS;
    float t = 0.f;
    if (o < stride) {
      t = ws[o];
#pragma unroll
      for (int p = 1; p < SG_BWD_PARTS; ++p) t += ws[(size_t)p * stride + o];
    }
    g[u] = t;
  }
  if (tid < GGAD_WAVE) {                                       // k_sage_loss: lane l adds rows l, l + 64, ...; the butterfly
    float t = 0.f;
    for (int i = tid; i < B; i += GGAD_WAVE) t += rowloss[i];
    t = wave_sum(t);
    if (tid == 0) loss[0] = t / (float)B;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < SG_SA_PER; ++u) {
    const int o = tid + u * SG_SA_THREADS;
    if (o < stride) {
      const bool enc = o < n_out;
      const int i = enc ? o : o - n_out;
      float *__restrict__ p = enc ? Wenc : Wcls, *__restrict__ m = enc ? mEnc : mCls, *__restrict__ v = enc ? vEnc : vCls;
      float pi = p[i], mi = m[i], vi = v[i];
      ggad_adam_elem(pi, mi, vi, g[u], wd, enc ? sc[0] : sc[2], enc ? sc[1] : sc[3]);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
  }
  __syncthreads();
  if (tid == 0) {
    *ctrEnc += 1;
    *ctrCls += 1;
  }
}

}  // namespace

extern "C" {

int32_t ggad_sage_supported(int32_t feat_dim, int32_t embed_dim, int32_t n_classes) {
  return feat_dim >= 1 && feat_dim <= SG_MAX_F && embed_dim >= 1 && embed_dim <= SG_MAX_D && n_classes == 2;
}
int32_t ggad_sage_bwd_parts(void) { return SG_BWD_PARTS; }
int64_t ggad_sage_bwd_workspace_elems(int32_t feat_dim, int32_t embed_dim) {
  if (!ggad_sage_supported(feat_dim, embed_dim, 2)) return 0;
  return (int64_t)SG_BWD_PARTS * ((int64_t)embed_dim * 2 * feat_dim + 2 * embed_dim);
}

int ggad_sage_fwd_f32(const float *feat, int32_t feat_dim, const int32_t *nodes, const int32_t *nbr, const int32_t *cnt,
                      int32_t n_batch, int32_t k, const float *w_enc, int32_t embed_dim, const float *w_cls, const int32_t *labels,
                      float *combined, float *emb, float *scores, float *loss, float *dscores, ggad_stream_t stream) {
  GGAD_REQUIRE(feat && nodes && nbr && cnt && w_enc && w_cls && combined && emb && scores);
  GGAD_REQUIRE(n_batch >= 1 && k >= 1 && (!labels || (loss && dscores)));
  if (!ggad_sage_supported(feat_dim, embed_dim, 2)) return GGAD_E_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const int groups = (n_batch + SG_WAVES - 1) / SG_WAVES;
  k_sage_fwd<<<dim3((unsigned)(groups > SG_MAX_GRID ? SG_MAX_GRID : groups)), dim3(SG_THREADS), 0, st>>>(
      feat, feat_dim, nodes, nbr, cnt, n_batch, k, w_enc, embed_dim, w_cls, labels, combined, emb, scores, labels ? loss + 1 : nullptr,
      dscores);
  if (labels) k_sage_loss<<<dim3(1), dim3(GGAD_WAVE), 0, st>>>(loss + 1, n_batch, loss);
  GGAD_CHECK_LAUNCH("sage_fwd");
  return GGAD_OK;
}

int ggad_sage_bwd_f32(const float *combined, const float *emb, const float *dscores, const float *w_cls, int32_t n_batch,
                      int32_t feat_dim, int32_t embed_dim, float *ws, float *d_enc, float *d_cls, ggad_stream_t stream) {
  GGAD_REQUIRE(combined && emb && dscores && w_cls && ws && d_enc && d_cls && n_batch >= 1);
  if (!ggad_sage_supported(feat_dim, embed_dim, 2)) return GGAD_E_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const int n_out = embed_dim * 2 * feat_dim, n_cls = 2 * embed_dim;
  const dim3 grid(SG_BWD_PARTS, (unsigned)((n_out + SG_BWD_TILE - 1) / SG_BWD_TILE));
  k_sage_bwd_part<<<grid, dim3(SG_THREADS), 0, st>>>(combined, emb, dscores, w_cls, n_batch, feat_dim, embed_dim, ws);
  k_sage_bwd_sum<<<dim3((unsigned)((n_out + n_cls + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, st>>>(ws, n_out, n_cls, d_enc,
                                                                                                           d_cls);
  GGAD_CHECK_LAUNCH("sage_bwd");
  return GGAD_OK;
}

int ggad_sage_sum_adam_f32(const float *ws, const float *rowloss, int32_t n_batch, int32_t feat_dim, int32_t embed_dim, float *w_enc,
                           float *m_enc, float *v_enc, int32_t *ctr_enc, float *w_cls, float *m_cls, float *v_cls, int32_t *ctr_cls,
                           float lr, float weight_decay, float *loss_out, ggad_stream_t stream) {
  GGAD_REQUIRE(ws && rowloss && w_enc && m_enc && v_enc && ctr_enc && w_cls && m_cls && v_cls && ctr_cls && loss_out && n_batch >= 1);
  if (!ggad_sage_supported(feat_dim, embed_dim, 2)) return GGAD_E_UNSUPPORTED;
  k_sage_sum_adam<<<dim3(1), dim3(SG_SA_THREADS), 0, as_stream(stream)>>>(ws, rowloss, n_batch, embed_dim * 2 * feat_dim, 2 * embed_dim,
                                                                          w_enc, m_enc, v_enc, ctr_enc, w_cls, m_cls, v_cls, ctr_cls, lr,
                                                                          weight_decay, loss_out);
  GGAD_CHECK_LAUNCH("sage_sum_adam");
  return GGAD_OK;
}

int ggad_sage_epoch_f32(const float *feat, int32_t feat_dim, const int32_t *table, int64_t stride, const int32_t *len_host,
                        int32_t n_steps, int32_t b_max, int32_t k, int32_t embed_dim, float *w_enc, float *m_enc, float *v_enc,
                        int32_t *ctr_enc, float *w_cls, float *m_cls, float *v_cls, int32_t *ctr_cls, float lr, float weight_decay,
                        float *combined, float *emb, float *scores, float *rowloss, float *dscores, float *ws, float *loss_log,
                        ggad_stream_t stream) {
  GGAD_REQUIRE(feat && table && len_host && w_enc && m_enc && v_enc && ctr_enc && w_cls && m_cls && v_cls && ctr_cls);
  GGAD_REQUIRE(combined && emb && scores && rowloss && dscores && ws && loss_log);
  GGAD_REQUIRE(n_steps >= 0 && b_max >= 1 && k >= 1 && stride >= (int64_t)b_max * (3 + (int64_t)k));
  if (!ggad_sage_supported(feat_dim, embed_dim, 2)) return GGAD_E_UNSUPPORTED;
  for (int32_t s = 0; s < n_steps; ++s) GGAD_REQUIRE(len_host[s] >= 1 && len_host[s] <= b_max);      // before the first launch
  hipStream_t st = as_stream(stream);
  const int n_out = embed_dim * 2 * feat_dim, n_cls = 2 * embed_dim;
  const dim3 bwd_grid(SG_BWD_PARTS, (unsigned)((n_out + SG_BWD_TILE - 1) / SG_BWD_TILE));
  for (int32_t s = 0; s < n_steps; ++s) {
    const int B = len_host[s];
    const int32_t *nodes = table + (int64_t)s * stride, *cnt = nodes + b_max, *labels = cnt + b_max, *nbr = labels + b_max;
    const int groups = (B + SG_WAVES - 1) / SG_WAVES;
    k_sage_fwd<<<dim3((unsigned)(groups > SG_MAX_GRID ? SG_MAX_GRID : groups)), dim3(SG_THREADS), 0, st>>>(
        feat, feat_dim, nodes, nbr, cnt, B, k, w_enc, embed_dim, w_cls, labels, combined, emb, scores, rowloss, dscores);
    k_sage_bwd_part<<<bwd_grid, dim3(SG_THREADS), 0, st>>>(combined, emb, dscores, w_cls, B, feat_dim, embed_dim, ws);
    k_sage_sum_adam<<<dim3(1), dim3(SG_SA_THREADS), 0, st>>>(ws, rowloss, B, n_out, n_cls, w_enc, m_enc, v_enc, ctr_enc, w_cls, m_cls,
                                                             v_cls, ctr_cls, lr, weight_decay, loss_log + s);
    GGAD_CHECK_LAUNCH("sage_epoch");
  }
  return GGAD_OK;
}

}  // extern "C"
