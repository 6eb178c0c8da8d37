// Full-graph AEGIS comparison model (reference model_AEGIS.py / aegis.py): the batch-norm heads of its two MLPs and its two losses.
//
// Both MLPs of the model are torch_geometric.nn.MLP stacks  Linear -> BatchNorm1d (training mode) -> act -> Linear  over all N (or
// 2N) rows.  The Linear layers run on ggad_gemm_f32; this file holds what sits between them:
//
//   ggad_aegis_bn_fwd_f32   column statistics over one or two row blocks (the statistics of their concatenation: cat(z, z_gen) is
//                           never built), the running-stat update, then y = act(BN(h)) written out, or -- the head of
//                           discriminator2 -- p = sigmoid(act(BN(h)) . w2 + b2) per row without writing y.
//   ggad_aegis_bn_bwd_f32   the backward of the same op (one row block): column sums of du and du * x_hat (and, with the head,
//                           of dl * y and dl), then dh, dgamma, dbeta (dw2, db2).
//   ggad_aegis_loss_fwd_f32 loss_g = BCE(p, 0) with torch's log clamp at -100 and loss_ae = mean_{i in rows} ||x_i - zd_i||.
//   ggad_aegis_loss_bwd_f32 their gradients (dp on every row; dzd on every row, zero off the list and past F).
//
// Each call is two launches at most.  Statistics and sums are per-workgroup partials over a fixed contiguous row range, merged by
// the LAST workgroup to finish (ticket word, agent-scope release before the ticket, acquire after it) in partial order: no float
// atomics, no workgroup waits on another, so a replayed hipGraph equals an eager epoch bit for bit.  Variance partials are
// (count, mean, M2) merged with Chan's formula, not sums of squares.
#include "common.h"
#include "handoff.h"

#define BN_C 64            // channels the kernels take (hid_dim of both MLPs, model_AEGIS.py:163)
#define BN_ROWS 256        // rows per statistics workgroup before the grid saturates
#define BN_MAX_G 256       // statistics / sums workgroups at most
#define LOSS_ROWS 64       // rows per loss workgroup before the grid saturates (one wave walks ~16 rows)
#define LOSS_MAX_G 256

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// (n, mean, M2) <- (n, mean, M2) merged with (nb, mb, M2b): Chan et al.; an empty side leaves the other unchanged
__device__ __forceinline__ void chan_merge(float &n, float &mean, float &m2, float nb, float mb, float m2b) {
  if (nb == 0.f) return;
  if (n == 0.f) {
    n = nb; mean = mb; m2 = m2b;
    return;
  }
  const float nt = n + nb, d = mb - mean;
  mean = mean + d * (nb / nt);
  m2 = m2 + m2b + d * d * (n * (nb / nt));
  n = nt;
}

__device__ __forceinline__ const float *bn_row(const float *h1, int64_t m1, int64_t ld1, const float *h2, int64_t ld2, int64_t r) {
  return r < m1 ? h1 + r * ld1 : h2 + (r - m1) * ld2;
}

__device__ __forceinline__ float act_f(float u, int act) { return act == 0 ? fmaxf(u, 0.f) : sigmoidf_(u); }
// d act / d u from the activation's output y (torch: relu -> grad where y > 0, sigmoid -> grad (1 - y) y)
__device__ __forceinline__ float act_d(float y, int act) { return act == 0 ? (y > 0.f ? 1.f : 0.f) : (1.f - y) * y; }

// Lane layout of the row kernels (C = 64): lane l covers columns 4 (l & 15) .. + 3 of one row, the four 16-lane quarters of a wave
// take four rows, so a workgroup of 4 waves walks 16 rows at a time (slot s = 4 wave + quarter).

// ------------------------------------------------------------------------------------------------ forward statistics
// Workgroup b owns rows [M b / G, M (b + 1) / G) of the concatenation; slot s takes rows lo + s, lo + s + 16, ...  Per column a
// running (count, mean, M2) per slot (Welford), the 16 slots merged in slot order, the workgroup's partial stored; the last
// workgroup merges the G partials in order (four quarters of the partial list, then the quarters in order), writes mean and
// 1 / sqrt(var + eps) and updates the running statistics (unbiased variance) and num_batches_tracked.
__global__ __launch_bounds__(256) void k_bn_stats(const float *__restrict__ h1, int64_t m1, int64_t ld1, const float *__restrict__ h2,
                                                  int64_t ld2, int64_t M, float eps, float momentum, float *__restrict__ run_mean,
                                                  float *__restrict__ run_var, int64_t *__restrict__ n_batches,
                                                  float *__restrict__ mean_out, float *__restrict__ invstd_out, float *__restrict__ ws,
                                                  int32_t *__restrict__ ticket) {
  __shared__ float s_mean[16][BN_C], s_m2[16][BN_C];
  __shared__ float s_n[16];
  __shared__ int flag;
  const int t = threadIdx.x, lane = t & 63, slot = (t >> 6) * 4 + (lane >> 4), c0 = (lane & 15) * 4;
  const int G = gridDim.x, b = blockIdx.x;
  const int64_t lo = M * b / G, hi = M * (b + 1) / G;
  float n = 0.f, mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = lo + slot; r < hi; r += 16) {
    const float4 v = *reinterpret_cast<const float4 *>(bn_row(h1, m1, ld1, h2, ld2, r) + c0);
    const float x[4] = {v.x, v.y, v.z, v.w};
    n += 1.f;
    const float inv_n = 1.f / n;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = x[k] - mean[k];
      mean[k] += d * inv_n;
      m2[k] += d * (x[k] - mean[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    s_mean[slot][c0 + k] = mean[k];
    s_m2[slot][c0 + k] = m2[k];
  }
  if ((lane & 15) == 0) s_n[slot] = n;
  __syncthreads();
  float *part = ws + (int64_t)b * (1 + 2 * BN_C);
  if (t < BN_C) {
    float pn = 0.f, pm = 0.f, pq = 0.f;
    for (int s = 0; s < 16; ++s) chan_merge(pn, pm, pq, s_n[s], s_mean[s][t], s_m2[s][t]);
    part[1 + t] = pm;
    part[1 + BN_C + t] = pq;
    if (t == 0) part[0] = pn;
  }
  if (!ggad_last_of(ticket, (int)gridDim.x, &flag)) return;
  // t = quarter * 64 + column: quarter q merges partials [G q / 4, G (q + 1) / 4)
  const int q = t >> 6, c = t & 63;
  {
    float pn = 0.f, pm = 0.f, pq = 0.f;
    for (int p = G * q / 4; p < G * (q + 1) / 4; ++p) {
      const float *pp = ws + (int64_t)p * (1 + 2 * BN_C);
      // the count is the same in every lane: an atomic load keeps it a vector load behind the acquire (a scalar-cache load of
      // bytes another workgroup handed off can be stale)
      const float cnt = __hip_atomic_load(pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      chan_merge(pn, pm, pq, cnt, pp[1 + c], pp[1 + BN_C + c]);
    }
    s_mean[q][c] = pm;
    s_m2[q][c] = pq;
    if (c == 0) s_n[q] = pn;
  }
  __syncthreads();
  if (t < BN_C) {
    float pn = 0.f, pm = 0.f, pq = 0.f;
    for (int k = 0; k < 4; ++k) chan_merge(pn, pm, pq, s_n[k], s_mean[k][t], s_m2[k][t]);
    const float var = pq / (float)M;                       // biased: what normalises
    mean_out[t] = pm;
    invstd_out[t] = 1.f / sqrtf(var + eps);
    if (run_mean) run_mean[t] = momentum * pm + (1.f - momentum) * run_mean[t];
    if (run_var) run_var[t] = momentum * (pq / (float)(M - 1)) + (1.f - momentum) * run_var[t];
    if (t == 0 && n_batches) n_batches[0] += 1;
  }
}

// ------------------------------------------------------------------------------------------------ forward apply
// Output row k = rows[k] of the concatenation (rows NULL: k).  y = act(gamma (h - mean) invstd + beta) written to y (row stride
// ldy), or with w2: p[k] = sigmoid(y . w2 + b2), the dot reduced over the row's 16 lanes in a fixed butterfly.
__global__ __launch_bounds__(256) void k_bn_apply(const float *__restrict__ h1, int64_t m1, int64_t ld1, const float *__restrict__ h2,
                                                  int64_t ld2, const int64_t *__restrict__ rows, int64_t n_out, const float *__restrict__ gamma,
                                                  const float *__restrict__ beta, const float *__restrict__ mean,
                                                  const float *__restrict__ invstd, int act, float *__restrict__ y, int64_t ldy,
                                                  const float *__restrict__ w2, const float *__restrict__ b2, float *__restrict__ p) {
  const int t = threadIdx.x, lane = t & 63, c0 = (lane & 15) * 4;
  const int64_t k = (int64_t)blockIdx.x * 16 + (t >> 6) * 4 + (lane >> 4);
  const bool live = k < n_out;
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const int64_t r = rows ? rows[k] : k;
    const float4 v = *reinterpret_cast<const float4 *>(bn_row(h1, m1, ld1, h2, ld2, r) + c0);
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = act_f((x[j] - mean[c0 + j]) * invstd[c0 + j] * gamma[c0 + j] + beta[c0 + j], act);
  }
  if (!w2) {
    if (live) *reinterpret_cast<float4 *>(y + k * ldy + c0) = make_float4(out[0], out[1], out[2], out[3]);
    return;
  }
  float d = 0.f;
  if (live) d = ((out[0] * w2[c0] + out[1] * w2[c0 + 1]) + out[2] * w2[c0 + 2]) + out[3] * w2[c0 + 3];
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) d += __shfl_xor(d, off, GGAD_WAVE);      // within the row's 16 lanes
  if (live && (lane & 15) == 0) p[k] = sigmoidf_(d + b2[0]);
}

// ------------------------------------------------------------------------------------------------ backward
// du of one row: dy (or, with the head, dl w2 with dl = dp p (1 - p)) times act'; x_hat and y recomputed from h and the saved
// statistics.
struct BnRow {
  float xh[4], y[4], du[4], dl;
};
__device__ __forceinline__ BnRow bn_bwd_row(const float *__restrict__ h, int64_t ldh, int64_t r, int c0, const float *__restrict__ gamma,
                                            const float *__restrict__ beta, const float *__restrict__ mean,
                                            const float *__restrict__ invstd, int act, const float *__restrict__ dy, int64_t lddy,
                                            const float *__restrict__ w2, const float *__restrict__ p, const float *__restrict__ dp) {
  BnRow o;
  const float4 v = *reinterpret_cast<const float4 *>(h + r * ldh + c0);
  const float x[4] = {v.x, v.y, v.z, v.w};
  float g[4];
  if (w2) {
    const float pr = p[r];
    o.dl = dp[r] * (1.f - pr) * pr;                       // torch sigmoid backward: grad (1 - p) p
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = o.dl * w2[c0 + j];
  } else {
    o.dl = 0.f;
    const float4 gv = *reinterpret_cast<const float4 *>(dy + r * lddy + c0);
    g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o.xh[j] = (x[j] - mean[c0 + j]) * invstd[c0 + j];
    o.y[j] = act_f(o.xh[j] * gamma[c0 + j] + beta[c0 + j], act);
    o.du[j] = g[j] * act_d(o.y[j], act);
  }
  return o;
}

// Column sums over the rows of workgroup b (same partition as the statistics): sdu, sdux = sum du x_hat and, with the head,
// sdly = sum dl y and sdl = sum dl.  The last workgroup adds the partials in order and writes dbeta = sdu, dgamma = sdux, dw2, db2.
__global__ __launch_bounds__(256) void k_bn_bwd_sums(const float *__restrict__ h, int64_t M, int64_t ldh, const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, const float *__restrict__ mean,
                                                     const float *__restrict__ invstd, int act, const float *__restrict__ dy,
                                                     int64_t lddy, const float *__restrict__ w2, const float *__restrict__ p,
                                                     const float *__restrict__ dp, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                     float *__restrict__ dw2, float *__restrict__ db2, float *__restrict__ ws,
                                                     int32_t *__restrict__ ticket) {
  __shared__ float s_acc[3][16][BN_C];
  __shared__ float s_dl[16];
  __shared__ int flag;
  constexpr int W = 3 * BN_C + 1;                         // partial row: sdu | sdux | sdly | sdl
  const int t = threadIdx.x, lane = t & 63, slot = (t >> 6) * 4 + (lane >> 4), c0 = (lane & 15) * 4;
  const int G = gridDim.x, b = blockIdx.x;
  const int64_t lo = M * b / G, hi = M * (b + 1) / G;
  float sdu[4] = {0.f, 0.f, 0.f, 0.f}, sdux[4] = {0.f, 0.f, 0.f, 0.f}, sdly[4] = {0.f, 0.f, 0.f, 0.f}, sdl = 0.f;
  for (int64_t r = lo + slot; r < hi; r += 16) {
    const BnRow o = bn_bwd_row(h, ldh, r, c0, gamma, beta, mean, invstd, act, dy, lddy, w2, p, dp);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sdu[j] += o.du[j];
      sdux[j] += o.du[j] * o.xh[j];
      sdly[j] += o.dl * o.y[j];
    }
    sdl += o.dl;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s_acc[0][slot][c0 + j] = sdu[j];
    s_acc[1][slot][c0 + j] = sdux[j];
    s_acc[2][slot][c0 + j] = sdly[j];
  }
  if ((lane & 15) == 0) s_dl[slot] = sdl;
  __syncthreads();
  float *part = ws + (int64_t)b * W;
  if (t < 3 * BN_C) {
    const int a = t / BN_C, c = t - a * BN_C;
    float acc = 0.f;
    for (int s = 0; s < 16; ++s) acc += s_acc[a][s][c];
    part[t] = acc;
  } else if (t == 3 * BN_C) {
    float acc = 0.f;
    for (int s = 0; s < 16; ++s) acc += s_dl[s];
    part[t] = acc;
  }
  if (!ggad_last_of(ticket, (int)gridDim.x, &flag)) return;
  if (t < W) {
    float acc = 0.f;
    for (int q = 0; q < G; ++q) acc += ws[(int64_t)q * W + t];
    if (t < BN_C) dbeta[t] = acc;
    else if (t < 2 * BN_C) dgamma[t - BN_C] = acc;
    else if (t < 3 * BN_C) { if (w2) dw2[t - 2 * BN_C] = acc; }
    else if (w2) db2[0] = acc;
  }
}

// dh = (du - sdu / M - x_hat sdux / M) invstd gamma   (torch's batch_norm backward in training mode, rearranged)
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const float *__restrict__ h, int64_t M, int64_t ldh, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, const float *__restrict__ mean,
                                                      const float *__restrict__ invstd, int act, const float *__restrict__ dy,
                                                      int64_t lddy, const float *__restrict__ w2, const float *__restrict__ p,
                                                      const float *__restrict__ dp, const float *__restrict__ sdux,
                                                      const float *__restrict__ sdu, float *__restrict__ dh, int64_t lddh) {
  const int t = threadIdx.x, lane = t & 63, c0 = (lane & 15) * 4;
  const int64_t r = (int64_t)blockIdx.x * 16 + (t >> 6) * 4 + (lane >> 4);
  if (r >= M) return;
  const BnRow o = bn_bwd_row(h, ldh, r, c0, gamma, beta, mean, invstd, act, dy, lddy, w2, p, dp);
  const float inv_m = 1.f / (float)M;
  float d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + j;
    d[j] = (o.du[j] - sdu[c] * inv_m - o.xh[j] * (sdux[c] * inv_m)) * (invstd[c] * gamma[c]);
  }
  *reinterpret_cast<float4 *>(dh + r * lddh + c0) = make_float4(d[0], d[1], d[2], d[3]);
}

// ------------------------------------------------------------------------------------------------ losses
// Workgroup b: list positions [nr b / G, nr (b + 1) / G) (one wave per row, lanes over F: attr = ||x_i - zd_i||, summed per wave in
// row order, the four waves in order) and p indices [n b / G, n (b + 1) / G) (BCE terms -max(log1p(-p), -100), thread-strided, then
// the wave butterfly and the waves in order).  The last workgroup adds the G partials (lane-strided, then the butterfly) and
// divides.
__global__ __launch_bounds__(256) void k_loss_fwd(const float *__restrict__ p, int64_t n, const float *__restrict__ x, int F,
                                                  const float *__restrict__ zd, int64_t ldz, const int64_t *__restrict__ rows, int64_t nr,
                                                  float *__restrict__ attr, float *__restrict__ loss_g, float *__restrict__ loss_ae,
                                                  float *__restrict__ ws, int32_t *__restrict__ ticket) {
  __shared__ float s_ae[4], s_g[4];
  __shared__ int flag;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int G = gridDim.x, b = blockIdx.x;
  float ae = 0.f;
  if (nr > 0) {
    const int64_t lo = nr * b / G, hi = nr * (b + 1) / G;
    for (int64_t k = lo + w; k < hi; k += 4) {
      const int64_t i = rows[k];
      const float *xi = x + i * F, *zi = zd + i * ldz;
      float s = 0.f;
      for (int f = lane; f < F; f += GGAD_WAVE) {
        const float d = xi[f] - zi[f];
        s += d * d;
      }
      s = sqrtf(wave_sum(s));
      if (lane == 0) attr[k] = s;
      ae += s;
    }
  }
  float g = 0.f;
  if (n > 0) {
    const int64_t lo = n * b / G, hi = n * (b + 1) / G;
    for (int64_t i = lo + t; i < hi; i += 256) g += -fmaxf(log1pf(-p[i]), -100.f);
  }
  g = wave_sum(g);
  if (lane == 0) {
    s_ae[w] = ae;
    s_g[w] = g;
  }
  __syncthreads();
  if (t == 0) {
    ws[2 * b] = ((s_ae[0] + s_ae[1]) + s_ae[2]) + s_ae[3];
    ws[2 * b + 1] = ((s_g[0] + s_g[1]) + s_g[2]) + s_g[3];
  }
  if (!ggad_last_of(ticket, (int)gridDim.x, &flag)) return;
  if (w == 0) {
    float a = 0.f, q = 0.f;
    for (int k = lane; k < G; k += GGAD_WAVE) {
      a += ws[2 * k];
      q += ws[2 * k + 1];
    }
    a = wave_sum(a);
    q = wave_sum(q);
    if (lane == 0) {
      if (loss_ae) loss_ae[0] = nr > 0 ? a / (float)nr : 0.f;
      if (loss_g) loss_g[0] = n > 0 ? q / (float)n : 0.f;
    }
  }
}

// One wave per row i < n: dp[i] = *gloss_g p / max(p (1 - p), 1e-12) / n (torch's BCE backward, mean reduction; a saturated p
// gives 0, not NaN) and dzd[i, 0..ldz) = *gloss_ae (zd - x) / (nr attr) on a listed row (pos[i] >= 0), 0 elsewhere and past F.
__global__ __launch_bounds__(256) void k_loss_bwd(const float *__restrict__ p, int64_t n, const float *__restrict__ gloss_g,
                                                  float *__restrict__ dp, const float *__restrict__ x, int F, const float *__restrict__ zd,
                                                  int64_t ldz, const int32_t *__restrict__ pos, int64_t nr, const float *__restrict__ attr,
                                                  const float *__restrict__ gloss_ae, float *__restrict__ dzd) {
  const int lane = lane_id();
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  if (dp && lane == 0) {
    const float pi = p[i];
    dp[i] = gloss_g[0] * pi / fmaxf((1.f - pi) * pi, 1e-12f) / (float)n;
  }
  if (!dzd) return;
  const int k = pos[i];
  const float sc = k >= 0 ? gloss_ae[0] / ((float)nr * attr[k]) : 0.f;
  const float *xi = x + i * F, *zi = zd + i * ldz;
  float *di = dzd + i * ldz;
  for (int f = lane; f < ldz; f += GGAD_WAVE) di[f] = (k >= 0 && f < F) ? sc * (zi[f] - xi[f]) : 0.f;
}

// ------------------------------------------------------------------------------------------------ host side
static int bn_groups(int64_t M) {
  int64_t g = (M + BN_ROWS - 1) / BN_ROWS;
  if (g > BN_MAX_G) g = BN_MAX_G;
  return (int)(g < 1 ? 1 : g);
}
static int loss_groups(int64_t m) {
  int64_t g = (m + LOSS_ROWS - 1) / LOSS_ROWS;
  if (g > LOSS_MAX_G) g = LOSS_MAX_G;
  return (int)(g < 1 ? 1 : g);
}
static bool al16(const void *q) { return ((uintptr_t)q & 15) == 0; }

extern "C" {

int32_t ggad_aegis_bn_channels(void) { return BN_C; }
int32_t ggad_aegis_bn_groups(int64_t M) { return M >= 1 ? bn_groups(M) : 0; }
int32_t ggad_aegis_bn_rows_per_group(void) { return BN_ROWS; }
int64_t ggad_aegis_bn_workspace_elems(int64_t M, int32_t C) { return M >= 1 && C >= 1 ? (int64_t)bn_groups(M) * (3 * C + 1) : 0; }

int ggad_aegis_bn_fwd_f32(const float *h1, int64_t m1, int64_t ld1, const float *h2, int64_t m2, int64_t ld2, int32_t C,
                          const float *gamma, const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                          int64_t *num_batches_tracked, int32_t act, const int64_t *rows, int64_t n_out, float *y, int64_t ldy,
                          const float *w2, const float *b2, float *p, float *mean, float *invstd, float *ws, int32_t *ticket,
                          ggad_stream_t stream) {
  GGAD_REQUIRE(h1 && m1 >= 0 && m2 >= 0 && (m2 == 0 || h2) && gamma && beta && mean && invstd && ws && ticket && n_out >= 0);
  const int64_t M = m1 + m2;
  GGAD_REQUIRE(M >= 2);                                   // torch: "Expected more than 1 value per channel when training"
  GGAD_REQUIRE(act == 0 || act == 1);
  GGAD_REQUIRE(w2 ? (b2 && p) : (y != nullptr));
  if (C != BN_C) return GGAD_E_UNSUPPORTED;
  GGAD_REQUIRE(ld1 >= C && ld1 % 4 == 0 && al16(h1) && (m2 == 0 || (ld2 >= C && ld2 % 4 == 0 && al16(h2))));
  GGAD_REQUIRE(w2 || (ldy >= C && ldy % 4 == 0 && al16(y)));
  GGAD_REQUIRE(rows || n_out <= M);
  k_bn_stats<<<dim3(bn_groups(M)), dim3(256), 0, as_stream(stream)>>>(h1, m1, ld1, h2, ld2, M, eps, momentum, running_mean, running_var,
                                                                      num_batches_tracked, mean, invstd, ws, ticket);
  GGAD_CHECK_LAUNCH("aegis_bn_stats");
  if (n_out > 0) {
    k_bn_apply<<<dim3((unsigned)((n_out + 15) / 16)), dim3(256), 0, as_stream(stream)>>>(h1, m1, ld1, h2, ld2, rows, n_out, gamma, beta, mean,
                                                                                         invstd, act, y, ldy, w2, b2, p);
    GGAD_CHECK_LAUNCH("aegis_bn_apply");
  }
  return GGAD_OK;
}

int ggad_aegis_bn_bwd_f32(const float *h, int64_t M, int64_t ldh, int32_t C, const float *gamma, const float *beta, const float *mean,
                          const float *invstd, int32_t act, const float *dy, int64_t lddy, const float *w2, const float *p,
                          const float *dp, float *dh, int64_t lddh, float *dgamma, float *dbeta, float *dw2, float *db2, float *ws,
                          int32_t *ticket, ggad_stream_t stream) {
  GGAD_REQUIRE(h && gamma && beta && mean && invstd && dh && dgamma && dbeta && ws && ticket);
  GGAD_REQUIRE(M >= 2);
  GGAD_REQUIRE(act == 0 || act == 1);
  GGAD_REQUIRE(w2 ? (p && dp && dw2 && db2) : (dy != nullptr));
  if (C != BN_C) return GGAD_E_UNSUPPORTED;
  GGAD_REQUIRE(ldh >= C && ldh % 4 == 0 && al16(h) && lddh >= C && lddh % 4 == 0 && al16(dh));
  GGAD_REQUIRE(w2 || (lddy >= C && lddy % 4 == 0 && al16(dy)));
  k_bn_bwd_sums<<<dim3(bn_groups(M)), dim3(256), 0, as_stream(stream)>>>(h, M, ldh, gamma, beta, mean, invstd, act, dy, lddy, w2, p, dp,
                                                                         dgamma, dbeta, dw2, db2, ws, ticket);
  GGAD_CHECK_LAUNCH("aegis_bn_bwd_sums");
  k_bn_bwd_apply<<<dim3((unsigned)((M + 15) / 16)), dim3(256), 0, as_stream(stream)>>>(h, M, ldh, gamma, beta, mean, invstd, act, dy, lddy,
                                                                                      w2, p, dp, dgamma, dbeta, dh, lddh);
  GGAD_CHECK_LAUNCH("aegis_bn_bwd_apply");
  return GGAD_OK;
}

int64_t ggad_aegis_loss_workspace_elems(int64_t n, int64_t n_rows) {
  return 2 * (int64_t)loss_groups(n > n_rows ? n : n_rows);
}

int ggad_aegis_loss_fwd_f32(const float *p, int64_t n, const float *x, int32_t F, const float *zd, int64_t ldz, const int64_t *rows,
                            int64_t n_rows, float *attr, float *loss_g, float *loss_ae, float *ws, int32_t *ticket, ggad_stream_t stream) {
  GGAD_REQUIRE(n >= 0 && n_rows >= 0 && (n > 0 || n_rows > 0) && ws && ticket);
  GGAD_REQUIRE(n == 0 || p);
  GGAD_REQUIRE(n_rows == 0 || (x && zd && rows && attr && F >= 1 && ldz >= F));
  k_loss_fwd<<<dim3(loss_groups(n > n_rows ? n : n_rows)), dim3(256), 0, as_stream(stream)>>>(p, n, x, F, zd, ldz, rows, n_rows, attr,
                                                                                              loss_g, loss_ae, ws, ticket);
  GGAD_CHECK_LAUNCH("aegis_loss_fwd");
  return GGAD_OK;
}

int ggad_aegis_loss_bwd_f32(const float *p, int64_t n, const float *gloss_g, float *dp, const float *x, int32_t F, const float *zd,
                            int64_t ldz, const int32_t *pos, int64_t n_rows, const float *attr, const float *gloss_ae, float *dzd,
                            ggad_stream_t stream) {
  GGAD_REQUIRE(n >= 1 && (dp || dzd));
  GGAD_REQUIRE(!dp || (p && gloss_g));
  GGAD_REQUIRE(!dzd || (x && zd && pos && attr && gloss_ae && F >= 1 && ldz >= F && n_rows >= 1));
  k_loss_bwd<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream)>>>(p, n, gloss_g, dp, x, F, zd, ldz, pos, n_rows, attr,
                                                                                 gloss_ae, dzd);
  GGAD_CHECK_LAUNCH("aegis_loss_bwd");
  return GGAD_OK;
}

}  // extern "C"
