// Mini-batch AEGIS comparison model (reference src/graphsage_aegis.py:167-173, 298-323): the discriminator step on the two 1-hop
// aggregates of a batch, x_feat and x_noise (B x F each, rows [batch_ptr[i], batch_ptr[i + 1]) of the two plan tables).
//   fwd   E = relu([x_feat; x_noise] W^T) (2B x 64),  H = E W0^T + b0
//         call 1, all R = 2B rows:  mu, var (biased), S = sigmoid((H - mu) / sqrt(var + 1e-5) gamma + beta), p = sigmoid(S w1^T + b1),
//                                   loss_dis = mean BCE(p, [0..0 1..1])
//         call 2, the B noise rows: the same H rows under their own mu', var';  p';  loss_g = mean BCE(p', 0)
//   bwd   of loss_dis + loss_g into W, W0, b0, gamma, beta, w1, b1 (the noise rows of H receive both calls' contributions)
//   fold  running_mean / running_var / num_batches_tracked of the batch norm, call 1 then call 2 of every batch in batch order
// BCE and its gradient are torch's: logs clamped at -100, the divisor max((1 - p) p, 1e-12).
//
// Layout.  One workgroup of 1024 threads (16 waves) per batch, lane = channel.  Wave w owns the row blocks w, w + 16, ... of four rows;
// a thread keeps H of its <= 32 rows in registers (AM_MAX_B = 256 rows per half), so H is computed once and the statistics are two-pass
// (mean, then the sum of squared deviations: never E[x^2] - mu^2).  W and W0 sit transposed in LDS (s[k * 64 + lane]: conflict-free);
// the row operand of both products comes from the lanes of the wave itself (v_readlane of lane k), one fused multiply-add per term in
// ascending k: a fixed order.  Column sums: a thread over its rows in row order, then the 16 waves in wave order; the row dot with
// w1: the wave butterfly.  The backward is ONE workgroup per batch, so no partial sums leave the workgroup and there is no ticket:
// phase 1 column sums of du and du x_hat of both calls, dw1, db1;  phase 2 dH (written over the saved H), db0, dE = dH W0 masked by
// E > 0;  phase 3 dW0 = dH^T E and dW = dE^T x over 32-row tiles staged in LDS (a thread adds the 32 terms of a tile in row order,
// then the tiles in tile order).  No floating-point atomics, no allocation, no host synchronisation: equal inputs give equal bits,
// eager or replayed.
//
// Resources (hipcc -O3, gfx950; the .s of --save-temps):  k_amb_fwd  114 VGPRs, no scratch, 36,992 bytes of LDS;  k_amb_bwd  97 VGPRs,
// no scratch, 32,832 bytes of LDS;  k_amb_fold  14 VGPRs, no scratch, no LDS.  1,024 threads leave 128 VGPRs per thread; the LDS is
// below 64 KB, so no dynamic-LDS attribute is set.
// At B = 150 the step is bound by launch latency and by the dependent chains inside the one workgroup (two products of F + 64 terms,
// five barriers' worth of column sums), not by bandwidth or arithmetic.
#include "common.h"

#define AM_THREADS 1024
#define AM_WAVES (AM_THREADS / GGAD_WAVE)
#define AM_C 64                 // channels of the discriminator (the reference's hid_dim == in_dim == emb_size)
#define AM_MAX_F 64
#define AM_MAX_B 256            // rows of one half of a batch
#define AM_RB 4                 // rows of a block: one LDS read of a weight serves four rows
#define AM_ITERS (2 * AM_MAX_B / (AM_RB * AM_WAVES))      // row blocks per wave at most (8)
#define AM_TILE 32              // rows staged per tile of the weight-gradient phase
#define AM_EPS 1e-5f

namespace {

__device__ __forceinline__ float am_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float am_lane(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// column sum over the workgroup: the waves' values in wave order (every thread of a column returns the same bits)
__device__ __forceinline__ float am_colsum(float *s_red, int wave, int lane, float v) {
  s_red[wave * AM_C + lane] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < AM_WAVES; ++w) t += s_red[w * AM_C + lane];
  __syncthreads();
  return t;
}

// rows [r0, r0 + B) of the tables; false (workgroup-uniform) when the batch is outside what the kernels take
__device__ __forceinline__ bool am_batch(const int32_t *__restrict__ batch_ptr, int i, int total_rows, int &r0, int &B) {
  r0 = batch_ptr[i];
  B = batch_ptr[i + 1] - r0;
  return r0 >= 0 && B >= 2 && B <= AM_MAX_B && r0 <= total_rows - B;
}

// mode 0: every output;  1: also E, H and the two inverse standard deviations for the backward;  2: scores only -- p_all is the
// COMPACT real-row half (total_rows floats, row r0 + r), p_gen and losses are not written.
__global__ __launch_bounds__(AM_THREADS) void k_amb_fwd(const float *__restrict__ xf, const float *__restrict__ xn,
                                                         const int32_t *__restrict__ batch_ptr, int total_rows, int F,
                                                         const float *__restrict__ W, const float *__restrict__ W0,
                                                         const float *__restrict__ b0, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, const float *__restrict__ w1,
                                                         const float *__restrict__ b1, int mode, float *__restrict__ p_all,
                                                         float *__restrict__ p_gen, float *__restrict__ losses,
                                                         float *__restrict__ stats, float *__restrict__ sv_rows,
                                                         float *__restrict__ sv_istd) {
  __shared__ float s_wt[AM_MAX_F * AM_C];      // s_wt[k * 64 + c] = W[c][k]
  __shared__ float s_w0t[AM_C * AM_C];         // s_w0t[k * 64 + j] = W0[j][k]
  __shared__ float s_red[AM_WAVES * AM_C];
  __shared__ float s_l[2][AM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x;
  int r0, B;
  if (!am_batch(batch_ptr, i, total_rows, r0, B)) return;
  const int R = 2 * B;
  for (int o = tid; o < AM_C * F; o += AM_THREADS) {
    const int c = o / F, k = o - c * F;
    s_wt[k * AM_C + c] = W[o];
  }
  for (int o = tid; o < AM_C * AM_C; o += AM_THREADS) s_w0t[(o & 63) * AM_C + (o >> 6)] = W0[o];
  const float bias0 = b0[lane], gm = gamma[lane], bt = beta[lane], wl = w1[lane], bl = b1[0];
  __syncthreads();

  float h[AM_ITERS][AM_RB];
  float *sv_e = sv_rows, *sv_h = sv_rows + (size_t)2 * total_rows * AM_C;
#pragma unroll
  for (int it = 0; it < AM_ITERS; ++it) {
    const int base = (it * AM_WAVES + wave) * AM_RB;
#pragma unroll
    for (int q = 0; q < AM_RB; ++q) h[it][q] = 0.f;
    if (base < R) {
      float xr[AM_RB], a[AM_RB], e[AM_RB], hh[AM_RB];
#pragma unroll
      for (int q = 0; q < AM_RB; ++q) {
        const int r = base + q;
        const float *src = r < B ? xf + (size_t)(r0 + r) * F : xn + (size_t)(r0 + r - B) * F;
        xr[q] = (r < R && lane < F) ? src[lane] : 0.f;
        a[q] = 0.f;
        hh[q] = 0.f;
      }
      for (int k = 0; k < F; ++k) {
        const float w = s_wt[k * AM_C + lane];
#pragma unroll
        for (int q = 0; q < AM_RB; ++q) a[q] = fmaf(am_lane(xr[q], k), w, a[q]);
      }
#pragma unroll
      for (int q = 0; q < AM_RB; ++q) e[q] = a[q] < 0.f ? 0.f : a[q];
#pragma unroll 4
      for (int k = 0; k < AM_C; ++k) {
        const float w = s_w0t[k * AM_C + lane];
#pragma unroll
        for (int q = 0; q < AM_RB; ++q) hh[q] = fmaf(am_lane(e[q], k), w, hh[q]);
      }
#pragma unroll
      for (int q = 0; q < AM_RB; ++q) {
        const int r = base + q;
        h[it][q] = hh[q] + bias0;
        if (mode == 1 && r < R) {
          sv_e[((size_t)2 * r0 + r) * AM_C + lane] = e[q];
          sv_h[((size_t)2 * r0 + r) * AM_C + lane] = h[it][q];
        }
      }
    }
  }

  // statistics of both calls: means, then squared deviations
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int it = 0; it < AM_ITERS; ++it)
#pragma unroll
    for (int q = 0; q < AM_RB; ++q) {
      const int r = (it * AM_WAVES + wave) * AM_RB + q;
      if (r < R) {
        s1 += h[it][q];
        if (r >= B) s2 += h[it][q];
      }
    }
  const float mu1 = am_colsum(s_red, wave, lane, s1) / (float)R;
  const float mu2 = am_colsum(s_red, wave, lane, s2) / (float)B;
  s1 = 0.f;
  s2 = 0.f;
#pragma unroll
  for (int it = 0; it < AM_ITERS; ++it)
#pragma unroll
    for (int q = 0; q < AM_RB; ++q) {
      const int r = (it * AM_WAVES + wave) * AM_RB + q;
      if (r < R) {
        const float d1 = h[it][q] - mu1;
        s1 = fmaf(d1, d1, s1);
        if (r >= B) {
          const float d2 = h[it][q] - mu2;
          s2 = fmaf(d2, d2, s2);
        }
      }
    }
  const float q1 = am_colsum(s_red, wave, lane, s1), q2 = am_colsum(s_red, wave, lane, s2);
  const float istd1 = 1.f / sqrtf(q1 / (float)R + AM_EPS), istd2 = 1.f / sqrtf(q2 / (float)B + AM_EPS);
  if (wave == 0) {
    float *st = stats + (size_t)i * 4 * AM_C;
    st[lane] = mu1;
    st[AM_C + lane] = q1 / (float)(R - 1);            // unbiased: what the running variance takes
    st[2 * AM_C + lane] = mu2;
    st[3 * AM_C + lane] = q2 / (float)(B - 1);
    if (mode == 1) {
      sv_istd[(size_t)i * 2 * AM_C + lane] = istd1;
      sv_istd[(size_t)i * 2 * AM_C + AM_C + lane] = istd2;
    }
  }

  // heads and BCE terms
  float l1 = 0.f, l2 = 0.f;
#pragma unroll
  for (int it = 0; it < AM_ITERS; ++it)
#pragma unroll
    for (int q = 0; q < AM_RB; ++q) {
      const int r = (it * AM_WAVES + wave) * AM_RB + q;
      if (r >= R) continue;                             // wave-uniform
      if (mode == 2 && r >= B) continue;
      const float S = am_sigmoid((h[it][q] - mu1) * istd1 * gm + bt);
      const float p = am_sigmoid(wave_sum(S * wl) + bl);
      if (mode == 2) {
        if (lane == 0) p_all[r0 + r] = p;
        continue;
      }
      if (lane == 0) p_all[(size_t)2 * r0 + r] = p;
      l1 += r >= B ? -fmaxf(logf(p), -100.f) : -fmaxf(log1pf(-p), -100.f);
      if (r >= B) {
        const float S2 = am_sigmoid((h[it][q] - mu2) * istd2 * gm + bt);
        const float p2 = am_sigmoid(wave_sum(S2 * wl) + bl);
        if (lane == 0) p_gen[r0 + r - B] = p2;
        l2 += -fmaxf(log1pf(-p2), -100.f);
      }
    }
  if (mode == 2) return;
  if (lane == 0) {
    s_l[0][wave] = l1;
    s_l[1][wave] = l2;
  }
  __syncthreads();
  if (tid < 2) {
    float t = 0.f;
    for (int w = 0; w < AM_WAVES; ++w) t += s_l[tid][w];
    losses[2 * (size_t)i + tid] = t / (float)(tid == 0 ? R : B);
  }
}

// du and x_hat of one call at one (row, channel): dz = dp (1 - p) p with dp = (p - y) / max((1 - p) p, 1e-12) / n
struct AmCall {
  float xh, S, dz, du;
};
__device__ __forceinline__ AmCall am_call(float h, float mu, float istd, float gm, float bt, float wl, float p, float y, float n) {
  AmCall o;
  const float pq = (1.f - p) * p;
  o.dz = (p - y) / fmaxf(pq, 1e-12f) / n * pq;
  o.xh = (h - mu) * istd;
  o.S = am_sigmoid(o.xh * gm + bt);
  o.du = o.dz * wl * ((1.f - o.S) * o.S);
  return o;
}

__global__ __launch_bounds__(AM_THREADS) void k_amb_bwd(const float *__restrict__ xf, const float *__restrict__ xn,
                                                         const int32_t *__restrict__ batch_ptr, int total_rows, int F,
                                                         const float *__restrict__ W0, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, const float *__restrict__ w1,
                                                         const float *__restrict__ p_all, const float *__restrict__ p_gen,
                                                         const float *__restrict__ stats, float *sv_rows,
                                                         const float *__restrict__ sv_istd, float *__restrict__ dW,
                                                         float *__restrict__ dW0, float *__restrict__ db0, float *__restrict__ dgamma,
                                                         float *__restrict__ dbeta, float *__restrict__ dw1, float *__restrict__ db1) {
  // phases 1-2: s_w0 (4096) | s_red (1024);  phase 3: four staged tiles of AM_TILE x 64 (8192)
  __shared__ float s_mem[4 * AM_TILE * AM_C];
  __shared__ float s_z[AM_WAVES];
  float *s_w0 = s_mem, *s_red = s_mem + AM_C * AM_C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int r0, B;
  if (!am_batch(batch_ptr, 0, total_rows, r0, B)) return;
  const int R = 2 * B;
  const float *sv_e = sv_rows;
  float *sv_h = sv_rows + (size_t)2 * total_rows * AM_C, *sv_g = sv_rows + (size_t)4 * total_rows * AM_C;
  for (int o = tid; o < AM_C * AM_C; o += AM_THREADS) s_w0[o] = W0[o];                    // s_w0[j * 64 + k]
  const float gm = gamma[lane], bt = beta[lane], wl = w1[lane];
  const float mu1 = stats[lane], mu2 = stats[2 * AM_C + lane], istd1 = sv_istd[lane], istd2 = sv_istd[AM_C + lane];
  const float fR = (float)R, fB = (float)B;

  // ---- phase 1: column sums
  float sdu1 = 0.f, sdux1 = 0.f, sdu2 = 0.f, sdux2 = 0.f, sw1 = 0.f, sz = 0.f;
  for (int it = 0; it < AM_ITERS; ++it)
    for (int q = 0; q < AM_RB; ++q) {
      const int r = (it * AM_WAVES + wave) * AM_RB + q;
      if (r >= R) continue;
      const float hv = sv_h[((size_t)2 * r0 + r) * AM_C + lane];
      const AmCall c1 = am_call(hv, mu1, istd1, gm, bt, wl, p_all[(size_t)2 * r0 + r], r >= B ? 1.f : 0.f, fR);
      sdu1 += c1.du;
      sdux1 = fmaf(c1.du, c1.xh, sdux1);
      sw1 = fmaf(c1.dz, c1.S, sw1);
      sz += c1.dz;
      if (r >= B) {
        const AmCall c2 = am_call(hv, mu2, istd2, gm, bt, wl, p_gen[r0 + r - B], 0.f, fB);
        sdu2 += c2.du;
        sdux2 = fmaf(c2.du, c2.xh, sdux2);
        sw1 = fmaf(c2.dz, c2.S, sw1);
        sz += c2.dz;
      }
    }
  __syncthreads();                                       // s_w0 is loaded
  sdu1 = am_colsum(s_red, wave, lane, sdu1);
  sdux1 = am_colsum(s_red, wave, lane, sdux1);
  sdu2 = am_colsum(s_red, wave, lane, sdu2);
  sdux2 = am_colsum(s_red, wave, lane, sdux2);
  sw1 = am_colsum(s_red, wave, lane, sw1);
  if (lane == 0) s_z[wave] = sz;
  __syncthreads();
  if (wave == 0) {
    dbeta[lane] = sdu1 + sdu2;
    dgamma[lane] = sdux1 + sdux2;
    dw1[lane] = sw1;
    if (lane == 0) {
      float t = 0.f;
      for (int w = 0; w < AM_WAVES; ++w) t += s_z[w];
      db1[0] = t;
    }
  }

  // ---- phase 2: dH over H, db0, dE masked
  const float m1 = sdu1 / fR, mx1 = sdux1 / fR, m2 = sdu2 / fB, mx2 = sdux2 / fB, g1 = istd1 * gm, g2 = istd2 * gm;
  float sb0 = 0.f;
  for (int it = 0; it < AM_ITERS; ++it) {
    const int base = (it * AM_WAVES + wave) * AM_RB;
    if (base >= R) continue;
    float dh[AM_RB], de[AM_RB];
#pragma unroll
    for (int q = 0; q < AM_RB; ++q) {
      const int r = base + q;
      dh[q] = 0.f;
      de[q] = 0.f;
      if (r < R) {
        const float hv = sv_h[((size_t)2 * r0 + r) * AM_C + lane];
        const AmCall c1 = am_call(hv, mu1, istd1, gm, bt, wl, p_all[(size_t)2 * r0 + r], r >= B ? 1.f : 0.f, fR);
        dh[q] = (c1.du - m1 - c1.xh * mx1) * g1;
        if (r >= B) {
          const AmCall c2 = am_call(hv, mu2, istd2, gm, bt, wl, p_gen[r0 + r - B], 0.f, fB);
          dh[q] += (c2.du - m2 - c2.xh * mx2) * g2;
        }
        sb0 += dh[q];
        sv_h[((size_t)2 * r0 + r) * AM_C + lane] = dh[q];
      }
    }
#pragma unroll 4
    for (int j = 0; j < AM_C; ++j) {
      const float w = s_w0[j * AM_C + lane];
#pragma unroll
      for (int q = 0; q < AM_RB; ++q) de[q] = fmaf(am_lane(dh[q], j), w, de[q]);
    }
#pragma unroll
    for (int q = 0; q < AM_RB; ++q) {
      const int r = base + q;
      if (r < R) {
        const size_t at = ((size_t)2 * r0 + r) * AM_C + lane;
        sv_g[at] = sv_e[at] > 0.f ? de[q] : 0.f;
      }
    }
  }
  sb0 = am_colsum(s_red, wave, lane, sb0);
  if (wave == 0) db0[lane] = sb0;
  __threadfence_block();
  __syncthreads();                                       // dH and dE of every row are written; s_w0 / s_red are free

  // ---- phase 3: dW0[j][k] = sum_r dH[r][j] E[r][k],  dW[c][k] = sum_r dE[r][c] x[r][k]
  float *s_dh = s_mem, *s_e = s_mem + AM_TILE * AM_C, *s_g = s_mem + 2 * AM_TILE * AM_C, *s_x = s_mem + 3 * AM_TILE * AM_C;
  const int n_w = AM_C * F;
  int oc[4], ok[4];
  float a0[4] = {0.f, 0.f, 0.f, 0.f}, aw[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = tid + u * AM_THREADS;
    oc[u] = o < n_w ? o / F : 0;
    ok[u] = o < n_w ? o - oc[u] * F : 0;
  }
  for (int t0 = 0; t0 < R; t0 += AM_TILE) {
    __syncthreads();                                     // the last tile has been read
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int idx = tid + v * AM_THREADS, row = idx >> 6, c = idx & 63, r = t0 + row;
      const bool live = r < R;
      const size_t at = ((size_t)2 * r0 + (live ? r : 0)) * AM_C + c;
      s_dh[idx] = live ? sv_h[at] : 0.f;
      s_e[idx] = live ? sv_e[at] : 0.f;
      s_g[idx] = live ? sv_g[at] : 0.f;
      float xv = 0.f;
      if (live && c < F) xv = r < B ? xf[(size_t)(r0 + r) * F + c] : xn[(size_t)(r0 + r - B) * F + c];
      s_x[idx] = xv;
    }
    __syncthreads();
    float p0[4] = {0.f, 0.f, 0.f, 0.f}, pw[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int r = 0; r < AM_TILE; ++r) {                  // rows past R are zeros: they add +0
      const float ev = s_e[r * AM_C + lane];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        p0[u] = fmaf(s_dh[r * AM_C + wave + AM_WAVES * u], ev, p0[u]);
        pw[u] = fmaf(s_g[r * AM_C + oc[u]], s_x[r * AM_C + ok[u]], pw[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a0[u] += p0[u];
      aw[u] += pw[u];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    dW0[(wave + AM_WAVES * u) * AM_C + lane] = a0[u];
    const int o = tid + u * AM_THREADS;
    if (o < n_w) dW[o] = aw[u];
  }
}

// running <- momentum * batch + (1 - momentum) * running, call 1 then call 2 of every batch in batch order (lane = channel)
__global__ __launch_bounds__(AM_C) void k_amb_fold(const float *__restrict__ stats, int n_batches, float momentum,
                                                    float *__restrict__ run_mean, float *__restrict__ run_var,
                                                    int64_t *__restrict__ n_tracked) {
  const int c = threadIdx.x;
  float m = run_mean[c], v = run_var[c];
  const float keep = 1.f - momentum;
  for (int i = 0; i < n_batches; ++i) {
    const float *st = stats + (size_t)i * 4 * AM_C;
    m = momentum * st[c] + keep * m;
    v = momentum * st[AM_C + c] + keep * v;
    m = momentum * st[2 * AM_C + c] + keep * m;
    v = momentum * st[3 * AM_C + c] + keep * v;
  }
  run_mean[c] = m;
  run_var[c] = v;
  if (c == 0 && n_tracked) n_tracked[0] += 2 * (int64_t)n_batches;
}

}  // namespace

extern "C" {

int32_t ggad_aegis_mb_max_rows(void) { return AM_MAX_B; }
int32_t ggad_aegis_mb_supported(int32_t feat_dim, int32_t embed_dim, int32_t max_rows) {
  return feat_dim >= 1 && feat_dim <= AM_MAX_F && embed_dim == AM_C && max_rows >= 2 && max_rows <= AM_MAX_B;
}
int64_t ggad_aegis_mb_scratch_elems(int64_t total_rows) { return total_rows >= 1 ? 6 * total_rows * AM_C : 0; }

int ggad_aegis_mb_fwd_f32(const float *x_feat, const float *x_noise, const int32_t *batch_ptr, int32_t n_batches, int32_t total_rows,
                          int32_t max_rows, int32_t feat_dim, int32_t embed_dim, const float *w_enc, const float *w0, const float *b0,
                          const float *gamma, const float *beta, const float *w1, const float *b1, int32_t mode, float *p_all,
                          float *p_gen, float *losses, float *stats, float *scratch, float *inv_std, ggad_stream_t stream) {
  GGAD_REQUIRE(x_feat && x_noise && batch_ptr && w_enc && w0 && b0 && gamma && beta && w1 && b1 && p_all && stats);
  GGAD_REQUIRE(n_batches >= 1 && total_rows >= 2 && mode >= 0 && mode <= 2);
  GGAD_REQUIRE(mode == 2 || (p_gen && losses));
  GGAD_REQUIRE(mode != 1 || (scratch && inv_std));
  if (!ggad_aegis_mb_supported(feat_dim, embed_dim, max_rows)) return GGAD_E_UNSUPPORTED;
  k_amb_fwd<<<dim3((unsigned)n_batches), dim3(AM_THREADS), 0, as_stream(stream)>>>(x_feat, x_noise, batch_ptr, total_rows, feat_dim, w_enc,
                                                                                   w0, b0, gamma, beta, w1, b1, mode, p_all, p_gen, losses,
                                                                                   stats, scratch, inv_std);
  GGAD_CHECK_LAUNCH("aegis_mb_fwd");
  return GGAD_OK;
}

int ggad_aegis_mb_bwd_f32(const float *x_feat, const float *x_noise, const int32_t *batch_ptr, int32_t total_rows, int32_t max_rows,
                          int32_t feat_dim, int32_t embed_dim, const float *w0, const float *gamma, const float *beta, const float *w1,
                          const float *p_all, const float *p_gen, const float *stats, float *scratch, const float *inv_std,
                          float *d_w_enc, float *d_w0, float *d_b0, float *d_gamma, float *d_beta, float *d_w1, float *d_b1,
                          ggad_stream_t stream) {
  GGAD_REQUIRE(x_feat && x_noise && batch_ptr && w0 && gamma && beta && w1 && p_all && p_gen && stats && scratch && inv_std);
  GGAD_REQUIRE(d_w_enc && d_w0 && d_b0 && d_gamma && d_beta && d_w1 && d_b1 && total_rows >= 2);
  if (!ggad_aegis_mb_supported(feat_dim, embed_dim, max_rows)) return GGAD_E_UNSUPPORTED;
  k_amb_bwd<<<dim3(1), dim3(AM_THREADS), 0, as_stream(stream)>>>(x_feat, x_noise, batch_ptr, total_rows, feat_dim, w0, gamma, beta, w1, p_all,
                                                                 p_gen, stats, scratch, inv_std, d_w_enc, d_w0, d_b0, d_gamma, d_beta, d_w1,
                                                                 d_b1);
  GGAD_CHECK_LAUNCH("aegis_mb_bwd");
  return GGAD_OK;
}

int ggad_aegis_mb_fold_f32(const float *stats, int32_t n_batches, float momentum, float *running_mean, float *running_var,
                           int64_t *num_batches_tracked, ggad_stream_t stream) {
  GGAD_REQUIRE(stats && running_mean && running_var && n_batches >= 1);
  k_amb_fold<<<dim3(1), dim3(AM_C), 0, as_stream(stream)>>>(stats, n_batches, momentum, running_mean, running_var, num_batches_tracked);
  GGAD_CHECK_LAUNCH("aegis_mb_fold");
  return GGAD_OK;
}

}  // extern "C"
