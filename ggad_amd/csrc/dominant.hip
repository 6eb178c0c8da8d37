// Full-graph DOMINANT comparison model (reference model_domaint.py / dominant.py): the attribute autoencoder and its loss.
//
// Per epoch the reference evaluates  x_ = W2 relu(W1 x + b1) + b2  on all N rows and reads it at two row lists:
//
//   score_k = ||x_r - x_r_hat||   (r = idx_test[k]),     loss = mean_{i in idx_train} ||x_i - x_i_hat||.
//
// Its GCN branch never reaches the loss (ggad_amd/model_dominant.py runs it on the GCN kernels and caches it), so the epoch is this
// autoencoder alone.
//
//   ggad_dominant_ae_f32     the fused path: ONE launch over the row list [train | test].  Per 16-row tile a workgroup gathers the
//                            rows of X, runs H = relu(X W1^T + b1) and X_ = H W2^T + b2 on fp32 MFMA (v_mfma_f32_16x16x4_f32),
//                            the per-row error norm, and on train tiles the backward at d loss = 1: G = (X_ - X) / (e m),
//                            dH = (G W2) . [H > 0], and dW1 += dH^T X, dW2 += G^T H, dB1 += colsum dH, dB2 += colsum G, the
//                            weight gradients held in MFMA accumulators across the workgroup's tiles.  x_ is never written; only
//                            listed rows are computed.  Each workgroup writes one partial; the last of each group of 16 (a ticket)
//                            adds its group's partials in order, and the last group adds the group sums in order.  No float
//                            atomics, so eager launches and graph replays are bitwise repeatable.
//   ggad_dominant_recon_f32  the wide path's loss: (x, x_, row lists) -> loss, scores and dX_ (every row written) in one launch.
//   ggad_dominant_scale_f32  dst = src * g[0]: the incoming loss gradient applied to gradients computed at d loss = 1.
//
// The fused path holds (H, F) when 2 ceil(H/16) ceil(F/16) <= DOM_MAX_TILES (the weight-gradient tiles of the 8 waves),
// ceil(F/16) <= DOM_MAX_FT, ceil(H/16) <= DOM_MAX_HT and the tile's LDS fits 64 KiB; ggad_dominant_ae_supported says so.
// n_h = 300 holds F <= 96.
#include "common.h"
#include "handoff.h"

#define DOM_THREADS 512                  // 8 waves
#define DOM_WAVES (DOM_THREADS / GGAD_WAVE)
#define DOM_TM 16                        // rows per tile
#define DOM_MAX_TILES 240                // gradient tiles (16 x 16) of dW1 and dW2 together
#define DOM_TPW (DOM_MAX_TILES / DOM_WAVES)  // accumulator tiles per wave (30)
#define DOM_MAX_FT 8                     // F <= 128
#define DOM_MAX_HT 32                    // H <= 512
#define DOM_MAX_G 256                    // workgroups at most
#define DOM_GROUP 16                     // partials per first-level reducer
#define RECON_MAX_G 256

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// out[e] = sum_{k < cnt} src[k * P + e] in k order, cnt <= DOM_GROUP (plain loads behind the acquire; all cnt of an element in
// flight before the first add)
__device__ __forceinline__ void dom_sum_partials(const float *src, int cnt, int64_t P, float *out) {
  for (int64_t e = threadIdx.x; e < P; e += DOM_THREADS) {
    float v[DOM_GROUP];
#pragma unroll
    for (int k = 0; k < DOM_GROUP; ++k) v[k] = k < cnt ? src[(int64_t)k * P + e] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < DOM_GROUP; ++k)
      if (k < cnt) s += v[k];
    out[e] = s;
  }
}

// ------------------------------------------------------------------------------------------------ fused autoencoder
// Partial layout (P floats): dW1 (H x F), dB1 (H), dW2 (F x H), dB2 (F), loss sum (1).
// LDS (floats): sX[16][FP], sH[16][HP], sG[16][FP], sD[16][HP], sE[16].  FP = 16 ceil(F / 16), HP = 16 ceil(H / 16); the pad
// columns are zero (W1 rows / W2 columns past H and F are read as zero), so the products over them add exact zeros.
__global__ __launch_bounds__(DOM_THREADS) void k_dominant_ae(
    const float *__restrict__ x, int F, const int64_t *__restrict__ rows, int64_t m, int64_t t_rows, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, int H, float *__restrict__ score,
    float *__restrict__ loss, float *__restrict__ dW1, float *__restrict__ dB1, float *__restrict__ dW2, float *__restrict__ dB2,
    float *__restrict__ ws, int32_t *__restrict__ tickets) {
  extern __shared__ float lds[];
  __shared__ int flag;
  const int FT = (F + 15) >> 4, HT = (H + 15) >> 4, FP = FT * 16, HP = HT * 16;
  float *sX = lds, *sH = sX + DOM_TM * FP, *sG = sH + DOM_TM * HP, *sD = sG + DOM_TM * FP, *sE = sD + DOM_TM * HP;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t n_train_t = (m + DOM_TM - 1) / DOM_TM, n_test_t = (t_rows + DOM_TM - 1) / DOM_TM, T = n_train_t + n_test_t;
  const int64_t G = gridDim.x, b = blockIdx.x;
  const int n_acc = 2 * HT * FT;                       // tiles [0, HT FT): dW1 (jn, jf); [HT FT, 2 HT FT): dW2 (jf, jn)

  f32x4 acc[DOM_TPW];
#pragma unroll
  for (int s = 0; s < DOM_TPW; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f, db2 = 0.f, lsum = 0.f;               // dB1[tid] (tid < H), dB2[tid] (tid < F), loss sum (thread 0)

  for (int64_t tile = T * b / G; tile < T * (b + 1) / G; ++tile) {
    const bool train = tile < n_train_t;
    const int64_t k0 = train ? tile * DOM_TM : m + (tile - n_train_t) * DOM_TM;
    const int64_t kend = train ? m : m + t_rows;
    const int valid = (int)(kend - k0 < DOM_TM ? kend - k0 : DOM_TM);
    // (1) the X rows of the tile (zero past F and past the list)
    for (int e = tid; e < DOM_TM * FP; e += DOM_THREADS) {
      const int r = e / FP, f = e - r * FP;
      sX[e] = (r < valid && f < F) ? x[rows[k0 + r] * (int64_t)F + f] : 0.f;
    }
    __syncthreads();
    // (2) H = relu(X W1^T + b1): output tile j (hidden units 16 j ..), K = FP
    for (int j = w; j < HT; j += DOM_WAVES) {
      const int n = 16 * j + li;
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int k = 0; k < FP; k += 4) {
        const int kk = k + lk;
        c = mfma4(sX[li * FP + kk], (n < H && kk < F) ? W1[(int64_t)n * F + kk] : 0.f, c);
      }
      const float bb = n < H ? b1[n] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) sH[(4 * lk + i) * HP + n] = fmaxf(c[i] + bb, 0.f);
    }
    __syncthreads();
    // (3) X_ = H W2^T + b2 and the difference D = X_ - X (kept in sG): output tile j (features 16 j ..), K = HP
    for (int j = w; j < FT; j += DOM_WAVES) {
      const int f = 16 * j + li;
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int k = 0; k < HP; k += 4) {
        const int kk = k + lk;
        c = mfma4(sH[li * HP + kk], (f < F && kk < H) ? W2[(int64_t)f * H + kk] : 0.f, c);
      }
      const float bb = f < F ? b2[f] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lk + i;
        sG[r * FP + f] = (f < F && r < valid) ? (c[i] + bb) - sX[r * FP + f] : 0.f;
      }
    }
    __syncthreads();
    // (4) e_r = ||D_r||: wave w takes rows w and w + 8, lanes over the columns in order, then the butterfly
    for (int r = w; r < DOM_TM; r += DOM_WAVES) {
      float s = 0.f;
      for (int f = lane; f < FP; f += GGAD_WAVE) {
        const float d = sG[r * FP + f];
        s += d * d;
      }
      s = sqrtf(wave_sum(s));
      if (lane == 0) {
        sE[r] = s;
        if (!train && r < valid) score[k0 - m + r] = s;
      }
    }
    __syncthreads();
    if (!train) continue;                               // (a uniform branch: the whole workgroup sees the same tile)
    if (tid == 0)
      for (int r = 0; r < valid; ++r) lsum += sE[r];
    // (5) G = D / (e m) on the valid rows (the others are zero already)
    for (int e = tid; e < DOM_TM * FP; e += DOM_THREADS) {
      const int r = e / FP;
      if (r < valid) sG[e] = sG[e] / (sE[r] * (float)m);
    }
    __syncthreads();
    // (6) dH = (G W2) . [H > 0]: output tile j (hidden units), K = FP
    for (int j = w; j < HT; j += DOM_WAVES) {
      const int n = 16 * j + li;
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int k = 0; k < FP; k += 4) {
        const int kk = k + lk;
        c = mfma4(sG[li * FP + kk], (n < H && kk < F) ? W2[(int64_t)kk * H + n] : 0.f, c);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lk + i;
        sD[r * HP + n] = sH[r * HP + n] > 0.f ? c[i] : 0.f;
      }
    }
    __syncthreads();
    // (7) the weight gradients of this tile into the wave's accumulators (K = the 16 rows), the bias gradients per thread
#pragma unroll
    for (int s = 0; s < DOM_TPW; ++s) {
      const int q = w + DOM_WAVES * s;
      if (q < n_acc) {
        const bool is1 = q < HT * FT;
        const int qq = is1 ? q : q - HT * FT;
        // dW1 tile (jn, jf): A[n][r] = dH[r][n], B[r][f] = X[r][f];  dW2 tile (jf, jn): A[f][r] = G[r][f], B[r][n] = H[r][n]
        const int ja = is1 ? qq / FT : qq / HT, jb = is1 ? qq % FT : qq % HT;
        const float *A = is1 ? sD : sG, *B = is1 ? sX : sH;
        const int lda = is1 ? HP : FP, ldb = is1 ? FP : HP;
#pragma unroll
        for (int k = 0; k < DOM_TM; k += 4)
          acc[s] = mfma4(A[(k + lk) * lda + 16 * ja + li], B[(k + lk) * ldb + 16 * jb + li], acc[s]);
      }
    }
    if (tid < HP)
      for (int r = 0; r < DOM_TM; ++r) db1 += sD[r * HP + tid];
    if (tid < FP)
      for (int r = 0; r < DOM_TM; ++r) db2 += sG[r * FP + tid];
    __syncthreads();
  }

  // this workgroup's partial
  const int64_t P = 2 * (int64_t)H * F + H + F + 1;
  float *part = ws + b * P;
#pragma unroll
  for (int s = 0; s < DOM_TPW; ++s) {
    const int q = w + DOM_WAVES * s;
    if (q < n_acc) {
      const bool is1 = q < HT * FT;
      const int qq = is1 ? q : q - HT * FT;
      const int ja = is1 ? qq / FT : qq / HT, jb = is1 ? qq % FT : qq % HT;
      const int col = 16 * jb + li;                    // C/D: col = lane & 15, row = 4 (lane >> 4) + i
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 16 * ja + 4 * lk + i;
        if (is1) {
          if (row < H && col < F) part[(int64_t)row * F + col] = acc[s][i];
        } else {
          if (row < F && col < H) part[(int64_t)H * F + H + (int64_t)row * H + col] = acc[s][i];
        }
      }
    }
  }
  if (tid < H) part[(int64_t)H * F + tid] = db1;
  if (tid < F) part[2 * (int64_t)H * F + H + tid] = db2;
  if (tid == 0) part[P - 1] = lsum;

  // first level: the last workgroup of group g adds the group's partials in order
  const int NG = (int)((G + DOM_GROUP - 1) / DOM_GROUP), g = (int)(b / DOM_GROUP);
  const int g0 = g * DOM_GROUP, gcnt = (int)((G - g0) < DOM_GROUP ? (G - g0) : DOM_GROUP);
  if (!ggad_last_of(tickets + g, gcnt, &flag)) return;
  float *gpart = ws + G * P + (int64_t)g * P;
  dom_sum_partials(ws + (int64_t)g0 * P, gcnt, P, gpart);
  // second level: the last group adds the group sums in order into the outputs
  if (!ggad_last_of(tickets + DOM_MAX_G / DOM_GROUP, NG, &flag)) return;
  const float *gs = ws + G * P;
  for (int64_t e = tid; e < P; e += DOM_THREADS) {
    float v[DOM_MAX_G / DOM_GROUP];
#pragma unroll
    for (int k = 0; k < DOM_MAX_G / DOM_GROUP; ++k) v[k] = k < NG ? gs[(int64_t)k * P + e] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < DOM_MAX_G / DOM_GROUP; ++k)
      if (k < NG) s += v[k];
    const int64_t HF = (int64_t)H * F;
    if (e < HF) dW1[e] = s;
    else if (e < HF + H) dB1[e - HF] = s;
    else if (e < 2 * HF + H) dW2[e - HF - H] = s;
    else if (e < 2 * HF + H + F) dB2[e - 2 * HF - H] = s;
    else loss[0] = s / (float)m;
  }
}

// ------------------------------------------------------------------------------------------------ wide path: the loss over x_
// One wave per task: tasks [0, m) the train rows (e, dX_ row = (x_ - x) / (e m), e summed per wave in task order), [m, m + t) the
// test rows (score), [m + t, m + t + N) row i - m - t of dX_ set to zero when it is not a train row (pos < 0).  Workgroup b takes the
// tasks [T b / G, T (b + 1) / G); its waves' sums in wave order are its partial, the last workgroup adds the partials in order.
__global__ __launch_bounds__(256) void k_dominant_recon(const float *__restrict__ x, const float *__restrict__ xh, int64_t n, int F,
                                                        const int64_t *__restrict__ rows, int64_t m, int64_t t_rows,
                                                        const int32_t *__restrict__ pos, float *__restrict__ score,
                                                        float *__restrict__ loss, float *__restrict__ dxh, float *__restrict__ ws,
                                                        int32_t *__restrict__ ticket) {
  __shared__ float s_l[4];
  __shared__ int flag;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t G = gridDim.x, b = blockIdx.x, T = m + t_rows + n;
  float ls = 0.f;
  for (int64_t k = T * b / G + w; k < T * (b + 1) / G; k += 4) {
    if (k < m + t_rows) {
      const int64_t i = rows[k];
      const float *xi = x + i * F, *hi = xh + i * F;
      float s = 0.f;
      for (int f = lane; f < F; f += GGAD_WAVE) {
        const float d = hi[f] - xi[f];
        s += d * d;
      }
      s = sqrtf(wave_sum(s));
      if (k < m) {
        ls += s;
        const float den = s * (float)m;
        for (int f = lane; f < F; f += GGAD_WAVE) dxh[i * F + f] = (hi[f] - xi[f]) / den;
      } else if (lane == 0) {
        score[k - m] = s;
      }
    } else {
      const int64_t i = k - m - t_rows;
      if (pos[i] < 0)
        for (int f = lane; f < F; f += GGAD_WAVE) dxh[i * F + f] = 0.f;
    }
  }
  if (lane == 0) s_l[w] = ls;
  __syncthreads();
  if (tid == 0) ws[b] = ((s_l[0] + s_l[1]) + s_l[2]) + s_l[3];
  if (!ggad_last_of(ticket, (int)G, &flag)) return;
  if (tid == 0) {
    float s = 0.f;
    for (int64_t k = 0; k < G; ++k) s += __hip_atomic_load(ws + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    loss[0] = s / (float)m;
  }
}

__global__ __launch_bounds__(256) void k_dominant_scale(const float *__restrict__ src, int64_t n, const float *__restrict__ g,
                                                        float *__restrict__ dst) {
  const float gg = g[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i] * gg;
}

// ------------------------------------------------------------------------------------------------ host side
static bool dom_fits(int32_t F, int32_t H) {
  if (F < 1 || H < 1) return false;
  const int64_t ft = (F + 15) / 16, ht = (H + 15) / 16;
  // (the LDS of one workgroup, 2 DOM_TM (FP + HP) + DOM_TM floats, stays within 64 KiB)
  return ft <= DOM_MAX_FT && ht <= DOM_MAX_HT && 2 * ft * ht <= DOM_MAX_TILES && 2 * DOM_TM * 16 * (ft + ht) + DOM_TM <= 16384;
}
static int64_t dom_groups(int64_t m, int64_t t) {
  const int64_t T = (m + DOM_TM - 1) / DOM_TM + (t + DOM_TM - 1) / DOM_TM;
  return T < 1 ? 1 : (T < DOM_MAX_G ? T : DOM_MAX_G);
}
static int64_t recon_groups(int64_t tasks) {
  const int64_t g = (tasks + 63) / 64;
  return g < 1 ? 1 : (g < RECON_MAX_G ? g : RECON_MAX_G);
}

extern "C" {

int32_t ggad_dominant_ae_supported(int32_t F, int32_t H) { return dom_fits(F, H) ? 1 : 0; }
int32_t ggad_dominant_tickets(void) { return DOM_MAX_G / DOM_GROUP + 1; }

int64_t ggad_dominant_ae_workspace_elems(int64_t m, int64_t t_rows, int32_t F, int32_t H) {
  if (m < 0 || t_rows < 0 || !dom_fits(F, H)) return 0;
  const int64_t G = dom_groups(m, t_rows), P = 2 * (int64_t)H * F + H + F + 1;
  return (G + (G + DOM_GROUP - 1) / DOM_GROUP) * P;
}

int ggad_dominant_ae_f32(const float *x, int32_t F, const int64_t *rows, int64_t m, int64_t t_rows, const float *W1, const float *b1,
                         const float *W2, const float *b2, int32_t H, float *score, float *loss, float *dW1, float *dB1, float *dW2,
                         float *dB2, float *ws, int32_t *tickets, ggad_stream_t stream) {
  if (!dom_fits(F, H)) return GGAD_E_UNSUPPORTED;
  GGAD_REQUIRE(x && rows && m >= 1 && t_rows >= 0 && (t_rows == 0 || score) && W1 && b1 && W2 && b2 && loss);
  GGAD_REQUIRE(dW1 && dB1 && dW2 && dB2 && ws && tickets);
  const int64_t G = dom_groups(m, t_rows);
  const int FP = (F + 15) / 16 * 16, HP = (H + 15) / 16 * 16;
  const size_t lds = sizeof(float) * (size_t)(2 * DOM_TM * FP + 2 * DOM_TM * HP + DOM_TM);
  k_dominant_ae<<<dim3((unsigned)G), dim3(DOM_THREADS), lds, as_stream(stream)>>>(x, F, rows, m, t_rows, W1, b1, W2, b2, H, score, loss,
                                                                                   dW1, dB1, dW2, dB2, ws, tickets);
  GGAD_CHECK_LAUNCH("dominant_ae");
  return GGAD_OK;
}

int64_t ggad_dominant_recon_workspace_elems(int64_t n, int64_t m, int64_t t_rows) { return recon_groups(n + m + t_rows); }

int ggad_dominant_recon_f32(const float *x, const float *xh, int64_t n, int32_t F, const int64_t *rows, int64_t m, int64_t t_rows,
                            const int32_t *pos, float *score, float *loss, float *dxh, float *ws, int32_t *ticket,
                            ggad_stream_t stream) {
  GGAD_REQUIRE(x && xh && n >= 1 && F >= 1 && rows && m >= 1 && t_rows >= 0 && (t_rows == 0 || score) && pos && loss && dxh && ws &&
               ticket);
  k_dominant_recon<<<dim3((unsigned)recon_groups(n + m + t_rows)), dim3(256), 0, as_stream(stream)>>>(x, xh, n, F, rows, m, t_rows, pos,
                                                                                                       score, loss, dxh, ws, ticket);
  GGAD_CHECK_LAUNCH("dominant_recon");
  return GGAD_OK;
}

int ggad_dominant_scale_f32(const float *src, int64_t n, const float *g, float *dst, ggad_stream_t stream) {
  GGAD_REQUIRE(src && g && dst && n >= 0);
  if (n == 0) return GGAD_OK;
  int64_t grid = (n + 255) / 256;
  if (grid > 1024) grid = 1024;
  k_dominant_scale<<<dim3((unsigned)grid), dim3(256), 0, as_stream(stream)>>>(src, n, g, dst);
  GGAD_CHECK_LAUNCH("dominant_scale");
  return GGAD_OK;
}

}  // extern "C"
