// Mini-batch DOMINANT / AnomalyDAE comparison models (reference src/graphsage_dominant.py:154-158, 274-276): the optimiser steps of an
// epoch in ONE launch of ONE workgroup, and the validation score of test_recon (src/utils.py:150-159) without h or r in HBM.
//   h = relu(x1 W^T) (B x 64),  r = relu(h Wfc^T) (B x F),  s_c = sum_b w(r_bc) (r_bc - t_bc)^2,  loss = mean_c sqrt(s_c)
//   dr = [r > 0] w (r - t) / sqrt(s_c) / F,  dWfc = dr^T h,  dh = [h > 0] dr Wfc,  dW = dh^T x1,  then Adam with L2 weight decay.
// Step s + 1 reads the weights step s wrote, so the steps are a serial chain; one workgroup that keeps the two weights and their four
// moments on chip loses no parallelism the chain of launches had, and needs no cross-workgroup synchronisation.
//
// Layout of k_rm_steps.  1,024 threads (16 waves).  Thread (own = tid / 16, q = tid % 16) owns Wfc[own][4q .. 4q + 3] and
// W[4q .. 4q + 3][own] with their moments in registers for the whole launch (own < F; the others only take part in the row phases).
// LDS: W transposed (s_wt[k * 64 + d]), Wfc with rows padded to 65 floats (one copy serves the lane = f reads of the forward and
// the lane = d reads of the backward, both conflict-free), the batch's x1 rows, h (overwritten in place by dh) and dr.
// Row phases: wave w owns the 4-row blocks w, w + 16, ...; lane = output channel; the row operand comes from the lanes of the wave
// itself (v_readlane of lane k), one fused multiply-add per term in ascending k.  A step is five phases, one barrier after each:
//   A  h, r of the wave's rows (the sign of r stays in a register), x1, h and r - t to LDS, the thread's part of the column sums
//   B  column sums over the 16 waves in wave order, sqrt, loss (wave 0, the wave butterfly), dr to LDS
//   D1 owners: dWfc = sum_b dr[b][f] h[b][4q ..] in ascending b, Adam on Wfc in registers (LDS keeps the old Wfc for phase C)
//   C  dh of the wave's rows from dr and the old Wfc, selected by h > 0, written over h
//   D2 owners: dW = sum_b dh[b][4q ..] x1[b][k] in ascending b, Adam on W, both new weights to LDS
// The ReLU backward selects (a zero column gives 0/0 behind a dropped element, and the element stays 0).  Every sum has a fixed
// order that does not depend on n_steps; no floating-point atomics, no tickets, no scratch.  The Adam update is k_adam_multi's
// (fullgraph.hip), expression for expression; the bias corrections of the launch's steps (at most 256: the host cuts a
// longer schedule into launches of 256) are formed in double side by side, one step per thread, before the weights are loaded.
//
// k_rm_scores: 256 threads, 128 rows per workgroup, the same forward block with both weights in static LDS; out[b] = sqrt(sum_c
// (r_bc - t_bc)^2) with the butterfly of k_recon_rows.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):  k_rm_steps  124 VGPRs, no scratch, dynamic LDS (the size of
// rm_lds_floats, at most 160 KiB - 512 B);  k_rm_scores  62 VGPRs, no scratch, 33,024 bytes of LDS.

#include "common.h"

#define RM_THREADS 1024
#define RM_WAVES (RM_THREADS / GGAD_WAVE)
#define RM_D 64                 // hidden channels
#define RM_MAX_F 64
#define RM_MAX_B 256
#define RM_RB 4                 // rows of a block: one LDS read of a weight serves four rows
#define RM_ITERS (RM_MAX_B / (RM_RB * RM_WAVES))      // row blocks per wave at most (4)
#define RM_FC_LD 65             // row stride of Wfc in LDS
#define RM_SC_STEPS 256         // steps of one launch (the table of bias corrections holds one entry per step)
#define RM_LDS_BYTES (160 * 1024 - 512)
#define RM_SCORE_ROWS 128       // rows per workgroup of k_rm_scores

static inline __host__ __device__ int rm_round4(int v) { return (v + 3) & ~3; }
static inline __host__ __device__ int rm_fixed_floats(int F) { return RM_D * F + rm_round4(RM_FC_LD * F) + RM_WAVES * 64 + 4 * RM_SC_STEPS; }
static inline __host__ __device__ int rm_lds_floats(int F, int rows) { return rm_fixed_floats(F) + rows * RM_D + 2 * rm_round4(rows * F); }

namespace {

__device__ __forceinline__ float rm_lane(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// h and r of the rows row0 .. row0 + nv - 1 (1 <= nv <= 4) of the tables; lane = channel.  xr / t: the lane's element of the x1 /
// target row (0 past F or past nv), h: relu(x1 W^T), r: relu(h Wfc^T) (0 in lanes >= F and rows >= nv).
__device__ __forceinline__ void rm_fwd_block(const float *__restrict__ x1, const float *__restrict__ tg, int64_t row0, int nv, int F,
                                             int lane, const float *s_wt, const float *s_wfc, float (&xr)[RM_RB], float (&t)[RM_RB],
                                             float (&h)[RM_RB], float (&r)[RM_RB]) {
  const bool col = lane < F;
  float a[RM_RB], rr[RM_RB];
#pragma unroll
  for (int j = 0; j < RM_RB; ++j) {
    const bool ok = col && j < nv;
    xr[j] = ok ? x1[(row0 + j) * F + lane] : 0.f;
    t[j] = ok ? tg[(row0 + j) * F + lane] : 0.f;
    a[j] = 0.f;
    rr[j] = 0.f;
  }
  for (int k = 0; k < F; ++k) {
    const float w = s_wt[k * RM_D + lane];
#pragma unroll
    for (int j = 0; j < RM_RB; ++j) a[j] = fmaf(rm_lane(xr[j], k), w, a[j]);
  }
#pragma unroll
  for (int j = 0; j < RM_RB; ++j) h[j] = a[j] < 0.f ? 0.f : a[j];
  const float *wf = s_wfc + (col ? lane : 0) * RM_FC_LD;
#pragma unroll 4
  for (int k = 0; k < RM_D; ++k) {
    const float w = wf[k];
#pragma unroll
    for (int j = 0; j < RM_RB; ++j) rr[j] = fmaf(rm_lane(h[j], k), w, rr[j]);
  }
#pragma unroll
  for (int j = 0; j < RM_RB; ++j) r[j] = (col && j < nv) ? (rr[j] < 0.f ? 0.f : rr[j]) : 0.f;
}

__global__ __launch_bounds__(RM_THREADS) void k_rm_steps(const float *__restrict__ x1, const float *__restrict__ tg,
                                                          const int32_t *__restrict__ batch_ptr, int n_steps, int total_rows,
                                                          int max_rows, int F, float *__restrict__ W, float *__restrict__ Wfc,
                                                          float *__restrict__ mW, float *__restrict__ vW, float *__restrict__ mF,
                                                          float *__restrict__ vF, int32_t *__restrict__ ctrW,
                                                          int32_t *__restrict__ ctrF, float lr, float wd, float w_pos, float w_neg,
                                                          float *__restrict__ losses, float *__restrict__ gW, float *__restrict__ gF) {
  extern __shared__ float4 rm_lds4[];
  float *s_wt = reinterpret_cast<float *>(rm_lds4);          // [k * 64 + d] = W[d][k]
  float *s_wfc = s_wt + RM_D * F;                            // [f * 65 + d] = Wfc[f][d]
  float *s_red = s_wfc + rm_round4(RM_FC_LD * F);            // [wave * 64 + f]
  float *s_sc = s_red + RM_WAVES * 64;                       // [4][RM_SC_STEPS]: lr / (1 - .9^t), sqrt(1 - .999^t) of W, then of Wfc
  float *s_h = s_sc + 4 * RM_SC_STEPS;                       // [b * 64 + d]: h, then dh
  float *s_dr = s_h + max_rows * RM_D;                       // [b * F + f]
  float *s_x = s_dr + rm_round4(max_rows * F);               // [b * F + k]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q4 = (tid & 15) * 4, own = tid >> 4;
  const bool owner = own < F, col = lane < F;

  const int c0w = *ctrW, c0f = *ctrF;
  {      // the bias corrections of the launch's steps, formed in double as k_adam_multi forms them: one step per thread and table
    const int k = tid & (RM_SC_STEPS - 1), which = tid >> 8;      // which: wave-uniform
    if (k < n_steps) {
      const double t = (double)((which < 2 ? c0w : c0f) + k + 1);
      s_sc[which * RM_SC_STEPS + k] = (which & 1) ? (float)sqrt(1.0 - pow(0.999, t)) : (float)((double)lr / (1.0 - pow(0.9, t)));
    }
  }
  float pw[4], mw[4], vw[4], pf[4], mf[4], vf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int iw = (q4 + j) * F + own, ifc = own * RM_D + q4 + j;
    pw[j] = owner ? W[iw] : 0.f;   mw[j] = owner ? mW[iw] : 0.f;   vw[j] = owner ? vW[iw] : 0.f;
    pf[j] = owner ? Wfc[ifc] : 0.f; mf[j] = owner ? mF[ifc] : 0.f; vf[j] = owner ? vF[ifc] : 0.f;
  }
  if (owner) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s_wt[own * RM_D + q4 + j] = pw[j];
      s_wfc[own * RM_FC_LD + q4 + j] = pf[j];
    }
  }
  const float inv_cols = 1.f / (float)F;
  int done = 0;
  __syncthreads();

  for (int s = 0; s < n_steps; ++s) {
    const int r0 = batch_ptr[s], B = batch_ptr[s + 1] - r0;
    if (!(r0 >= 0 && B >= 1 && B <= max_rows && r0 <= total_rows - B)) {      // workgroup-uniform: a batch outside the tables is no step
      if (tid == 0) losses[s] = __int_as_float(0x7fc00000);
      continue;
    }
    // ---- A: forward of the wave's rows
    unsigned pos = 0u;      // which of the thread's elements have r > 0 (bit it * 4 + j); r - t waits in s_dr
    float cs = 0.f;
#pragma unroll 1
    for (int it = 0; it < RM_ITERS; ++it) {
      const int base = (it * RM_WAVES + wave) * RM_RB;
      if (base >= B) break;
      const int nv = B - base < RM_RB ? B - base : RM_RB;
      float xr[RM_RB], t[RM_RB], h[RM_RB], r[RM_RB];
      rm_fwd_block(x1, tg, (int64_t)r0 + base, nv, F, lane, s_wt, s_wfc, xr, t, h, r);
#pragma unroll
      for (int j = 0; j < RM_RB; ++j) {
        if (j < nv) {
          s_h[(base + j) * RM_D + lane] = h[j];
          if (col) {
            s_x[(base + j) * F + lane] = xr[j];
            const float av = r[j], d = av - t[j];
            cs += (d * d) * (av > 0.f ? w_pos : w_neg);
            s_dr[(base + j) * F + lane] = d;
            pos |= (av > 0.f ? 1u : 0u) << (it * RM_RB + j);
          }
        }
      }
    }
    s_red[wave * 64 + lane] = cs;
    __syncthreads();

    // ---- B: column sums, loss, dr (over the thread's own r - t)
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < RM_WAVES; ++w) tot += s_red[w * 64 + lane];
    const float sq = sqrtf(tot);
    if (wave == 0) {
      const float acc = wave_sum(col ? sq : 0.f);
      if (lane == 0) losses[s] = acc / (float)F;
    }
    if (col) {
#pragma unroll 1
      for (int it = 0; it < RM_ITERS; ++it) {
        const int base = (it * RM_WAVES + wave) * RM_RB;
        if (base >= B) break;
#pragma unroll
        for (int j = 0; j < RM_RB; ++j) {
          if (base + j < B) {      // r > 0 takes w_pos; the ReLU backward drops the others (0, not 0 * (0 / 0))
            float *dp = s_dr + (base + j) * F + lane;
            const float g = (w_pos * *dp / sq) * inv_cols;
            *dp = ((pos >> (it * RM_RB + j)) & 1u) ? g : 0.f;
          }
        }
      }
    }
    __syncthreads();

    const int sc_i = done & (RM_SC_STEPS - 1);
    const bool last = s == n_steps - 1;
    // ---- D1: dWfc and Adam on Wfc (registers only)
    if (owner) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int b = 0; b < B; ++b) {
        const float dv = s_dr[b * F + own];
        const float4 hv = *reinterpret_cast<const float4 *>(s_h + b * RM_D + q4);
        acc[0] = fmaf(dv, hv.x, acc[0]); acc[1] = fmaf(dv, hv.y, acc[1]);
        acc[2] = fmaf(dv, hv.z, acc[2]); acc[3] = fmaf(dv, hv.w, acc[3]);
      }
      const float sc0 = s_sc[2 * RM_SC_STEPS + sc_i], sc1 = s_sc[3 * RM_SC_STEPS + sc_i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (last && gF) gF[own * RM_D + q4 + j] = acc[j];
        ggad_adam_elem(pf[j], mf[j], vf[j], acc[j], wd, sc0, sc1);
      }
    }
    __syncthreads();

    // ---- C: dh of the wave's rows over h
#pragma unroll 1
    for (int it = 0; it < RM_ITERS; ++it) {
      const int base = (it * RM_WAVES + wave) * RM_RB;
      if (base >= B) break;
      {
        float dv[RM_RB], a[RM_RB];
#pragma unroll
        for (int j = 0; j < RM_RB; ++j) {
          dv[j] = (col && base + j < B) ? s_dr[(base + j) * F + lane] : 0.f;
          a[j] = 0.f;
        }
        for (int k = 0; k < F; ++k) {
          const float w = s_wfc[k * RM_FC_LD + lane];
#pragma unroll
          for (int j = 0; j < RM_RB; ++j) a[j] = fmaf(rm_lane(dv[j], k), w, a[j]);
        }
#pragma unroll
        for (int j = 0; j < RM_RB; ++j) {
          if (base + j < B) {
            float *hp = s_h + (base + j) * RM_D + lane;
            *hp = *hp > 0.f ? a[j] : 0.f;
          }
        }
      }
    }
    __syncthreads();

    // ---- D2: dW, Adam on W, the new weights to LDS
    if (owner) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int b = 0; b < B; ++b) {
        const float xv = s_x[b * F + own];
        const float4 dh = *reinterpret_cast<const float4 *>(s_h + b * RM_D + q4);
        acc[0] = fmaf(dh.x, xv, acc[0]); acc[1] = fmaf(dh.y, xv, acc[1]);
        acc[2] = fmaf(dh.z, xv, acc[2]); acc[3] = fmaf(dh.w, xv, acc[3]);
      }
      const float sc0 = s_sc[sc_i], sc1 = s_sc[RM_SC_STEPS + sc_i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (last && gW) gW[(q4 + j) * F + own] = acc[j];
        ggad_adam_elem(pw[j], mw[j], vw[j], acc[j], wd, sc0, sc1);
        s_wt[own * RM_D + q4 + j] = pw[j];
        s_wfc[own * RM_FC_LD + q4 + j] = pf[j];
      }
    }
    ++done;
    __syncthreads();
  }

  if (owner) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int iw = (q4 + j) * F + own, ifc = own * RM_D + q4 + j;
      W[iw] = pw[j];   mW[iw] = mw[j];  vW[iw] = vw[j];
      Wfc[ifc] = pf[j]; mF[ifc] = mf[j]; vF[ifc] = vf[j];
    }
  }
  if (tid == 0) {
    *ctrW = c0w + done;
    *ctrF = c0f + done;
  }
}

__global__ __launch_bounds__(256) void k_rm_scores(const float *__restrict__ x1, const float *__restrict__ tg, int64_t n_rows, int F,
                                                   const float *__restrict__ W, const float *__restrict__ Wfc,
                                                   float *__restrict__ out) {
  __shared__ float s_wt[RM_MAX_F * RM_D];
  __shared__ float s_wfc[RM_MAX_F * RM_FC_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int o = tid; o < RM_D * F; o += 256) {
    const int c = o / F, k = o - c * F;
    s_wt[k * RM_D + c] = W[o];
  }
  for (int o = tid; o < F * RM_D; o += 256) s_wfc[(o >> 6) * RM_FC_LD + (o & 63)] = Wfc[o];
  __syncthreads();
  const int64_t wg0 = (int64_t)blockIdx.x * RM_SCORE_ROWS;
  for (int blk = wave; blk < RM_SCORE_ROWS / RM_RB; blk += 4) {
    const int64_t row0 = wg0 + (int64_t)blk * RM_RB;
    if (row0 >= n_rows) break;
    const int nv = n_rows - row0 < RM_RB ? (int)(n_rows - row0) : RM_RB;
    float xr[RM_RB], t[RM_RB], h[RM_RB], r[RM_RB];
    rm_fwd_block(x1, tg, row0, nv, F, lane, s_wt, s_wfc, xr, t, h, r);
#pragma unroll
    for (int j = 0; j < RM_RB; ++j) {
      const float d = r[j] - t[j];
      const float sum = wave_sum(d * d);
      if (lane == 0 && j < nv) out[row0 + j] = sqrtf(sum);
    }
  }
}

}  // namespace

extern "C" {

int32_t ggad_recon_mb_max_rows(int32_t feat_dim) {
  if (feat_dim < 1 || feat_dim > RM_MAX_F) return 0;
  const int cap = (RM_LDS_BYTES / 4 - rm_fixed_floats(feat_dim) - 8) / (RM_D + 2 * feat_dim);      // (8: the two round-ups to 4 floats)
  return cap < RM_MAX_B ? cap : RM_MAX_B;
}

int32_t ggad_recon_mb_supported(int32_t feat_dim, int32_t embed_dim, int32_t max_rows) {
  return feat_dim >= 1 && feat_dim <= RM_MAX_F && embed_dim == RM_D && max_rows >= 1 && max_rows <= ggad_recon_mb_max_rows(feat_dim);
}

int ggad_recon_mb_steps_f32(const float *x1, const float *target, const int32_t *batch_ptr, int32_t n_steps, int32_t total_rows,
                            int32_t max_rows, int32_t feat_dim, int32_t embed_dim, float *w_enc, float *w_fc, float *m_enc, float *v_enc,
                            float *m_fc, float *v_fc, int32_t *ctr_enc, int32_t *ctr_fc, float lr, float weight_decay, float w_pos,
                            float w_neg, float *losses, float *g_enc, float *g_fc, ggad_stream_t stream) {
  GGAD_REQUIRE(x1 && target && batch_ptr && w_enc && w_fc && m_enc && v_enc && m_fc && v_fc && ctr_enc && ctr_fc && losses);
  GGAD_REQUIRE(n_steps >= 1 && total_rows >= 1);
  GGAD_REQUIRE(ggad_recon_mb_supported(feat_dim, embed_dim, max_rows));
  GGAD_REQUIRE((int64_t)total_rows * feat_dim < (1ll << 31));
  const size_t lds = (size_t)rm_lds_floats(feat_dim, max_rows) * sizeof(float);
  GGAD_REQUIRE(lds <= (size_t)RM_LDS_BYTES);
  static ggad_lds_optin lds_optin;
  const int ready = ggad_lds_opt_in(lds_optin, RM_LDS_BYTES, k_rm_steps);
  if (ready == 0) return GGAD_E_INVALID;
  if (ready != 1) { ggad_set_error(hipErrorInvalidValue, "recon_mb_steps: this device cannot give k_rm_steps its LDS"); return GGAD_E_LAUNCH; }
  for (int32_t s0 = 0; s0 < n_steps; s0 += RM_SC_STEPS) {      // an epoch of the handlers (150 or 50 steps) is one launch
    const int32_t n = n_steps - s0 < RM_SC_STEPS ? n_steps - s0 : RM_SC_STEPS;
    const bool tail = s0 + n == n_steps;
    k_rm_steps<<<dim3(1), dim3(RM_THREADS), lds, as_stream(stream)>>>(x1, target, batch_ptr + s0, n, total_rows, max_rows, feat_dim, w_enc,
                                                                    w_fc, m_enc, v_enc, m_fc, v_fc, ctr_enc, ctr_fc, lr, weight_decay,
                                                                    w_pos, w_neg, losses + s0, tail ? g_enc : nullptr,
                                                                    tail ? g_fc : nullptr);
  }
  GGAD_CHECK_LAUNCH("recon_mb_steps");
  return GGAD_OK;
}

int ggad_recon_mb_scores_f32(const float *x1, const float *target, int64_t n_rows, int32_t feat_dim, int32_t embed_dim, const float *w_enc,
                             const float *w_fc, float *out, ggad_stream_t stream) {
  GGAD_REQUIRE(x1 && target && w_enc && w_fc && out && n_rows >= 0);
  GGAD_REQUIRE(feat_dim >= 1 && feat_dim <= RM_MAX_F && embed_dim == RM_D);
  if (n_rows == 0) return GGAD_OK;
  const int64_t blocks = (n_rows + RM_SCORE_ROWS - 1) / RM_SCORE_ROWS;
  GGAD_REQUIRE(blocks < (1ll << 31));
  k_rm_scores<<<dim3((unsigned)blocks), dim3(256), 0, as_stream(stream)>>>(x1, target, n_rows, feat_dim, w_enc, w_fc, out);
  GGAD_CHECK_LAUNCH("recon_mb_scores");
  return GGAD_OK;
}

}  // extern "C"
