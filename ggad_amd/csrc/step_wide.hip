// Wide variant of the layered step chain of step.hip (gfx950): the same stages
//
//   project -> fwd_rows -> loss_pos -> loss_rows -> bwd_flat -> grad_reduce [+ Adam | + exchange + Adam]
//   row_coefs, score, encode
//
// for embedding widths 64 < D <= 256 (and, as `chain = 3`, for any D <= 256: that is how the tests pin these kernels
// to the vectors the D <= 64 kernels are pinned to).  Reference ops: GCNEncoder.forward + GCN.loss
// (src/graphsage.py:395-454, 171-258), their backward and Adam (src/model_handler.py:363-364).
//
// Layout.  A lane owns the channels d = lane + 64 j, j < NJ = ceil(D / 64) <= 4 (template parameter): a D-float row is
// read as NJ consecutive 256-byte coalesced segments, and a reduction over channels is a fixed-order per-lane partial
// over j followed by the wave reduction of step_common.h.  No float atomics, every sum in a fixed order (reruns give
// the same bits), row and index loads broadcast with v_readlane, project / bwd_flat flat over entries.
//
// What does not fit where it fits at D = 64 (160 KB of LDS and 512 VGPRs per lane at one wave per SIMD):
//   * fc / fc^T is D*D floats = 256 KB at D = 256: never staged in LDS; both matrix-vector products (gen = relu(fc nbar),
//     fc^T dz) read it through L2 with d as the contiguous index, the D-long sum split over the waves of the workgroup
//     and combined in LDS in wave order.
//   * W^T columns in registers would cost F * NJ VGPRs (68 at F = 17, 512 at F = 128) and an LDS copy F * D floats
//     (128 KB at F = 128, D = 256, filled by every workgroup for a handful of rows).  Instead a wave projects 8 rows at
//     once: W^T[f][.] is loaded once per f (NJ coalesced loads, L1/L2 hits: all waves walk the same F * D block) and
//     used for the 8 rows, whose features come through the scalar cache.  F is a run-time value; no F-sized storage.
//   * bwd_flat accumulates dW for a tile of 17 features (NJ * 17 accumulators per lane); wider F takes more tiles in
//     gridDim.y.  The four waves of a workgroup are combined through ONE [17][NJ * 64] LDS block in wave order.
//   * d fc is D * D outputs, each a sum over the label-1 rows: the same thread-per-output reduction as at D = 64, on
//     (D * D + 63) / 64 workgroups.
#include "common.h"
#include "step_common.h"

namespace {

constexpr int WIDE_MAX_D = 256;

template <int NJ>
struct Chan {                     // the NJ channels of this lane; d[] is clamped into the row for loads, on[] guards stores
  int d[NJ];
  bool on[NJ];
  __device__ __forceinline__ Chan(int lane, int D) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      on[j] = c < D;
      d[j] = on[j] ? c : D - 1;
    }
  }
};

// acc[i][j] = sum_f W^T[f][d_j] * x_i[f] for R wave-uniform feature rows (f ascending, fma from 0: the order of step.hip)
template <int NJ, int R, typename Rows>
__device__ __forceinline__ void dot_rows(const float *__restrict__ Wt, int D, int F, const Chan<NJ> &ch, const Rows &xr,
                                         float (&acc)[R][NJ]) {
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = 0.0f;
  for (int f = 0; f < F; ++f) {
    float w[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) w[j] = Wt[(int64_t)f * D + ch.d[j]];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float x = xr[i][f];
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = fmaf(w[j], x, acc[i][j]);
    }
  }
}

// ------------------------------------------------------------------ project: h2 at owner entries (flat over entries)
constexpr int WP_EPW = 8;   // entries per wave
template <int NJ>
__global__ void __launch_bounds__(256) k_project_w(const float *__restrict__ params, ParamLayout L, const float *__restrict__ x2,
                                                   const int32_t *__restrict__ ent_own, int ent0, int n_ents,
                                                   float *__restrict__ h2) {
  const int D = L.D, F = L.F;
  const int lane = lane_id(), wid = threadIdx.x / 64;
  const Chan<NJ> ch(lane, D);
  const int base = (blockIdx.x * 4 + wid) * WP_EPW;
  if (base >= n_ents) return;
  const int ov = (lane < WP_EPW && base + lane < n_ents) ? ent_own[ent0 + base + lane] : -1;
  const float *xr[WP_EPW];
  bool own[WP_EPW];
  bool any = false;
#pragma unroll
  for (int i = 0; i < WP_EPW; ++i) {
    const int o = __builtin_amdgcn_readlane(ov, i);
    own[i] = o == ent0 + base + i;                        // not an owner (or past the end): computed on a valid row, not stored
    any = any || own[i];
    xr[i] = x2 + (int64_t)(own[i] ? o : ent0 + base) * F;
  }
  if (!any) return;                                       // wave-uniform
  float acc[WP_EPW][NJ];
  dot_rows<NJ, WP_EPW>(params + L.o_Wt(), D, F, ch, xr, acc);
#pragma unroll
  for (int i = 0; i < WP_EPW; ++i) {
    if (!own[i]) continue;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (ch.on[j]) h2[(int64_t)(base + i) * D + ch.d[j]] = fmaxf(acc[i][j], 0.0f);      // relu(W x2[u])   graphsage.py:419
  }
}

// ------------------------------------------------------------------ forward rows (16 waves per row)
constexpr int WF_NW = 16;
template <int NJ>
__global__ void __launch_bounds__(WF_NW * 64) k_fwd_rows_w(const float *__restrict__ params, ParamLayout L,
                                                           const float *__restrict__ x1, const float *__restrict__ h2,
                                                           const int32_t *__restrict__ ent_ptr, const int32_t *__restrict__ ent_own,
                                                           const int32_t *__restrict__ labels, int row0, int ent0,
                                                           float *__restrict__ h1, float *__restrict__ nbar, float *__restrict__ gen) {
  constexpr int DP = NJ * 64;
  __shared__ float part[WF_NW][DP];
  __shared__ float ns[DP];
  const int D = L.D, F = L.F;
  const int lane = lane_id(), wid = threadIdx.x / 64;
  const Chan<NJ> ch(lane, D);
  const int row = row0 + blockIdx.x;
  const int e0 = ent_ptr[row], e1 = ent_ptr[row + 1];
  const int r = e1 - e0;
  // partial sum of h2[own(e)] over e = e0 + wid, e0 + wid + NW, ...  (NJ 256-byte coalesced loads per entry)
  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.0f;
  for (int blk = wid; blk < r; blk += WF_NW * 64) {
    const int my = blk + WF_NW * lane;
    const int ov = (my < r) ? ent_own[e0 + my] : 0;
    const int cnt = min(64, (r - blk + WF_NW - 1) / WF_NW);
    int i = 0;
    for (; i + 4 <= cnt; i += 4) {                       // hub rows: 4 NJ row loads in flight per wave (same summation order)
      float a[4][NJ];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t o = (int64_t)(__builtin_amdgcn_readlane(ov, i + q) - ent0) * D;
#pragma unroll
        for (int j = 0; j < NJ; ++j) a[q][j] = h2[o + ch.d[j]];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] += a[q][j];
    }
    for (; i < cnt; ++i) {
      const int64_t o = (int64_t)(__builtin_amdgcn_readlane(ov, i) - ent0) * D;
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] += h2[o + ch.d[j]];
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) part[wid][lane + 64 * j] = acc[j];
  __syncthreads();
  const float inv_r = 1.0f / (float)r;                                      // mask_row = mask / rowsum  graphsage.py:317
  const int y = labels[row];
  if (wid == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float tot = 0.0f;
#pragma unroll
      for (int k = 0; k < WF_NW; ++k) tot += part[k][lane + 64 * j];        // fixed order
      const float nb = inv_r * tot;
      if (ch.on[j]) nbar[(int64_t)row * D + ch.d[j]] = nb;                  // mask_row.mm(...)          graphsage.py:421
      ns[lane + 64 * j] = ch.on[j] ? nb : 0.0f;
    }
  }
  if (wid == 1) {                                                           // h1 = relu(W x1[row])      graphsage.py:412
    const float *xr[1] = {x1 + (int64_t)row * F};
    float h[1][NJ];
    dot_rows<NJ, 1>(params + L.o_Wt(), D, F, ch, xr, h);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (ch.on[j]) h1[(int64_t)row * D + ch.d[j]] = fmaxf(h[0][j], 0.0f);
  }
  if (y != 1) return;                                                       // block-uniform exit
  __syncthreads();
  // outlier generation gen = relu(fc nbar): the waves split the d2 range; fc^T through L2, d contiguous   graphsage.py:428-430
  const float *fcT = params + L.o_fcT();
  const int q = (D + WF_NW - 1) / WF_NW;
  float a[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) a[j] = 0.0f;
  for (int d2 = wid * q; d2 < min(D, (wid + 1) * q); ++d2) {
    const float nv = ns[d2];
#pragma unroll
    for (int j = 0; j < NJ; ++j) a[j] = fmaf(fcT[(int64_t)d2 * D + ch.d[j]], nv, a[j]);
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) part[wid][lane + 64 * j] = a[j];             // (every wave is past its reads of part: barrier above)
  __syncthreads();
  if (wid == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float g = 0.0f;
#pragma unroll
      for (int k = 0; k < WF_NW; ++k) g += part[k][lane + 64 * j];
      if (ch.on[j]) gen[(int64_t)row * D + ch.d[j]] = fmaxf(g, 0.0f);
    }
  }
}

// ------------------------------------------------------------------ loss: one wave per position, then one wave per row
template <int NJ>
__device__ __forceinline__ PosVals eval_position_w(const float (&wd)[NJ], const float (&c)[NJ], const float (&nb)[NJ]) {
  float ps = 0.0f, pa = 0.0f, pb = 0.0f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    ps = fmaf(wd[j], c[j], ps);
    pa = fmaf(c[j], c[j], pa);
    pb = fmaf(nb[j], nb[j], pb);
  }
  PosVals v;
  v.s = wave_sum_fast(ps);                                              // scores = weight.mm(embeds)  graphsage.py:174
  v.na = sqrtf(wave_sum_fast(pa));
  v.nbn = sqrtf(wave_sum_fast(pb));
  v.nac = fmaxf(v.na, 1e-8f);                                           // cosine_similarity eps      graphsage.py:234
  v.nbc = fmaxf(v.nbn, 1e-8f);
  float pf = 0.0f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) pf = fmaf(c[j] / v.nac, nb[j] / v.nbc, pf);
  v.aff = wave_sum_fast(pf);
  return v;
}

template <int NJ>
__global__ void __launch_bounds__(256) k_loss_pos_w(const float *__restrict__ params, int D, const float *__restrict__ h1,
                                                    const float *__restrict__ nbar, const float *__restrict__ gen,
                                                    const int32_t *__restrict__ pos_meta, int row0, int B,
                                                    float *__restrict__ pos_scal, float *__restrict__ part) {
  __shared__ float red[4][8];
  const int lane = lane_id(), wid = threadIdx.x / 64;
  const Chan<NJ> ch(lane, D);
  const int q = blockIdx.x * 4 + wid;
  float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (q < B) {
    const int meta = pos_meta[row0 + q];
    const int src = meta >> 2, y = meta & 1;
    const bool from_gen = (meta & 2) != 0;
    float wd[NJ], c[NJ], nb[NJ];
    float pr = 0.0f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int64_t so = (int64_t)src * D + ch.d[j];
      const float hv = h1[so];
      const float cv = from_gen ? gen[so] : hv;                                  // combined_all[:, q]
      wd[j] = ch.on[j] ? params[ch.d[j]] : 0.0f;
      c[j] = ch.on[j] ? cv : 0.0f;
      nb[j] = ch.on[j] ? nbar[(int64_t)(row0 + q) * D + ch.d[j]] : 0.0f;         // to_feats_neigh[q, :]
      const float dl = (ch.on[j] && from_gen) ? hv - cv : 0.0f;
      pr = fmaf(dl, dl, pr);
    }
    const PosVals v = eval_position_w<NJ>(wd, c, nb);
    float recn = 0.0f;
    if (from_gen) recn = sqrtf(wave_sum_fast(pr));                       // recon2   graphsage.py:197-198
    o[0] = (1.0f - (float)y) * v.s - log_sigmoid(v.s);                   // BCEWithLogits, pos_weight 1 graphsage.py:246
    o[1] = y == 0 ? v.aff : 0.0f; o[2] = y == 1 ? v.aff : 0.0f; o[3] = recn;
    o[4] = y == 0 ? 1.0f : 0.0f;  o[5] = y == 1 ? 1.0f : 0.0f;
    if (lane == 0) {
      float *ps = pos_scal + (int64_t)q * 8;
      ps[0] = v.s; ps[1] = v.aff; ps[2] = v.na; ps[3] = v.nbn; ps[4] = recn;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[wid][k] = o[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    part[(int64_t)blockIdx.x * 8 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// fc^T dz for the (up to) four rows of a workgroup: zs[r][dd] holds dz of row r (zero for a row without one).  Wave w
// sums dd over its quarter of [0, D) for all four rows (fc read once per workgroup, through L2, d contiguous), the
// quarters are combined in wave order.  Returns this wave's row (row wid) in out[].  Block-uniform call.
template <int NJ>
__device__ __forceinline__ void fct_dz(const float *__restrict__ fc, int D, const Chan<NJ> &ch, int lane, int wid,
                                       const float (*zs)[NJ * 64], float (*mv)[4][NJ * 64], float (&out)[NJ]) {
  const int q = (D + 3) / 4;
  float a[4][NJ];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < NJ; ++j) a[r][j] = 0.0f;
#pragma unroll 4
  for (int dd = wid * q; dd < min(D, (wid + 1) * q); ++dd) {
    float f[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) f[j] = fc[(int64_t)dd * D + ch.d[j]];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = zs[r][dd];
#pragma unroll
      for (int j = 0; j < NJ; ++j) a[r][j] = fmaf(f[j], z, a[r][j]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < NJ; ++j) mv[wid][r][lane + 64 * j] = a[r][j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    out[j] = (mv[0][wid][c] + mv[1][wid][c]) + (mv[2][wid][c] + mv[3][wid][c]);
  }
}

template <int NJ>
__global__ void __launch_bounds__(256) k_loss_rows_w(const float *__restrict__ params, ParamLayout L,
                                                     const float *__restrict__ h1, const float *__restrict__ nbar,
                                                     const float *__restrict__ gen, const int32_t *__restrict__ labels,
                                                     const int32_t *__restrict__ pos_meta, const int32_t *__restrict__ row_pos,
                                                     const int32_t *__restrict__ ent_ptr, int row0, int B,
                                                     const float *__restrict__ pos_scal, const float *__restrict__ part,
                                                     float *__restrict__ gw_part, float *__restrict__ losses8,
                                                     float *__restrict__ d_h1, float *__restrict__ d_gen,
                                                     float *__restrict__ d_nbar, float *__restrict__ dz,
                                                     float *__restrict__ coef_a, float *__restrict__ coef_g,
                                                     int32_t *__restrict__ step_counter) {
  constexpr int DP = NJ * 64;
  __shared__ float gw[4][DP];
  __shared__ float zs[4][DP];
  __shared__ float mv[4][4][DP];
  const int D = L.D;
  const int lane = lane_id(), wid = threadIdx.x / 64;
  const Chan<NJ> ch(lane, D);
  // every wave reduces the per-workgroup partials the same way -> identical scalars everywhere
  const int nwg = loss_nwg(B);
  float t[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    float v = 0.0f;
    for (int g = lane; g < nwg; g += 64) v += part[(int64_t)g * 8 + k];
    t[k] = wave_sum_fast(v);
  }
  const float fB = (float)B;
  const float cls = t[0] / fB;
  const float an = t[1] / t[4], ab = t[2] / t[5];
  const float mg = 1.0f - (an - ab);                                     // confidence_margin = 1      graphsage.py:236-240
  const float active = (mg >= 0.0f) ? 1.0f : 0.0f;                       // clamp_min backward: pass where x >= min
  const float rec_coef = 0.1f / t[5];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float margin = fmaxf(mg, 0.0f), rec = t[3] / t[5];
    losses8[0] = cls + margin + 0.1f * rec;                              // graphsage.py:258
    losses8[1] = cls; losses8[2] = margin; losses8[3] = rec;
    losses8[4] = rec_coef; losses8[5] = active; losses8[6] = t[4]; losses8[7] = t[5];
    if (step_counter) *step_counter += 1;
  }
  const int i = blockIdx.x * 4 + wid;
  const int row = row0 + min(i, B - 1);
  const int y = (i < B) ? labels[row] : 0;
  const int r = ent_ptr[row + 1] - ent_ptr[row];
  bool any1 = false;                                                     // block-uniform: a label-1 row among the four
#pragma unroll
  for (int k = 0; k < 4; ++k) any1 = any1 || (blockIdx.x * 4 + k < B && labels[row0 + blockIdx.x * 4 + k] == 1);
  float gwd[NJ], dNb[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) { gwd[j] = 0.0f; dNb[j] = 0.0f; zs[wid][lane + 64 * j] = 0.0f; }
  if (i < B) {
    // ---- C-side: this row is the source of column q1
    const int q1 = row_pos[row];
    const float *p1 = pos_scal + (int64_t)q1 * 8;
    const float s1 = p1[0], aff1 = p1[1], na1 = p1[2], nbn1 = p1[3], recn = p1[4];
    const int y1 = pos_meta[row0 + q1] & 1;
    const float nac1 = fmaxf(na1, 1e-8f), nbc1 = fmaxf(nbn1, 1e-8f);
    const float ds = (1.0f / (1.0f + expf(-s1)) - (float)y1) / fB;
    const float gq1 = active * (y1 == 0 ? -1.0f / t[4] : 1.0f / t[5]);
    // ---- nb-side: position i pairs nbar[row] with column i of combined_all
    const float *p2 = pos_scal + (int64_t)i * 8;
    const float aff2 = p2[1], na2 = p2[2], nbn2 = p2[3];
    const int m2 = pos_meta[row0 + i];
    const int src2 = m2 >> 2;
    const float nac2 = fmaxf(na2, 1e-8f), nbc2 = fmaxf(nbn2, 1e-8f);
    const float gq2 = active * (y == 0 ? -1.0f / t[4] : 1.0f / t[5]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const float wd = ch.on[j] ? params[ch.d[j]] : 0.0f;
      const int64_t off = (int64_t)row * D + ch.d[j];
      const float H1 = h1[off];
      const float NB = nbar[off];
      const float G = (y == 1) ? gen[off] : 0.0f;
      const float C = (y == 1) ? G : H1;                                 // this row's column of combined_all
      const float nbq = nbar[(int64_t)(row0 + q1) * D + ch.d[j]];
      // aff = sum (c/nac)(nb/nbc); torch clamps a detached copy of the norms, so autograd sees
      // d aff / d c = (nb/nbc)/nac - (aff/nac) * c/|c|   (and symmetrically for nb)
      const float ca = na1 > 0.0f ? C / na1 : 0.0f;
      const float dC = ds * wd + gq1 * ((nbq / nbc1) / nac1 - (aff1 / nac1) * ca);
      float gH = dC, gG = 0.0f;
      if (y == 1) {                                                      // recon term 0.1 * mean_i |h1_i - gen_i|  graphsage.py:258
        const float tt = rec_coef * ((H1 - G) / recn);
        gH = tt; gG = dC - tt;
      }
      gwd[j] = ch.on[j] ? ds * C : 0.0f;
      const int64_t so = (int64_t)src2 * D + ch.d[j];
      const float c2 = (m2 & 2) ? gen[so] : h1[so];
      const float cb = nbn2 > 0.0f ? NB / nbn2 : 0.0f;
      dNb[j] = gq2 * ((c2 / nac2) / nbc2 - (aff2 / nbc2) * cb);
      if (d_h1 != nullptr && ch.on[j]) { d_h1[off] = gH; d_gen[off] = gG; d_nbar[off] = dNb[j]; }
      // ---- backward coefficients of this row
      if (ch.on[j]) coef_a[off] = (H1 > 0.0f) ? gH : 0.0f;
      if (y == 1) {
        const float dZ = (G > 0.0f) ? gG : 0.0f;                         // relu(fc(.))
        if (ch.on[j]) { dz[off] = dZ; zs[wid][lane + 64 * j] = dZ; }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) gw[wid][lane + 64 * j] = gwd[j];
  __syncthreads();
  if (any1) {
    float a[NJ];
    fct_dz<NJ>(params + L.o_fc(), D, ch, lane, wid, zs, mv, a);
    if (y == 1) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) dNb[j] += a[j];                       // fc^T dZ
    }
  }
  if (i < B) {
    const float inv_r = 1.0f / (float)r;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (ch.on[j]) coef_g[(int64_t)row * D + ch.d[j]] = dNb[j] * inv_r;
  }
  for (int c = threadIdx.x; c < DP; c += 256)
    gw_part[(int64_t)blockIdx.x * DP + c] = (gw[0][c] + gw[1][c]) + (gw[2][c] + gw[3][c]);
}

// stand-alone VJP front end (layered autograd API): upstream gradients given by the caller
//   coef_a = d_h1 * [h1 > 0];  dz = d_gen * [gen > 0] (label-1 rows);  coef_g = (d_nbar + fc^T dz) / r
template <int NJ>
__global__ void __launch_bounds__(256) k_row_coefs_w(const float *__restrict__ params, ParamLayout L,
                                                     const int32_t *__restrict__ labels, const int32_t *__restrict__ ent_ptr,
                                                     int row0, int B, const float *__restrict__ h1, const float *__restrict__ gen,
                                                     const float *__restrict__ d_h1, const float *__restrict__ d_gen,
                                                     const float *__restrict__ d_nbar, float *__restrict__ dz,
                                                     float *__restrict__ coef_a, float *__restrict__ coef_g) {
  constexpr int DP = NJ * 64;
  __shared__ float zs[4][DP];
  __shared__ float mv[4][4][DP];
  const int D = L.D;
  const int lane = lane_id(), wid = threadIdx.x / 64;
  const Chan<NJ> ch(lane, D);
  const int i = blockIdx.x * 4 + wid;
  const int row = row0 + min(i, B - 1);
  const int y = (i < B) ? labels[row] : 0;
  const int r = ent_ptr[row + 1] - ent_ptr[row];
  bool any1 = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) any1 = any1 || (blockIdx.x * 4 + k < B && labels[row0 + blockIdx.x * 4 + k] == 1);
  float dNb[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int64_t off = (int64_t)row * D + ch.d[j];
    dNb[j] = d_nbar[off];
    float dZ = 0.0f;
    if (i < B && ch.on[j]) {
      coef_a[off] = (h1[off] > 0.0f) ? d_h1[off] : 0.0f;
      if (y == 1) {
        dZ = (gen[off] > 0.0f) ? d_gen[off] : 0.0f;                      // relu(fc(.))
        dz[off] = dZ;
      }
    }
    zs[wid][lane + 64 * j] = dZ;
  }
  __syncthreads();
  if (any1) {
    float a[NJ];
    fct_dz<NJ>(params + L.o_fc(), D, ch, lane, wid, zs, mv, a);
    if (y == 1) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) dNb[j] += a[j];
    }
  }
  if (i < B) {
    const float inv_r = 1.0f / (float)r;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (ch.on[j]) coef_g[(int64_t)row * D + ch.d[j]] = dNb[j] * inv_r;
  }
}

// ------------------------------------------------------------------ backward, flat over entries + rows
// work item idx < n_ents : entry e = ent0 + idx :  coef = coef_g[row(e)] * [h2[own(e)] > 0],  x = x2[own(e)]
//           idx >= n_ents: row  = row0 + idx - n_ents:  coef = coef_a[row],                  x = x1[row]
// dW[d][f] = sum_items coef_d * x_f.  Workgroup (p, t) writes features [17 t, 17 t + 17) of partial p ([F][D]).
constexpr int WB_FT = 17;
template <int NJ>
__global__ void __launch_bounds__(256) k_bwd_flat_w(ParamLayout L, const float *__restrict__ x1, const float *__restrict__ x2,
                                                    const float *__restrict__ h2, const int32_t *__restrict__ ent_own,
                                                    const int32_t *__restrict__ ent_row, int row0, int n_rows, int ent0,
                                                    int n_ents, const float *__restrict__ coef_a,
                                                    const float *__restrict__ coef_g, float *__restrict__ dw_part) {
  constexpr int DP = NJ * 64;
  __shared__ float comb[WB_FT][DP];
  const int D = L.D, F = L.F;
  const int lane = lane_id(), wid = threadIdx.x / 64;
  const Chan<NJ> ch(lane, D);
  const int f0 = blockIdx.y * WB_FT;
  const int nf = min(WB_FT, F - f0);
  float acc[WB_FT][NJ];
#pragma unroll
  for (int k = 0; k < WB_FT; ++k)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[k][j] = 0.0f;
  const int n_items = n_ents + n_rows;
  const int wave_g = blockIdx.x * 4 + wid, n_waves = gridDim.x * 4;
  for (int base = wave_g; base < n_items; base += n_waves * 64) {
    // lane l holds the indices of item base + l * n_waves
    const int idx = base + lane * n_waves;
    int xo = -1, co = 0, ho = 0;                     // xo: row in x2 (>= 0) or x1 (encoded as -2 - row); co: coef row; ho: h2 row
    if (idx < n_ents) {
      const int e = ent0 + idx;
      const int o = ent_own[e];
      xo = o; ho = o - ent0; co = ent_row[e];        // h2 stored per owner (k_project_w)
    } else if (idx < n_items) {
      co = row0 + idx - n_ents; xo = -2 - co;
    }
    const int cnt = min(64, (n_items - base + n_waves - 1) / n_waves);
    for (int i = 0; i < cnt; ++i) {
      const int sx = __builtin_amdgcn_readlane(xo, i);
      const int sc = __builtin_amdgcn_readlane(co, i);
      const int sh = __builtin_amdgcn_readlane(ho, i);
      float coef[NJ];
      const float *xr;
      if (sx >= 0) {                                 // wave-uniform branch
        xr = x2 + (int64_t)sx * F;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const float g = coef_g[(int64_t)sc * D + ch.d[j]];
          const float hv = h2[(int64_t)sh * D + ch.d[j]];
          coef[j] = (ch.on[j] && hv > 0.0f) ? g : 0.0f;
        }
      } else {
        xr = x1 + (int64_t)(-2 - sx) * F;
#pragma unroll
        for (int j = 0; j < NJ; ++j) coef[j] = ch.on[j] ? coef_a[(int64_t)sc * D + ch.d[j]] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < WB_FT; ++k) {
        const float x = xr[min(f0 + k, F - 1)];      // (features past F: computed on a valid element, never stored)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[k][j] = fmaf(coef[j], x, acc[k][j]);
      }
    }
  }
  // the four waves, in wave order, through one LDS block
  for (int w = 0; w < 4; ++w) {
    if (wid == w) {
#pragma unroll
      for (int k = 0; k < WB_FT; ++k)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = lane + 64 * j;
          comb[k][c] = (w == 0) ? acc[k][j] : comb[k][c] + acc[k][j];
        }
    }
    __syncthreads();
  }
  float *out = dw_part + (int64_t)blockIdx.x * F * D + (int64_t)f0 * D;
  for (int i = threadIdx.x; i < nf * D; i += 256) {
    const int k = i / D, d = i - k * D;
    out[i] = comb[k][d];
  }
}

// ------------------------------------------------------------------ gradient reduce (+ fused Adam / exchange)
// k_grad_reduce of step.hip with the d w partials at a stride of NJ * 64 floats.  block = 64 parameters x GR_SUB
// sub-reducers; MODE 0: gradients only; 1: + Adam; 2: + the one-shot data-parallel exchange and Adam.
constexpr int GR_SUB = 16;
template <int MODE>
__global__ void __launch_bounds__(64 * GR_SUB) k_grad_reduce_w(ParamLayout L, const int32_t *__restrict__ pos_meta, int row0,
                                                       const float *__restrict__ losses8, const float *__restrict__ nbar,
                                                       const float *__restrict__ dw_part, int n_parts,
                                                       const float *__restrict__ dz, const float *__restrict__ gw_part,
                                                       int n_gw, int gw_stride, float *__restrict__ grads,
                                                       float *__restrict__ params, float *__restrict__ m, float *__restrict__ v,
                                                       float lr, float wd, const int32_t *__restrict__ step_counter,
                                                       ggad_xchg_view X, uint32_t xstep, float grad_scale) {
  __shared__ float sc[2];
  __shared__ float red[GR_SUB][64];
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if (MODE != 0) {
    if (tid == 0) {
      const double t = (double)(*step_counter);
      const double bc1 = 1.0 - pow(0.9, t), bc2 = 1.0 - pow(0.999, t);
      sc[0] = (float)((double)lr / bc1);      // step_size
      sc[1] = (float)sqrt(bc2);               // bias_correction2_sqrt
    }
  }
  const int D = L.D, F = L.F;
  const int t = blockIdx.x * 64 + threadIdx.x;
  const int sub = threadIdx.y;
  float g = 0.0f;
  int pidx = -1;
  if (t < D) {
    for (int k = sub; k < n_gw; k += GR_SUB) g += gw_part[(int64_t)k * gw_stride + t];   // d w = sum_q ds_q * combined_all[:, q]
    pidx = t;
  } else if (t < D + D * F) {
    const int u = t - D;
    const int f = u / D, d = u - f * D;           // consecutive threads -> consecutive d (coalesced reads)
    const float *p = dw_part + (int64_t)f * D + d;
    const int64_t stride = (int64_t)F * D;
    const int per = (n_parts + GR_SUB - 1) / GR_SUB;
    const int b0 = sub * per, b1 = min(n_parts, b0 + per);
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] += p[(int64_t)(b + k) * stride];
    }
    for (; b < b1; ++b) s[0] += p[(int64_t)b * stride];
    g = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    pidx = L.o_W() + d * F + f;
  } else if (t < L.n_train()) {
    const int u = t - D - D * F;
    const int dd = u / D, d2 = u - dd * D;        // d fc[dd][d2] = sum_{label-1 rows i} dZ_i[dd] * nbar_i[d2]
    const int n0 = (int)losses8[6], n1 = (int)losses8[7];
    float s0 = 0.0f;
    for (int j = sub; j < n1; j += GR_SUB) {      // label-1 rows = sources of the last n1 columns, in order
      const int ra = pos_meta[row0 + n0 + j] >> 2;
      s0 = fmaf(dz[(int64_t)ra * D + dd], nbar[(int64_t)ra * D + d2], s0);
    }
    g = s0; pidx = L.o_fc() + u;
  }
  red[sub][threadIdx.x] = g;
  __syncthreads();
  if (sub != 0 || pidx < 0) return;
  g = 0.0f;
#pragma unroll
  for (int k = 0; k < GR_SUB; ++k) g += red[k][threadIdx.x];          // fixed order
  grads[pidx] = g;
  if (MODE == 1) adam_update(params, m, v, L, pidx, g, wd, sc[0], sc[1]);
  if (MODE == 2) {
    const float s = xchg_sum(X, xstep, pidx, g);
    adam_update(params, m, v, L, pidx, s * grad_scale, wd, sc[0], sc[1]);
  }
}

// ------------------------------------------------------------------ score / encode: 8 rows per wave
constexpr int WS_RPW = 8;
template <int NJ, bool SCORE>
__global__ void __launch_bounds__(256) k_rows_w(const float *__restrict__ params, ParamLayout L, const float *__restrict__ x1,
                                                int n_rows, float *__restrict__ out) {
  const int D = L.D, F = L.F;
  const int lane = lane_id();
  const Chan<NJ> ch(lane, D);
  float wd[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wd[j] = ch.on[j] ? params[ch.d[j]] : 0.0f;
  const int wpb = blockDim.x / 64;
  for (int base = (blockIdx.x * wpb + threadIdx.x / 64) * WS_RPW; base < n_rows; base += gridDim.x * wpb * WS_RPW) {
    const float *xr[WS_RPW];
#pragma unroll
    for (int i = 0; i < WS_RPW; ++i) xr[i] = x1 + (int64_t)min(base + i, n_rows - 1) * F;
    float acc[WS_RPW][NJ];
    dot_rows<NJ, WS_RPW>(params + L.o_Wt(), D, F, ch, xr, acc);
#pragma unroll
    for (int i = 0; i < WS_RPW; ++i) {
      if (base + i >= n_rows) break;                                               // wave-uniform
      if (SCORE) {
        float p = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) p = fmaf(wd[j], fmaxf(acc[i][j], 0.0f), p);
        const float s = wave_sum_fast(p);
        if (lane == 0) out[base + i] = 1.0f / (1.0f + expf(-s));                   // torch.sigmoid            graphsage.py:180
      } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          if (ch.on[j]) out[(int64_t)(base + i) * D + ch.d[j]] = fmaxf(acc[i][j], 0.0f);   // graphsage.py:412
      }
    }
  }
}

// launch KERNEL<NJ, ...> with NJ = ceil(D / 64)
#define WIDE_DISPATCH(D, LAUNCH)        \
  switch (((D) + 63) / 64) {            \
    case 1: { constexpr int NJ = 1; LAUNCH; } break; \
    case 2: { constexpr int NJ = 2; LAUNCH; } break; \
    case 3: { constexpr int NJ = 3; LAUNCH; } break; \
    default: { constexpr int NJ = 4; LAUNCH; } break; \
  }

}  // namespace

bool ggad_int_wide_ok(int D, int F) { return D >= 1 && D <= WIDE_MAX_D && F >= 1 && F <= GGAD_MAX_F; }

int ggad_int_wide_project(const float *params, int32_t D, int32_t F, const float *x2, const int32_t *ent_own, int32_t ent0,
                          int32_t n_ents, float *h2, ggad_stream_t stream) {
  GGAD_REQUIRE(params && x2 && ent_own && h2 && ggad_int_wide_ok(D, F) && ent0 >= 0 && n_ents >= 0);
  if (n_ents == 0) return GGAD_OK;
  ParamLayout L{D, F};
  const int blocks = (n_ents + 4 * WP_EPW - 1) / (4 * WP_EPW);
  WIDE_DISPATCH(D, (k_project_w<NJ><<<dim3(blocks), dim3(256), 0, as_stream(stream)>>>(params, L, x2, ent_own, ent0, n_ents, h2)));
  GGAD_CHECK_LAUNCH("mb_project (wide)");
  return GGAD_OK;
}

int ggad_int_wide_fwd_rows(const float *params, int32_t D, int32_t F, const float *x1, const float *h2, const int32_t *ent_ptr,
                           const int32_t *ent_own, const int32_t *labels, int32_t row0, int32_t n_rows, int32_t ent0, float *h1,
                           float *nbar, float *gen, ggad_stream_t stream) {
  GGAD_REQUIRE(params && x1 && h2 && ent_ptr && ent_own && labels && h1 && nbar && gen && ggad_int_wide_ok(D, F));
  GGAD_REQUIRE(n_rows >= 0 && row0 >= 0 && ent0 >= 0);
  if (n_rows == 0) return GGAD_OK;
  ParamLayout L{D, F};
  WIDE_DISPATCH(D, (k_fwd_rows_w<NJ><<<dim3(n_rows), dim3(WF_NW * 64), 0, as_stream(stream)>>>(
                       params, L, x1, h2, ent_ptr, ent_own, labels, row0, ent0, h1, nbar, gen)));
  GGAD_CHECK_LAUNCH("mb_fwd_rows (wide)");
  return GGAD_OK;
}

// loss_ws: pos_scal[n_rows][8] | part[nwg][8] | d w partials [nwg][NJ * 64]  (ggad_mb_loss_workspace_elems sizes the last for NJ = 4)
int ggad_int_wide_loss(const float *params, int32_t D, int32_t F, const float *h1, const float *nbar, const float *gen,
                       const int32_t *labels, const int32_t *pos_meta, const int32_t *row_pos, const int32_t *ent_ptr,
                       int32_t row0, int32_t n_rows, float *loss_ws, float *losses8, float *d_h1, float *d_gen, float *d_nbar,
                       float *dz, float *coef_a, float *coef_g, int32_t *step_counter, ggad_stream_t stream) {
  GGAD_REQUIRE(params && h1 && nbar && gen && labels && pos_meta && row_pos && ent_ptr && loss_ws && losses8);
  GGAD_REQUIRE(dz && coef_a && coef_g);
  GGAD_REQUIRE((d_h1 == nullptr) == (d_gen == nullptr) && (d_h1 == nullptr) == (d_nbar == nullptr));
  GGAD_REQUIRE(ggad_int_wide_ok(D, F) && n_rows >= 1 && row0 >= 0);
  ParamLayout L{D, F};
  const int nwg = loss_nwg(n_rows);
  float *pos_scal = loss_ws, *part = loss_ws + (int64_t)n_rows * 8, *gw_part = part + (int64_t)nwg * 8;
  hipStream_t st = as_stream(stream);
  WIDE_DISPATCH(D, (k_loss_pos_w<NJ><<<dim3(nwg), dim3(256), 0, st>>>(params, D, h1, nbar, gen, pos_meta, row0, n_rows, pos_scal, part)));
  WIDE_DISPATCH(D, (k_loss_rows_w<NJ><<<dim3(nwg), dim3(256), 0, st>>>(params, L, h1, nbar, gen, labels, pos_meta, row_pos, ent_ptr, row0,
                                                                       n_rows, pos_scal, part, gw_part, losses8, d_h1, d_gen, d_nbar, dz,
                                                                       coef_a, coef_g, step_counter)));
  GGAD_CHECK_LAUNCH("mb_loss (wide)");
  return GGAD_OK;
}

int ggad_int_wide_row_coefs(const float *params, int32_t D, int32_t F, const int32_t *labels, const int32_t *ent_ptr,
                            int32_t row0, int32_t n_rows, const float *h1, const float *gen, const float *d_h1,
                            const float *d_gen, const float *d_nbar, float *dz, float *coef_a, float *coef_g,
                            ggad_stream_t stream) {
  GGAD_REQUIRE(params && labels && ent_ptr && h1 && gen && d_h1 && d_gen && d_nbar && dz && coef_a && coef_g);
  GGAD_REQUIRE(ggad_int_wide_ok(D, F) && n_rows >= 1 && row0 >= 0);
  ParamLayout L{D, F};
  WIDE_DISPATCH(D, (k_row_coefs_w<NJ><<<dim3((n_rows + 3) / 4), dim3(256), 0, as_stream(stream)>>>(
                       params, L, labels, ent_ptr, row0, n_rows, h1, gen, d_h1, d_gen, d_nbar, dz, coef_a, coef_g)));
  GGAD_CHECK_LAUNCH("mb_row_coefs (wide)");
  return GGAD_OK;
}

int ggad_int_wide_bwd_flat(int32_t D, int32_t F, const float *x1, const float *x2, const float *h2, const int32_t *ent_own,
                           const int32_t *ent_row, int32_t row0, int32_t n_rows, int32_t ent0, int32_t n_ents,
                           const float *coef_a, const float *coef_g, float *dw_part, ggad_stream_t stream) {
  GGAD_REQUIRE(x1 && x2 && h2 && ent_own && ent_row && coef_a && coef_g && dw_part && ggad_int_wide_ok(D, F));
  GGAD_REQUIRE(n_rows >= 1 && row0 >= 0 && ent0 >= 0 && n_ents >= 0);
  ParamLayout L{D, F};
  const dim3 grid(GGAD_MB_BWD_PARTS, (F + WB_FT - 1) / WB_FT);
  WIDE_DISPATCH(D, (k_bwd_flat_w<NJ><<<grid, dim3(256), 0, as_stream(stream)>>>(L, x1, x2, h2, ent_own, ent_row, row0, n_rows, ent0,
                                                                                 n_ents, coef_a, coef_g, dw_part)));
  GGAD_CHECK_LAUNCH("mb_bwd_flat (wide)");
  return GGAD_OK;
}

// mode 0: gradients only (params / m / v unused); 1: + Adam; 2: + exchange (xv) + Adam
int ggad_int_wide_grad_reduce(int32_t D, int32_t F, const int32_t *pos_meta, int32_t row0, int32_t n_rows, const float *losses8,
                              const float *nbar, const float *dw_part, const float *dz, const float *loss_ws, float *grads,
                              int mode, float *params, float *m, float *v, float lr, float wd, const int32_t *step_counter,
                              const ggad_xchg_view *xv, uint32_t xstep, float grad_scale, ggad_stream_t stream) {
  GGAD_REQUIRE(pos_meta && losses8 && nbar && dw_part && dz && loss_ws && grads && ggad_int_wide_ok(D, F) && n_rows >= 1);
  GGAD_REQUIRE(mode == 0 || (params && m && v && step_counter));
  GGAD_REQUIRE(mode != 2 || xv != nullptr);
  ParamLayout L{D, F};
  const int nwg = loss_nwg(n_rows);
  const float *gw_part = loss_ws + (int64_t)n_rows * 8 + (int64_t)nwg * 8;
  const int gws = (D + 63) / 64 * 64;
  const dim3 grid((L.n_train() + 63) / 64), block(64, GR_SUB);
  hipStream_t st = as_stream(stream);
  if (mode == 0)
    k_grad_reduce_w<0><<<grid, block, 0, st>>>(L, pos_meta, row0, losses8, nbar, dw_part, GGAD_MB_BWD_PARTS, dz, gw_part, nwg, gws, grads,
                                               nullptr, nullptr, nullptr, 0.f, 0.f, nullptr, ggad_xchg_view{}, 0u, 1.0f);
  else if (mode == 1)
    k_grad_reduce_w<1><<<grid, block, 0, st>>>(L, pos_meta, row0, losses8, nbar, dw_part, GGAD_MB_BWD_PARTS, dz, gw_part, nwg, gws, grads,
                                               params, m, v, lr, wd, step_counter, ggad_xchg_view{}, 0u, 1.0f);
  else
    k_grad_reduce_w<2><<<grid, block, 0, st>>>(L, pos_meta, row0, losses8, nbar, dw_part, GGAD_MB_BWD_PARTS, dz, gw_part, nwg, gws, grads,
                                               params, m, v, lr, wd, step_counter, *xv, xstep, grad_scale);
  GGAD_CHECK_LAUNCH("mb_grad_reduce (wide)");
  return GGAD_OK;
}

int ggad_int_wide_rows(const float *params, int32_t D, int32_t F, const float *x1, int32_t n_rows, float *out, int score,
                       ggad_stream_t stream) {
  GGAD_REQUIRE(params && x1 && out && ggad_int_wide_ok(D, F) && n_rows >= 0);
  if (n_rows == 0) return GGAD_OK;
  ParamLayout L{D, F};
  const int want = (n_rows + 4 * WS_RPW - 1) / (4 * WS_RPW);
  const int blocks = want < 4096 ? want : 4096;
  if (score) {
    WIDE_DISPATCH(D, (k_rows_w<NJ, true><<<dim3(blocks), dim3(256), 0, as_stream(stream)>>>(params, L, x1, n_rows, out)));
  } else {
    WIDE_DISPATCH(D, (k_rows_w<NJ, false><<<dim3(blocks), dim3(256), 0, as_stream(stream)>>>(params, L, x1, n_rows, out)));
  }
  GGAD_CHECK_LAUNCH(score ? "mb_score (wide)" : "mb_encode (wide)");
  return GGAD_OK;
}

extern "C" {

int ggad_mb_wide_max_embed_dim(void) { return WIDE_MAX_D; }
int ggad_mb_wide_supported(int32_t D, int32_t F) { return ggad_int_wide_ok(D, F) ? 1 : 0; }

}  // extern "C"
