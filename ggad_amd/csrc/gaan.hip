// Full-graph GAAN comparison model (reference model_gaan.py / gaan.py): the edge loss over A_hat.
//
// The reference builds a = sigmoid(emb emb^T) and a' = sigmoid(z z^T) as dense N x N matrices and reads them at the edge set
// E = { (i, j) : i in idx_train (list order), (normalize_adj(A) + I)[i, j] > 0 (j ascending) }:
//
//   loss = (BCE(a'_E, 0) + BCE(a_E, 1)) / 2,   each a mean over the m = |E| entries, a' detached.
//
// Only the m entries of E are ever evaluated here.  E is handed in as two int32 arrays in the reference's order (erow = i, ecol = j),
// built on the host from the row list (ggad_amd/model_gaan.py: edge_structs), with the column side grouped per node for the
// backward (tptr / trow / tedge: the entries (i, k) of column k in ascending entry order).
//
//   ggad_gaan_edge_fwd_f32  one pass over E: both dots, both sigmoids, both clamped logs; a_e = sigmoid(<emb_i, emb_j>) kept per
//                           entry (m floats: the backward's coefficient is a function of it and the incoming gradient); per-workgroup
//                           partial sums, then a one-workgroup launch adds them in order and divides.
//   ggad_gaan_edge_bwd_f32  dE_k = sum_{(k,j) in E} g_kj emb_j + sum_{(i,k) in E} g_ik emb_i for every node k (zero rows where k has no
//                           entry), g_e = ((g/2/m) (a_e - 1) / max((1 - a_e) a_e, 1e-12)) (1 - a_e) a_e as torch's BCE and sigmoid
//                           backwards compute it.
//
// Layout: C = 64 channels = 16 lanes x float4; a wave holds four 16-lane groups, a workgroup sixteen.  Per entry a group gathers the
// two 256-byte rows it needs (emb_j, z_j forward; emb_src backward).  Every sum has a fixed order and there are no atomics, so a
// replayed hipGraph equals an eager epoch bit for bit.
#include "common.h"

#define GAAN_C 64            // channels the kernels take (hid_dim of the discriminator, model_gaan.py:160)
#define GAAN_FWD_ENTRIES 1024 // entries per forward workgroup (64 per 16-lane group)
#define GAAN_BWD_SMALL 64    // a node with at most this many (row + column) entries is walked by one 16-lane group, else by a workgroup
#define GAAN_UNROLL 4        // entries in flight per group

__device__ __forceinline__ float gaan_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// sum over the 16 lanes of a group (xor butterfly: every lane of the group gets the same bits)
__device__ __forceinline__ float group_sum16(float v) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, GGAD_WAVE);
  return v;
}

__device__ __forceinline__ float dot4(float4 a, float4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

__device__ __forceinline__ float4 ld4(const float *__restrict__ base, int64_t row, int c0) {
  return *reinterpret_cast<const float4 *>(base + row * GAAN_C + c0);
}

// ------------------------------------------------------------------------------------------------ forward
// Workgroup b owns entries [m b / G, m (b + 1) / G); group g of it the contiguous sixteenth g of that range, walked in order
// GAAN_UNROLL entries at a time (all their gathers issued before the first dot).  Per entry: d = <emb_i, emb_j>, d' = <z_i, z_j>,
// a = sigmoid(d) stored, the BCE terms -max(log(a), -100) (target 1) and -max(log1p(-a'), -100) (target 0) as torch evaluates them:
// a = 1.0f gives log1p(-a) = -inf -> -100, a = 0.0f gives log(a) = -inf -> -100.  The group's two sums, then the 16 groups in order,
// go to part[2 b], part[2 b + 1].
__global__ __launch_bounds__(256) void k_gaan_fwd(const float *__restrict__ emb, const float *__restrict__ z,
                                                  const int32_t *__restrict__ erow, const int32_t *__restrict__ ecol, int64_t m,
                                                  float *__restrict__ a_out, float *__restrict__ part) {
  __shared__ float s_r[16], s_f[16];
  const int t = threadIdx.x, grp = t >> 4, l = t & 15, c0 = l * 4;
  const int64_t G = gridDim.x, b = blockIdx.x;
  const int64_t lo = m * b / G, hi = m * (b + 1) / G, len = hi - lo;
  const int64_t e0 = lo + len * grp / 16, e1 = lo + len * (grp + 1) / 16;
  float sr = 0.f, sf = 0.f;
  for (int64_t eb = e0; eb < e1; eb += GAAN_UNROLL) {
    float4 ei[GAAN_UNROLL], ej[GAAN_UNROLL], zi[GAAN_UNROLL], zj[GAAN_UNROLL];
#pragma unroll
    for (int u = 0; u < GAAN_UNROLL; ++u) {
      if (eb + u < e1) {
        const int64_t i = erow[eb + u], j = ecol[eb + u];
        ei[u] = ld4(emb, i, c0);
        ej[u] = ld4(emb, j, c0);
        zi[u] = ld4(z, i, c0);
        zj[u] = ld4(z, j, c0);
      }
    }
#pragma unroll
    for (int u = 0; u < GAAN_UNROLL; ++u) {
      if (eb + u < e1) {                                  // (uniform across the group: its 16 lanes share eb)
        const float d = group_sum16(dot4(ei[u], ej[u]));
        const float dz = group_sum16(dot4(zi[u], zj[u]));
        const float a = gaan_sigmoid(d), af = gaan_sigmoid(dz);
        sr += -fmaxf(logf(a), -100.f);
        sf += -fmaxf(log1pf(-af), -100.f);
        if (l == 0) a_out[eb + u] = a;
      }
    }
  }
  if (l == 0) {
    s_r[grp] = sr;
    s_f[grp] = sf;
  }
  __syncthreads();
  if (t == 0) {
    float r = 0.f, f = 0.f;
    for (int g = 0; g < 16; ++g) {
      r += s_r[g];
      f += s_f[g];
    }
    part[2 * b] = r;
    part[2 * b + 1] = f;
  }
}

// One workgroup: thread t adds partials t, t + 256, ... in order, the 256 thread sums go through the wave butterflies and the four
// waves in order.  loss[1] = BCE(a', 0) = sum_f / m, loss[2] = BCE(a, 1) = sum_r / m, loss[0] = (loss[1] + loss[2]) / 2 (the
// reference's (loss_f + loss_r) / 2).  m = 0 gives NaN, as torch's mean of nothing does.
__global__ __launch_bounds__(256) void k_gaan_fwd_final(const float *__restrict__ part, int G, int64_t m, float *__restrict__ loss) {
  __shared__ float s_r[4], s_f[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  float r = 0.f, f = 0.f;
  for (int k = t; k < G; k += 256) {
    r += part[2 * k];
    f += part[2 * k + 1];
  }
  r = wave_sum(r);
  f = wave_sum(f);
  if (lane == 0) {
    s_r[w] = r;
    s_f[w] = f;
  }
  __syncthreads();
  if (t == 0) {
    const float sr = ((s_r[0] + s_r[1]) + s_r[2]) + s_r[3];
    const float sf = ((s_f[0] + s_f[1]) + s_f[2]) + s_f[3];
    const float lf = sf / (float)m, lr = sr / (float)m;
    loss[0] = (lf + lr) / 2.f;
    loss[1] = lf;
    loss[2] = lr;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// Entry t of node k's list: t < rdeg -> row side (entry e = rbeg + t, source j = ecol[e]), else column side (q = cbeg + t - rdeg,
// e = tedge[q], source i = trow[q]).  acc += g_e emb_src over [t0, t1) in order, GAAN_UNROLL gathers in flight.
__device__ __forceinline__ float gaan_coef(float a, float g0) {
  // torch: BCE backward grad (a - t) / max((1 - a) a, 1e-12), then sigmoid backward grad (1 - a) a
  return ((g0 * (a - 1.f)) / fmaxf((1.f - a) * a, 1e-12f)) * (1.f - a) * a;
}

__device__ __forceinline__ void gaan_walk(const float *__restrict__ emb, const int32_t *__restrict__ ecol, const int32_t *__restrict__ trow,
                                          const int32_t *__restrict__ tedge, const float *__restrict__ a, float g0, int64_t rbeg, int64_t rdeg,
                                          int64_t cbeg, int64_t t0, int64_t t1, int c0, float4 &acc) {
  for (int64_t tb = t0; tb < t1; tb += GAAN_UNROLL) {
    float4 x[GAAN_UNROLL];
    float c[GAAN_UNROLL];
#pragma unroll
    for (int u = 0; u < GAAN_UNROLL; ++u) {
      const int64_t tt = tb + u;
      if (tt < t1) {
        int64_t e, src;
        if (tt < rdeg) {
          e = rbeg + tt;
          src = ecol[e];
        } else {
          const int64_t q = cbeg + (tt - rdeg);
          e = tedge[q];
          src = trow[q];
        }
        c[u] = a[e];
        x[u] = ld4(emb, src, c0);
      }
    }
#pragma unroll
    for (int u = 0; u < GAAN_UNROLL; ++u) {
      if (tb + u < t1) {
        const float g = gaan_coef(c[u], g0);
        acc.x = fmaf(g, x[u].x, acc.x);
        acc.y = fmaf(g, x[u].y, acc.y);
        acc.z = fmaf(g, x[u].z, acc.z);
        acc.w = fmaf(g, x[u].w, acc.w);
      }
    }
  }
}

struct GaanNode {
  int64_t rbeg, rdeg, cbeg, count;
};
__device__ __forceinline__ GaanNode gaan_node(int64_t k, const int32_t *__restrict__ pos, const int32_t *__restrict__ rptr,
                                              const int32_t *__restrict__ tptr) {
  GaanNode o;
  const int p = pos[k];
  o.rbeg = p >= 0 ? rptr[p] : 0;
  o.rdeg = p >= 0 ? (int64_t)rptr[p + 1] - o.rbeg : 0;
  o.cbeg = tptr[k];
  o.count = o.rdeg + ((int64_t)tptr[k + 1] - o.cbeg);
  return o;
}

// Blocks [0, n_small_blocks): group g of block b takes node small[16 b + g] and walks its whole list.  Blocks after that: one node
// big[b - n_small_blocks] per workgroup, group g walking the contiguous sixteenth g of its list; the 16 partial rows are added in
// group order.  Every node is in exactly one of the two lists.
__global__ __launch_bounds__(256) void k_gaan_bwd(const float *__restrict__ emb, const int32_t *__restrict__ pos,
                                                  const int32_t *__restrict__ rptr, const int32_t *__restrict__ ecol,
                                                  const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                  const int32_t *__restrict__ tedge, const float *__restrict__ a, int64_t m,
                                                  const float *__restrict__ gloss, const int32_t *__restrict__ small, int64_t n_small,
                                                  const int32_t *__restrict__ big, int64_t n_small_blocks, float *__restrict__ dE) {
  __shared__ float4 s_acc[16][16];
  const int t = threadIdx.x, grp = t >> 4, l = t & 15, c0 = l * 4;
  const float g0 = (gloss[0] / 2.f) / (float)m;                   // d loss / d a_e before BCE: (g / 2) / m (mean backward)
  const int64_t b = blockIdx.x;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (b < n_small_blocks) {
    const int64_t s = b * 16 + grp;
    if (s >= n_small) return;                                     // (no barrier in this branch)
    const int64_t k = small[s];
    const GaanNode nd = gaan_node(k, pos, rptr, tptr);
    gaan_walk(emb, ecol, trow, tedge, a, g0, nd.rbeg, nd.rdeg, nd.cbeg, 0, nd.count, c0, acc);
    *reinterpret_cast<float4 *>(dE + k * GAAN_C + c0) = acc;
    return;
  }
  const int64_t k = big[b - n_small_blocks];
  const GaanNode nd = gaan_node(k, pos, rptr, tptr);
  gaan_walk(emb, ecol, trow, tedge, a, g0, nd.rbeg, nd.rdeg, nd.cbeg, nd.count * grp / 16, nd.count * (grp + 1) / 16, c0, acc);
  s_acc[grp][l] = acc;
  __syncthreads();
  if (t < GAAN_C) {
    const int ll = t >> 2, cc = t & 3;
    float v = 0.f;
    for (int g = 0; g < 16; ++g) {
      const float4 p = s_acc[g][ll];
      v += cc == 0 ? p.x : cc == 1 ? p.y : cc == 2 ? p.z : p.w;
    }
    dE[k * GAAN_C + t] = v;
  }
}

// ------------------------------------------------------------------------------------------------ host side
static int64_t gaan_fwd_groups(int64_t m) {
  const int64_t g = (m + GAAN_FWD_ENTRIES - 1) / GAAN_FWD_ENTRIES;
  return g < 1 ? 1 : g;
}
static bool gaan_al16(const void *q) { return ((uintptr_t)q & 15) == 0; }

extern "C" {

int32_t ggad_gaan_edge_channels(void) { return GAAN_C; }
int32_t ggad_gaan_bwd_small_count(void) { return GAAN_BWD_SMALL; }
int64_t ggad_gaan_edge_fwd_workspace_elems(int64_t m) { return m >= 0 ? 2 * gaan_fwd_groups(m) : 0; }

int ggad_gaan_edge_fwd_f32(const float *emb, const float *z, int64_t n, int32_t C, const int32_t *erow, const int32_t *ecol, int64_t m,
                           float *a_out, float *ws, float *loss, ggad_stream_t stream) {
  GGAD_REQUIRE(emb && z && n >= 1 && m >= 0 && (m == 0 || (erow && ecol && a_out)) && ws && loss);
  if (C != GAAN_C) return GGAD_E_UNSUPPORTED;
  GGAD_REQUIRE(gaan_al16(emb) && gaan_al16(z));
  const int64_t G = gaan_fwd_groups(m);
  GGAD_REQUIRE(G <= 0x7fffffff);
  if (m > 0) {
    k_gaan_fwd<<<dim3((unsigned)G), dim3(256), 0, as_stream(stream)>>>(emb, z, erow, ecol, m, a_out, ws);
    GGAD_CHECK_LAUNCH("gaan_edge_fwd");
  }
  k_gaan_fwd_final<<<dim3(1), dim3(256), 0, as_stream(stream)>>>(ws, m > 0 ? (int)G : 0, m, loss);
  GGAD_CHECK_LAUNCH("gaan_edge_fwd_final");
  return GGAD_OK;
}

int ggad_gaan_edge_bwd_f32(const float *emb, int64_t n, int32_t C, const int32_t *pos, const int32_t *rptr, const int32_t *ecol,
                           const int32_t *tptr, const int32_t *trow, const int32_t *tedge, const float *a, int64_t m, const float *gloss,
                           const int32_t *small, int64_t n_small, const int32_t *big, int64_t n_big, float *dE, ggad_stream_t stream) {
  GGAD_REQUIRE(emb && n >= 1 && pos && rptr && tptr && gloss && dE && m >= 1 && ecol && trow && tedge && a);
  GGAD_REQUIRE(n_small >= 0 && n_big >= 0 && n_small + n_big == n && (n_small == 0 || small) && (n_big == 0 || big));
  if (C != GAAN_C) return GGAD_E_UNSUPPORTED;
  GGAD_REQUIRE(gaan_al16(emb) && gaan_al16(dE));
  const int64_t nsb = (n_small + 15) / 16, grid = nsb + n_big;
  GGAD_REQUIRE(grid <= 0x7fffffff);
  k_gaan_bwd<<<dim3((unsigned)grid), dim3(256), 0, as_stream(stream)>>>(emb, pos, rptr, ecol, tptr, trow, tedge, a, m, gloss, small, n_small,
                                                                        big, nsb, dE);
  GGAD_CHECK_LAUNCH("gaan_edge_bwd");
  return GGAD_OK;
}

}  // extern "C"
