// Full-graph TAM comparison model (reference tam.py:113-146): the affinity head and its loss, fused.
//
//   a_i    = r_inv_i <e_hat_i, sum_{j in R_i} v_ij e_hat_j>      e_hat_i = inv_i e_i,  inv_i = 1 / |e_i| (inf -> 0)
//   loss   = - sum_i cnt_i (a_i - lo) / (hi - lo)                 lo = min a, hi = max a, cnt_i = occurrences of i in the index list
//   m_i    = (a_i - lo) / (hi - lo)
//
// Forward, three launches (+ one when m is asked for):
//   k_tam_inv     inv_i, one wave per row.
//   k_tam_gather  (forward form) one wave per work item.  Items [0, n) are the rows: a row of at most TAM_HUB entries is gathered whole
//                 and a_i stored; a longer row (a hub) is left to items [n, n + n_pieces), one per piece of TAM_HUB consecutive entries,
//                 which store the SCALAR <e_i, sum_{j in piece} v_ij inv_j e_j> (the dot product is linear in the row sum).
//   k_tam_reduce  adds a hub's scalars in piece order and stores its a_i; min, max, their tie counts and S = sum cnt_i a_i as one
//                 partial per workgroup over a fixed row range; the last workgroup behind the ticket merges the partials in slot
//                 order and writes (loss, lo, hi, n_lo, n_hi, S).
//   k_tam_norm    m_i (optional).
// Backward, two launches:
//   k_tam_coef    c_i = g r_inv_i dloss/da_i (closed form of torch's evenly distributed min / max gradient).
//   k_tam_gather  (backward form) den_i = sum_j v_ij (c_i + c_j) e_hat_j (R symmetric), d_e_i = inv_i (den_i - e_hat_i <e_hat_i, den_i>).
//                 A hub's pieces store their part of den_i; the last piece WAVE to arrive behind the hub's own ticket adds the parts
//                 in piece order and finishes the row.
//
// e_hat is never stored: the gather reads e_j and inv_j and scales on the fly.  A lane owns channels lane + 64 q (1 <= h <= 256: at
// most four).  A row's sum runs in CSR order with TAM_FLY neighbour rows in flight per wave; every load is unconditional with its
// index clamped (a clamped entry gets the weight 0).  No float atomics, no workgroup waits on another: equal inputs give equal bits.
#include "common.h"
#include "handoff.h"
#include <algorithm>

#define TAM_MAX_H 256
#define TAM_HUB 512          // a row with MORE stored entries than this is cut into pieces of this many
#define TAM_FLY 4            // neighbour rows in flight per wave
#define TAM_MAX_G 256        // workgroups (partial slots) of k_tam_reduce
#define TAM_SLOT 8           // words per slot: lo, hi, S, n_lo, n_hi, n_nan, -, -
#define TAM_SCAL 8           // floats of the scalar block: loss, lo, hi, n_lo, n_hi, S, -, -

// ------------------------------------------------------------------------------------------------ inv
__global__ void __launch_bounds__(256) k_tam_inv(const float *__restrict__ E, int n, int h, float *__restrict__ inv) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int lane = lane_id();
  const float *x = E + (int64_t)r * h;
  float ss = 0.f;
  for (int c = lane; c < h; c += 64) ss = fmaf(x[c], x[c], ss);
  ss = wave_sum(ss);
  float iv = 1.0f / sqrtf(ss);
  if (isinf(iv)) iv = 0.0f;
  if (lane == 0) inv[r] = iv;
}

// ------------------------------------------------------------------------------------------------ gather
// acc[q] += sum over entries [p0, p1) of row i (p0 < p1) of  w_p * E[col_p][lane + 64 q],  w_p = v_p inv_j (ci + c_j in the backward)
template <int Q, bool BWD>
__device__ __forceinline__ void tam_row_sum(const int32_t *__restrict__ col, const float *__restrict__ val, const float *__restrict__ E,
                                            const float *__restrict__ inv, const float *__restrict__ cvec, float ci, int n, int h,
                                            int p0, int p1, const int (&ch)[Q], float (&acc)[Q]) {
  for (int p = p0; p < p1; p += TAM_FLY) {
    float w[TAM_FLY], x[TAM_FLY][Q];
#pragma unroll
    for (int k = 0; k < TAM_FLY; ++k) {
      const int pk = min(p + k, p1 - 1);
      const int j = min(max(col[pk], 0), n - 1);
      float wk = val[pk] * inv[j];
      if (BWD) wk *= ci + cvec[j];
      w[k] = (p + k < p1) ? wk : 0.f;
      const float *ej = E + (int64_t)j * h;
#pragma unroll
      for (int q = 0; q < Q; ++q) x[k][q] = ej[ch[q]];
    }
#pragma unroll
    for (int k = 0; k < TAM_FLY; ++k)
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] = fmaf(w[k], x[k][q], acc[q]);
  }
}

// items [0, n): rows; [n, n + n_pieces): pieces of the hubs (hub_rows[b] owns pieces [hub_pp[b], hub_pp[b + 1])).
// forward:  a[i] or part_s[piece];  backward: dE[i], hubs through part_v[piece][h] and tickets[b].
template <int Q, bool BWD>
__global__ void __launch_bounds__(256) k_tam_gather(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const float *__restrict__ val, const float *__restrict__ E,
                                                    const float *__restrict__ inv, const float *__restrict__ r_inv,
                                                    const float *__restrict__ cvec, int n, int h, const int32_t *__restrict__ hub_rows,
                                                    const int32_t *__restrict__ hub_pp, int n_hub, int n_pieces,
                                                    float *__restrict__ a, float *__restrict__ part_s, float *__restrict__ dE,
                                                    float *__restrict__ part_v, int32_t *__restrict__ tickets) {
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= n + n_pieces) return;
  const int lane = lane_id();
  int i = item, hb = -1, piece = 0;
  if (item >= n) {                                         // a hub piece: the last b with hub_pp[b] <= piece
    piece = item - n;
    int lo = 0, hi = n_hub;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (hub_pp[mid] <= piece) lo = mid; else hi = mid;
    }
    hb = lo;
    i = min(max(hub_rows[hb], 0), n - 1);
  }
  const int s = rowptr[i], e = rowptr[i + 1];
  int p0 = s, p1 = e;
  if (hb < 0) {
    if (e - s > TAM_HUB && n_hub > 0) return;              // its pieces do it
  } else {
    p0 = min(s + max(piece - hub_pp[hb], 0) * TAM_HUB, e);
    p1 = min(p0 + TAM_HUB, e);
  }
  int ch[Q];
  float msk[Q], acc[Q], ei[Q];
  const float *erow = E + (int64_t)i * h;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c = lane + 64 * q;
    ch[q] = min(c, h - 1);
    msk[q] = c < h ? 1.f : 0.f;
    acc[q] = 0.f;
    ei[q] = erow[ch[q]] * msk[q];
  }
  const float iv = inv[i];
  const float ci = BWD ? cvec[i] : 0.f;
  if (p0 < p1) tam_row_sum<Q, BWD>(col, val, E, inv, cvec, ci, n, h, p0, p1, ch, acc);

  if (!BWD) {
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) dot = fmaf(ei[q], acc[q], dot);
    dot = wave_sum(dot);
    if (lane == 0) {
      if (hb < 0) a[i] = r_inv[i] * (iv * dot);
      else part_s[piece] = dot;
    }
    return;
  }

  if (hb >= 0) {
    // the piece's part of den_i, then the hub's ticket (handoff.h, the wave form)
    float *pv = part_v + (int64_t)piece * h;
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (lane + 64 * q < h) pv[lane + 64 * q] = acc[q];
    const int first = hub_pp[hb], cnt = hub_pp[hb + 1] - first;
    if (!ggad_last_wave_of(tickets + hb, cnt)) return;
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    for (int k = 0; k < cnt; ++k) {                        // piece order
      const float *pk = part_v + (int64_t)(first + k) * h;
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] += ld_agent(pk + ch[q]);
    }
  }
  float dot = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    ei[q] *= iv;                                           // e_hat_i
    dot = fmaf(ei[q], acc[q], dot);
  }
  dot = wave_sum(dot);
  float *drow = dE + (int64_t)i * h;
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (lane + 64 * q < h) drow[lane + 64 * q] = iv * (acc[q] - ei[q] * dot);
}

// ------------------------------------------------------------------------------------------------ reduce
struct TamPart {
  float lo, hi, s;
  int n_lo, n_hi, n_nan;
};
__device__ __forceinline__ void tam_merge(TamPart &x, const TamPart &y) {      // commutative, exact but for s
  if (y.lo < x.lo) { x.lo = y.lo; x.n_lo = y.n_lo; } else if (y.lo == x.lo) x.n_lo += y.n_lo;
  if (y.hi > x.hi) { x.hi = y.hi; x.n_hi = y.n_hi; } else if (y.hi == x.hi) x.n_hi += y.n_hi;
  x.s += y.s;
  x.n_nan += y.n_nan;
}
// the workgroup's 256 values -> one, valid in thread 0: the wave butterfly, then the four waves in wave order
__device__ __forceinline__ void tam_block_merge(TamPart &x, TamPart *sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    TamPart y;
    y.lo = __shfl_xor(x.lo, off, GGAD_WAVE); y.hi = __shfl_xor(x.hi, off, GGAD_WAVE); y.s = __shfl_xor(x.s, off, GGAD_WAVE);
    y.n_lo = __shfl_xor(x.n_lo, off, GGAD_WAVE); y.n_hi = __shfl_xor(x.n_hi, off, GGAD_WAVE);
    y.n_nan = __shfl_xor(x.n_nan, off, GGAD_WAVE);
    tam_merge(x, y);
  }
  __syncthreads();                                         // sh may still be read from an earlier call
  if (lane_id() == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w) tam_merge(x, sh[w]);
}

__global__ void __launch_bounds__(256) k_tam_reduce(const int32_t *__restrict__ rowptr, const float *__restrict__ inv,
                                                    const float *__restrict__ r_inv, const float *__restrict__ cnt, float K, int n,
                                                    const int32_t *__restrict__ hub_rows, const int32_t *__restrict__ hub_pp, int n_hub,
                                                    const float *__restrict__ part_s, float *__restrict__ a, float *__restrict__ slots,
                                                    float *__restrict__ scal, int32_t *__restrict__ ticket) {
  __shared__ TamPart sh[4];
  __shared__ int flag;
  const int t = threadIdx.x, G = gridDim.x, b = blockIdx.x;
  const int r0 = (int)((int64_t)n * b / G), r1 = (int)((int64_t)n * (b + 1) / G);
  TamPart x = {INFINITY, -INFINITY, 0.f, 0, 0, 0};
  for (int i = r0 + t; i < r1; i += 256) {
    float ai;
    if (rowptr[i + 1] - rowptr[i] > TAM_HUB && n_hub > 0) {               // a hub: its scalars in piece order
      const int hb = min(lower_bound_i32(hub_rows, 0, n_hub, i), n_hub - 1);
      float dot = 0.f;
      for (int k = hub_pp[hb]; k < hub_pp[hb + 1]; ++k) dot += part_s[k];
      ai = r_inv[i] * (inv[i] * dot);
      a[i] = ai;
    } else {
      ai = a[i];
    }
    const TamPart y = {ai, ai, cnt[i] * ai, 1, 1, ai != ai ? 1 : 0};
    tam_merge(x, y);
  }
  tam_block_merge(x, sh);
  if (t == 0) {
    float *sl = slots + (int64_t)b * TAM_SLOT;
    sl[0] = x.lo; sl[1] = x.hi; sl[2] = x.s;
    sl[3] = __int_as_float(x.n_lo); sl[4] = __int_as_float(x.n_hi); sl[5] = __int_as_float(x.n_nan);
  }
  if (!ggad_last_of(ticket, G, &flag)) return;
  TamPart y = {INFINITY, -INFINITY, 0.f, 0, 0, 0};
  if (t < G) {                                             // G <= 256: slot t in thread t, merged in slot order by the fixed tree
    const float *sl = slots + (int64_t)t * TAM_SLOT;
    y.lo = ld_agent(sl); y.hi = ld_agent(sl + 1); y.s = ld_agent(sl + 2);
    y.n_lo = __float_as_int(ld_agent(sl + 3)); y.n_hi = __float_as_int(ld_agent(sl + 4)); y.n_nan = __float_as_int(ld_agent(sl + 5));
  }
  tam_block_merge(y, sh);
  if (t == 0) {
    if (y.n_nan > 0) { y.lo = NAN; y.hi = NAN; }           // torch.min / torch.max hand a NaN on
    const float d = y.hi - y.lo, num = y.s - K * y.lo;
    scal[0] = -num / d;
    scal[1] = y.lo; scal[2] = y.hi; scal[3] = (float)y.n_lo; scal[4] = (float)y.n_hi; scal[5] = y.s;
    scal[6] = 0.f; scal[7] = 0.f;
  }
}

__global__ void __launch_bounds__(256) k_tam_norm(const float *__restrict__ a, const float *__restrict__ scal, int n,
                                                  float *__restrict__ m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float lo = scal[1], d = scal[2] - lo;
  m[i] = (a[i] - lo) / d;
}

// c_i = g r_inv_i (-cnt_i / d + [a_i = lo] (K / d - N / d^2) / n_lo + [a_i = hi] (N / d^2) / n_hi),  N = S - K lo
__global__ void __launch_bounds__(256) k_tam_coef(const float *__restrict__ a, const float *__restrict__ scal,
                                                  const float *__restrict__ cnt, const float *__restrict__ r_inv,
                                                  const float *__restrict__ g, float K, int n, float *__restrict__ cvec) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float lo = scal[1], hi = scal[2], d = hi - lo, num = scal[5] - K * lo, nd2 = num / (d * d);
  const float ai = a[i];
  float da = -cnt[i] / d;
  if (ai == lo) da += (K / d - nd2) / scal[3];
  if (ai == hi) da += nd2 / scal[4];
  cvec[i] = (*g * r_inv[i]) * da;
}

// ------------------------------------------------------------------------------------------------ host
// workspace (floats; the ticket words are int32 in the same block and must be ZERO before the first call, the kernels leave them zero):
//   [tickets: 1 + n_hub, rounded up to 64][c: n][slots: TAM_MAX_G * TAM_SLOT][part_s: n_pieces][part_v: n_pieces * h]
struct TamWs {
  int32_t *tickets;
  float *c, *slots, *part_s, *part_v;
  int64_t total;
};
static TamWs tam_ws(float *ws, int64_t n, int64_t h, int64_t n_hub, int64_t n_pieces) {
  TamWs w;
  int64_t o = 0;
  w.tickets = reinterpret_cast<int32_t *>(ws);
  o += (1 + n_hub + 63) / 64 * 64;
  w.c = ws + o; o += n;
  w.slots = ws + o; o += (int64_t)TAM_MAX_G * TAM_SLOT;
  w.part_s = ws + o; o += n_pieces;
  w.part_v = ws + o; o += n_pieces * h;
  w.total = o;
  return w;
}

extern "C" {

int32_t ggad_tam_head_max_dim(void) { return TAM_MAX_H; }
int32_t ggad_tam_head_hub_len(void) { return TAM_HUB; }
int32_t ggad_tam_head_supported(int32_t n, int32_t h) { return (n >= 1 && h >= 1 && h <= TAM_MAX_H) ? 1 : 0; }
int64_t ggad_tam_head_workspace_elems(int32_t n, int32_t h, int32_t n_hub, int32_t n_pieces) {
  if (n < 0 || h < 0 || n_hub < 0 || n_pieces < 0) return 0;
  return tam_ws(nullptr, n, h, n_hub, n_pieces).total;
}

#define TAM_GATHER(BWD, ...)                                                                                 \
  do {                                                                                                       \
    const dim3 grid((unsigned)(((int64_t)n + n_pieces + 3) / 4)), block(256);                                \
    switch ((h + 63) / 64) {                                                                                 \
      case 1: k_tam_gather<1, BWD><<<grid, block, 0, st>>>(__VA_ARGS__); break;                              \
      case 2: k_tam_gather<2, BWD><<<grid, block, 0, st>>>(__VA_ARGS__); break;                              \
      case 3: k_tam_gather<3, BWD><<<grid, block, 0, st>>>(__VA_ARGS__); break;                              \
      default: k_tam_gather<4, BWD><<<grid, block, 0, st>>>(__VA_ARGS__); break;                             \
    }                                                                                                        \
  } while (0)

static bool tam_args_ok(int32_t n, int32_t n_hub, int32_t n_pieces, const int32_t *hub_rows, const int32_t *hub_pp) {
  return n >= 1 && n_hub >= 0 && n_pieces >= 0 && (n_hub == 0 ? n_pieces == 0 : (hub_rows && hub_pp && n_pieces >= 2 * (int64_t)n_hub));
}

int ggad_tam_head_fwd_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *emb, const float *r_inv,
                          const float *cnt, float k_total, int32_t n, int32_t h, const int32_t *hub_rows, const int32_t *hub_piece_ptr,
                          int32_t n_hub, int32_t n_pieces, float *a, float *scal, float *m, float *inv, float *workspace,
                          ggad_stream_t stream) {
  GGAD_REQUIRE(rowptr && col && val && emb && r_inv && cnt && a && scal && inv && workspace);
  if (!ggad_tam_head_supported(n, h)) return GGAD_E_UNSUPPORTED;
  GGAD_REQUIRE(tam_args_ok(n, n_hub, n_pieces, hub_rows, hub_piece_ptr));
  hipStream_t st = as_stream(stream);
  const TamWs w = tam_ws(workspace, n, h, n_hub, n_pieces);
  k_tam_inv<<<dim3((n + 3) / 4), dim3(256), 0, st>>>(emb, n, h, inv);
  GGAD_CHECK_LAUNCH("k_tam_inv");
  TAM_GATHER(false, rowptr, col, val, emb, inv, r_inv, nullptr, n, h, hub_rows, hub_piece_ptr, n_hub, n_pieces, a, w.part_s,
             nullptr, nullptr, nullptr);
  GGAD_CHECK_LAUNCH("k_tam_gather fwd");
  const int G = (int)std::min<int64_t>(TAM_MAX_G, ((int64_t)n + 255) / 256);
  k_tam_reduce<<<dim3(G), dim3(256), 0, st>>>(rowptr, inv, r_inv, cnt, k_total, n, hub_rows, hub_piece_ptr, n_hub, w.part_s, a,
                                              w.slots, scal, w.tickets);
  GGAD_CHECK_LAUNCH("k_tam_reduce");
  if (m) {
    k_tam_norm<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(a, scal, n, m);
    GGAD_CHECK_LAUNCH("k_tam_norm");
  }
  return GGAD_OK;
}

int ggad_tam_head_bwd_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *emb, const float *r_inv,
                          const float *cnt, float k_total, int32_t n, int32_t h, const int32_t *hub_rows, const int32_t *hub_piece_ptr,
                          int32_t n_hub, int32_t n_pieces, const float *a, const float *scal, const float *inv, const float *g,
                          float *d_emb, float *workspace, ggad_stream_t stream) {
  GGAD_REQUIRE(rowptr && col && val && emb && r_inv && cnt && a && scal && inv && g && d_emb && workspace);
  if (!ggad_tam_head_supported(n, h)) return GGAD_E_UNSUPPORTED;
  GGAD_REQUIRE(tam_args_ok(n, n_hub, n_pieces, hub_rows, hub_piece_ptr));
  hipStream_t st = as_stream(stream);
  const TamWs w = tam_ws(workspace, n, h, n_hub, n_pieces);
  k_tam_coef<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(a, scal, cnt, r_inv, g, k_total, n, w.c);
  GGAD_CHECK_LAUNCH("k_tam_coef");
  TAM_GATHER(true, rowptr, col, val, emb, inv, r_inv, w.c, n, h, hub_rows, hub_piece_ptr, n_hub, n_pieces, nullptr, nullptr, d_emb,
             w.part_v, w.tickets + 1);
  GGAD_CHECK_LAUNCH("k_tam_gather bwd");
  return GGAD_OK;
}

}  // extern "C"
