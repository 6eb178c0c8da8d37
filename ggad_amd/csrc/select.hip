// Model selection on the device: "if this epoch's validation metric is the best so far, keep this epoch's weights", with no host
// round trip, so that it can sit at the end of a captured and replayed training epoch.
//
//   k_select_decide  ONE thread: reads the eight doubles ggad_rank_metrics_f32 / ggad_rank_wide_f32 left in out8, appends
//                    {auroc, ap, status} to the curve, compares the chosen metric with the best so far (strict > in double: an equal
//                    later epoch never displaces an earlier one; a NaN or a non-zero status never wins) and leaves the verdict in
//                    state4[3], the epoch counter advanced in state4[2]
//   k_select_copy    copies up to SEL_MAX_T tensors src -> dst if and only if state4[3] == 1, grid-stride over the concatenated
//                    tensors in units of four floats
//
// The decision is a launch of its own so that every workgroup of the copy reads a word nobody writes while the copy runs: no
// workgroup waits on another, there is no ticket and no floating-point atomic.  A model with more tensors than one launch takes is
// copied by several launches after ONE decide: they all follow the same flag.  Neither call takes a workspace, and each reads only
// words the host or an earlier launch wrote: both are capturable and replayable.
//
// Alignment.  A parameter may be a view at any 4-byte offset and its length need not be a multiple of 4.  Where source and
// destination sit at the SAME offset within a 16-byte line, the first 0..3 floats are peeled (4-byte accesses), the body moves as
// 16-byte vectors and the last 0..3 floats are 4-byte accesses again; where the two offsets differ no 16-byte access can be aligned
// on both sides and the whole tensor moves in 4-byte accesses.  dst is never read.
#include "common.h"

namespace {

constexpr int SEL_MAX_T = 16;
constexpr int SEL_T = 256;                // threads of a workgroup
constexpr int SEL_MAX_G = 2048;           // workgroups at most (8 per CU): beyond that the grid strides

struct SelectCopy {
  const float *src[SEL_MAX_T];
  float *dst[SEL_MAX_T];
  int64_t n[SEL_MAX_T];                   // elements of every tensor
  int64_t unit0[SEL_MAX_T + 1];           // first unit of every tensor in the concatenated range; [n_t] = all units
  int32_t head[SEL_MAX_T];                // floats ahead of the first 16-byte line (0..3, <= n); unit 0 of the tensor moves them too
  int32_t vec[SEL_MAX_T];                 // 1: full units of this tensor are 16-byte aligned on both sides
  int32_t n_t;
};

__global__ void k_select_decide(const double *__restrict__ out8, int which, double *__restrict__ state4, double *__restrict__ curve,
                                int64_t curve_cap) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double auroc = out8[0], ap = out8[1], status = out8[7];
  const double ed = state4[2];
  const int64_t e = (int64_t)ed;
  if (curve && e >= 0 && e < curve_cap) {
    curve[3 * e + 0] = auroc;
    curve[3 * e + 1] = ap;
    curve[3 * e + 2] = status;
  }
  const double value = which ? ap : auroc;
  const bool taken = status == 0.0 && value == value && (state4[1] < 0.0 || value > state4[0]);
  if (taken) {
    state4[0] = value;
    state4[1] = ed;
  }
  state4[2] = ed + 1.0;
  state4[3] = taken ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(SEL_T) k_select_copy(SelectCopy C, const double *__restrict__ state4) {
  if (state4[3] != 1.0) return;                                  // (written by k_select_decide, an earlier launch: uniform)
  const int64_t total = C.unit0[C.n_t], stride = (int64_t)gridDim.x * SEL_T;
  int t = 0;
  for (int64_t u = (int64_t)blockIdx.x * SEL_T + threadIdx.x; u < total; u += stride) {
    while (u >= C.unit0[t + 1]) ++t;                             // (u only grows; u < total = unit0[n_t] bounds t)
    const float *__restrict__ s = C.src[t];
    float *__restrict__ d = C.dst[t];
    const int64_t nt = C.n[t], lu = u - C.unit0[t];
    const int h = C.head[t];
    if (lu == 0)
      for (int k = 0; k < h; ++k) d[k] = s[k];
    const int64_t i0 = h + 4 * lu;
    if (i0 + 4 <= nt) {
      if (C.vec[t]) {
        *reinterpret_cast<float4 *>(d + i0) = *reinterpret_cast<const float4 *>(s + i0);
      } else {
        const float a = s[i0], b = s[i0 + 1], c = s[i0 + 2], e = s[i0 + 3];
        d[i0] = a; d[i0 + 1] = b; d[i0 + 2] = c; d[i0 + 3] = e;
      }
    } else {
      for (int64_t i = i0; i < nt; ++i) d[i] = s[i];
    }
  }
}

}  // namespace

extern "C" {

int32_t ggad_select_max_tensors(void) { return SEL_MAX_T; }

int ggad_select_decide_f64(const double *out8, int32_t which, double *state4, double *curve, int64_t curve_cap, ggad_stream_t stream) {
  GGAD_REQUIRE(out8 && state4 && (which == 0 || which == 1) && (!curve || curve_cap >= 0));
  k_select_decide<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(out8, which, state4, curve, curve_cap);
  GGAD_CHECK_LAUNCH("select_decide_f64");
  return GGAD_OK;
}

int ggad_select_copy_f32(int32_t n, const float *const *src, float *const *dst, const int64_t *numel, const double *state4,
                         ggad_stream_t stream) {
  GGAD_REQUIRE(n >= 1 && n <= SEL_MAX_T && src && dst && numel && state4);
  SelectCopy C;
  int64_t units = 0;
  int k = 0;
  for (int t = 0; t < n; ++t) {
    const uintptr_t sa = reinterpret_cast<uintptr_t>(src[t]), da = reinterpret_cast<uintptr_t>(dst[t]);
    GGAD_REQUIRE(numel[t] >= 0 && sa % 4 == 0 && da % 4 == 0 && (numel[t] == 0 || (src[t] && dst[t])));      // (an empty tensor may be null)
    if (numel[t] == 0) continue;
    const bool same = sa % 16 == da % 16;
    int64_t h = same ? (int64_t)((16 - sa % 16) % 16 / 4) : 0;
    if (h > numel[t]) h = numel[t];
    const int64_t body = (numel[t] - h + 3) / 4;
    C.src[k] = src[t]; C.dst[k] = dst[t]; C.n[k] = numel[t];
    C.head[k] = (int32_t)h; C.vec[k] = same ? 1 : 0;
    C.unit0[k] = units;
    units += body > 0 ? body : 1;                                // (a tensor that ends inside its head still has unit 0)
    ++k;
  }
  if (k == 0) return GGAD_OK;
  C.unit0[k] = units;
  C.n_t = k;
  int64_t blocks = (units + SEL_T - 1) / SEL_T;
  if (blocks > SEL_MAX_G) blocks = SEL_MAX_G;
  k_select_copy<<<dim3((unsigned)blocks), dim3(SEL_T), 0, as_stream(stream)>>>(C, state4);
  GGAD_CHECK_LAUNCH("select_copy_f32");
  return GGAD_OK;
}

}  // extern "C"
