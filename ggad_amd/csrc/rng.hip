// torch.randn's CPU stream, continued on the device (ggad_mt_randn_f32).
//
// torch's default CPU generator is MT19937.  `torch.randn(n)` (float32, contiguous, n >= 16) takes n raw 32-bit words, turns each
// into u = (w & 0xFFFFFF) * 2^-24, and runs Box-Muller over chunks of 16: for j < 8, u1 = 1 - u[j], u2 = u[j + 8],
// r = sqrt(-2 log u1), t = 2 pi u2, out[j] = r cos t, out[j + 8] = r sin t.  When n % 16 != 0 it draws 16 more words and recomputes the
// LAST 16 outputs from them.  Here the 624 state words and the read position live in HBM, so a captured launch draws fresh values on
// every replay and the host does nothing in between.
//
// MT19937 is a lag recurrence: word k + 624 needs words k, k + 1 and k + 397, so at most 227 new words can be computed side by side.
// A block of 624 words is therefore three dependent steps (227 + 227 + 170 words), and a draw of n words is a serial chain of about
// 3 n / 624 steps: it belongs to ONE workgroup with the state in LDS (k_mt_words: two images, the new block is written beside the old
// one, one barrier per step).  That workgroup only tempers the words and stores them; the conversion and Box-Muller are independent
// per pair and run on the whole grid in a second launch (k_mt_normal).
//
// The block is regenerated lazily, exactly when torch's engine would do it (a draw that ends on a block boundary leaves the position
// at 624), so the state handed back to the host is word for word the one the host generator would hold.
#include "common.h"

namespace {

constexpr int MT_N = 624, MT_M = 397, MT_LAG = MT_N - MT_M;      // 227 independent words per step
constexpr int MT_POS = MT_N;                                      // state[624]: words of the current block already consumed, 0..624
constexpr int MT_STATE_WORDS = 640;                               // 624 + position, padded to a multiple of 64 bytes
constexpr int MT_THREADS = 256;
constexpr int64_t MT_MAX_N = (int64_t)1 << 36;

__device__ __forceinline__ uint32_t mt_twist(uint32_t cur, uint32_t nxt, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((nxt & 1u) ? 0x9908b0dfu : 0u);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// One workgroup: advances `state` by `total` words and writes them, tempered, to words[0, total).
__global__ __launch_bounds__(MT_THREADS) void k_mt_words(uint32_t *__restrict__ state, uint32_t *__restrict__ words, int64_t total) {
  __shared__ uint32_t s[2][MT_N];
  const int t = threadIdx.x;
  for (int i = t; i < MT_N; i += MT_THREADS) s[0][i] = state[i];
  int pos = (int)state[MT_POS];
  pos = pos < 0 ? 0 : (pos > MT_N ? MT_N : pos);                  // (a corrupt position must not index outside the block)
  int cur = 0;
  __syncthreads();
  int64_t done = 0;
  while (done < total) {                                          // uniform: every thread sees the same pos / done
    if (pos == MT_N) {
      const uint32_t *o = s[cur];
      uint32_t *nw = s[cur ^ 1];
      if (t < MT_LAG) nw[t] = mt_twist(o[t], o[t + 1], o[t + MT_M]);                        // 0..226: old words only
      __syncthreads();
      if (t < MT_LAG) {                                                                     // 227..453: new words 0..226
        const int i = MT_LAG + t;
        nw[i] = mt_twist(o[i], o[i + 1], nw[i - MT_LAG]);
      }
      __syncthreads();
      {                                                                                     // 454..623: new words 227..396, and new word 0
        const int i = 2 * MT_LAG + t;
        if (i < MT_N) nw[i] = mt_twist(o[i], i + 1 < MT_N ? o[i + 1] : nw[0], nw[i - MT_LAG]);
      }
      __syncthreads();
      cur ^= 1;
      pos = 0;
    }
    const int64_t left = total - done;
    const int take = left < (int64_t)(MT_N - pos) ? (int)left : MT_N - pos;
    for (int i = t; i < take; i += MT_THREADS) words[done + i] = mt_temper(s[cur][pos + i]);
    done += take;
    pos += take;
  }
  for (int i = t; i < MT_N; i += MT_THREADS) state[i] = s[cur][i];
  if (t == 0) state[MT_POS] = (uint32_t)pos;
}

__device__ __forceinline__ float mt_uniform(uint32_t w) { return (float)(w & 0xffffffu) * 5.9604644775390625e-08f; }      // 2^-24, exact

// One thread per Box-Muller pair.  The pairs of the full chunks read words[c * 16 + j], [c * 16 + j + 8]; with n % 16 != 0 eight more
// pairs read words[n, n + 16) and own out[n - 16, n), which the full chunks then leave alone.
__global__ __launch_bounds__(MT_THREADS) void k_mt_normal(const uint32_t *__restrict__ words, float *__restrict__ out, int64_t n, float scale,
                                                          float shift) {
  const int64_t p = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  const int64_t full = (n >> 4) << 3;
  const bool has_tail = (n & 15) != 0;
  if (p >= full + (has_tail ? 8 : 0)) return;
  const int j = (int)(p & 7);
  const bool tail = p >= full;
  const int64_t w0 = tail ? n + j : ((p >> 3) << 4) + j;
  const int64_t o0 = tail ? n - 16 + j : w0;
  const int64_t lim = (has_tail && !tail) ? n - 16 : n;
  const float u1 = 1.0f - mt_uniform(words[w0]);                  // (0, 1]: exact, and never 0
  const float u2 = mt_uniform(words[w0 + 8]);
  const float r = sqrtf(__fmul_rn(-2.0f, logf(u1)));
  const float th = __fmul_rn(6.283185307179586f, u2);
  float sn, cs;
  sincosf(th, &sn, &cs);
  // product and sum rounded separately, as `torch.randn(...) * var + mean` rounds them
  if (o0 < lim) out[o0] = __fadd_rn(__fmul_rn(__fmul_rn(r, cs), scale), shift);
  if (o0 + 8 < lim) out[o0 + 8] = __fadd_rn(__fmul_rn(__fmul_rn(r, sn), scale), shift);
}

}  // namespace

extern "C" {

int32_t ggad_mt_state_words(void) { return MT_STATE_WORDS; }

int64_t ggad_mt_randn_scratch_elems(int64_t n) { return (n < 16 || n > MT_MAX_N) ? 0 : n + 16; }

int ggad_mt_randn_f32(uint32_t *state, float *out, int64_t n, float scale, float shift, uint32_t *scratch, ggad_stream_t stream) {
  GGAD_REQUIRE(state && out && scratch);
  GGAD_REQUIRE(n >= 16 && n <= MT_MAX_N);
  const int64_t total = n + ((n & 15) ? 16 : 0);
  k_mt_words<<<dim3(1), dim3(MT_THREADS), 0, as_stream(stream)>>>(state, scratch, total);
  GGAD_CHECK_LAUNCH("mt_words");
  const int64_t pairs = ((n >> 4) << 3) + ((n & 15) ? 8 : 0);
  const int64_t grid = (pairs + MT_THREADS - 1) / MT_THREADS;
  k_mt_normal<<<dim3((unsigned)grid), dim3(MT_THREADS), 0, as_stream(stream)>>>(scratch, out, n, scale, shift);
  GGAD_CHECK_LAUNCH("mt_normal");
  return GGAD_OK;
}

}  // extern "C"
