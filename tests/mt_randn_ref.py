"""numpy restatement of `torch.randn` (float32, contiguous, n >= 16) on torch's CPU generator, from any state and position.  Test
infrastructure: the reference of tests/test_device_noise_cpu.py (against torch itself) and tests/test_device_noise_gpu.py (the kernel).

    n raw MT19937 words w -> u = float32(w & 0xFFFFFF) * 2^-24
    per chunk of 16, j < 8:  u1 = 1 - u[j], u2 = u[j + 8], r = sqrt(-2 log u1), t = 2 pi u2, out[j] = r cos t, out[j + 8] = r sin t
    n % 16 != 0: 16 MORE words are drawn and out[n - 16:n] is recomputed from them (the call consumes n + 16 words)

State = (words, pos): the 624 words of the current block and how many of them are consumed; pos = 624 regenerates the block before the
next word, as torch's engine does (lazily: a draw that ends on a block boundary leaves pos = 624)."""
import numpy as np

MT_N, MT_M = 624, 397
LAG = MT_N - MT_M


def _f(cur, nxt, far):
    y = (cur & np.uint32(0x80000000)) | (nxt & np.uint32(0x7FFFFFFF))
    return far ^ (y >> np.uint32(1)) ^ np.where(nxt & np.uint32(1), np.uint32(0x9908B0DF), np.uint32(0)).astype(np.uint32)


def twist(words):
    """The next block of 624 words: word k + 624 from words k, k + 1, k + 397 -- three dependent steps of at most 227 words."""
    o = np.asarray(words, dtype=np.uint32)
    nw = np.empty_like(o)
    nw[:LAG] = _f(o[:LAG], o[1:LAG + 1], o[MT_M:])
    nw[LAG:2 * LAG] = _f(o[LAG:2 * LAG], o[LAG + 1:2 * LAG + 1], nw[:LAG])
    nw[2 * LAG:MT_N - 1] = _f(o[2 * LAG:MT_N - 1], o[2 * LAG + 1:], nw[LAG:MT_M - 1])
    nw[MT_N - 1] = _f(o[MT_N - 1:], nw[:1], nw[MT_M - 1:MT_M])[0]
    return nw


def temper(y):
    y = np.asarray(y, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def raw_words(words, pos, count):
    """(count tempered words, words', pos')."""
    words = np.asarray(words, dtype=np.uint32).copy()
    pos = int(pos)
    out = np.empty(count, dtype=np.uint32)
    done = 0
    while done < count:
        if pos == MT_N:
            words, pos = twist(words), 0
        take = min(MT_N - pos, count - done)
        out[done:done + take] = temper(words[pos:pos + take])
        done += take
        pos += take
    return out, words, pos


def words_consumed(n):
    return n + (16 if n % 16 else 0)


def draw_uniforms(words, pos, n):
    """(u, words', pos'): the words_consumed(n) uniforms of one `torch.randn(n)` as float32, and the state after it."""
    if n < 16:
        raise ValueError("torch.randn below 16 elements is a different algorithm")
    w, words, pos = raw_words(words, pos, words_consumed(n))
    return (w & np.uint32(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24), words, pos


def _pairs(chunks, dtype):
    """float64: the formula.  float32: every operation of torch's float32 evaluation (1 - u, log, -2 *, sqrt, 2 pi *, cos / sin, r *)
    with its result rounded to float32 -- log, cos and sin evaluated in float64 first, so that they are the correctly rounded float32
    values on any host (numpy's own float32 routines differ between CPUs); torch's vector routines are within a float32 step of them."""
    if np.dtype(dtype) == np.float64:
        c = chunks.astype(np.float64)
        u1, u2 = 1.0 - c[:, :8], c[:, 8:]
        r = np.sqrt(-2.0 * np.log(u1))
        t = 2.0 * np.pi * u2
        return np.concatenate([r * np.cos(t), r * np.sin(t)], axis=1), np.concatenate([r, r], axis=1)
    f32, f64 = np.float32, np.float64
    c = chunks.astype(f32)
    u1, u2 = f32(1) - c[:, :8], c[:, 8:]
    r = np.sqrt((f32(-2) * np.log(u1.astype(f64)).astype(f32)).astype(f64)).astype(f32)
    t = (f32(2 * np.pi) * u2).astype(f32)
    cs, sn = np.cos(t.astype(f64)).astype(f32), np.sin(t.astype(f64)).astype(f32)
    return np.concatenate([r * cs, r * sn], axis=1).astype(f32), np.concatenate([r, r], axis=1)


def box_muller(u, n, dtype=np.float32):
    """(values, r): the n normals of the draw whose uniforms are `u`, evaluated in `dtype` (float32: the restatement of torch;
    float64: the formula itself on the same u), and the radius r of every value."""
    full = n // 16 * 16
    v, r = _pairs(u[:full].reshape(-1, 16), dtype)
    out, rad = np.empty(n, dtype=dtype), np.empty(n, dtype=dtype)
    out[:full], rad[:full] = v.reshape(-1), r.reshape(-1)
    if n % 16:
        v, r = _pairs(u[n:n + 16].reshape(1, 16), dtype)
        out[n - 16:], rad[n - 16:] = v.reshape(-1), r.reshape(-1)
    return out, rad


def randn(words, pos, n):
    """(values float32, words', pos') of `torch.randn(n)` from the state (words, pos)."""
    u, words, pos = draw_uniforms(words, pos, n)
    return box_muller(u, n)[0], words, pos
