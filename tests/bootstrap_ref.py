"""The reference of `ggad_rank_bootstrap_f32` (csrc/rank_metrics.hip; the scheme is stated in include/ggad_hip.h), numpy on the host.

`philox4x32_10` is Random123's generator in uint64 arithmetic (every word a 32-bit value held in 64 bits, so the 32 x 32 products are
exact); `draws` is the call-to-draw rule (call j gives draws 2j and 2j + 1; a draw over m outcomes is the high 64 bits of x m);
`bins` makes the chain's three arrays -- the sorted positives, histU, histE -- from scores and labels; `replicate` bins the draws of
one replicate into (w, cU, cE); `terms` turns three such histograms into (AP* by `math.fsum`, the exact AUROC numerator).
`element_weights` expands a replicate into one weight per element, for scikit-learn's `sample_weight`.
tests/test_bootstrap_cpu.py holds this against known answers, scikit-learn and DeLong; tests/test_bootstrap_gpu.py holds the kernel
against it."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MAX_POS, MAX_REPS = 9216, 4096
TOO_FEW, TOO_MANY = 8, 9


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two ints; the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) for c in counter)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def mulhi64(x, m):
    """(x m) >> 64 for uint64 x and an integer 0 < m < 2^32."""
    assert 0 < m < 1 << 32
    m = np.uint64(m)
    return ((x >> S32) * m + (((x & MASK) * m) >> S32)) >> S32


def draws(seed, rep, stream, count, m):
    """`count` draws over m outcomes of replicate `rep` on `stream`, int64."""
    calls = (count + 1) // 2
    j = np.arange(calls, dtype=np.uint64)
    c = philox4x32_10((j & MASK, j >> S32, rep, stream), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    x = np.empty(2 * calls, dtype=np.uint64)
    x[0::2], x[1::2] = c[0] | (c[1] << S32), c[2] | (c[3] << S32)
    return mulhi64(x[:count], m).astype(np.int64)


def fold(s):
    s = np.asarray(s, dtype=np.float32)
    return np.where(s == 0, np.float32(0.0), s)


def bins(s, y):
    """(pos sorted ascending, histU[P + 1], histE[P + 1], order of the positives, ub per negative, tie per negative)."""
    s, y = fold(s), np.asarray(y)
    ip, ineg = np.flatnonzero(y == 1), np.flatnonzero(y != 1)
    order = ip[np.argsort(s[ip], kind="stable")]
    pos, neg = s[order], s[ineg]
    P = len(pos)
    ub = np.searchsorted(pos, neg, side="right").astype(np.int64)
    tie = (ub >= 1) & (pos[np.maximum(ub - 1, 0)] == neg) if P else np.zeros(len(neg), dtype=bool)
    hist_u = np.bincount(ub, minlength=P + 1).astype(np.int64)
    hist_e = np.bincount(ub[tie] - 1, minlength=P + 1).astype(np.int64)
    return pos, hist_u, hist_e, order, ub, tie


def runs(pos):
    """(s, e): first and last index of the run of equal values that holds each sorted positive."""
    return np.searchsorted(pos, pos, side="left").astype(np.int64), np.searchsorted(pos, pos, side="right").astype(np.int64) - 1


def replicate(seed, rep, hist_u, hist_e):
    """(w[P + 1] with w[P] = 0, cU[P + 1], cE[P + 1]) of replicate `rep`, int64."""
    P = len(hist_u) - 1
    Nn = int(hist_u.sum())
    w = np.bincount(draws(seed, rep, 0, P, P), minlength=P + 1).astype(np.int64)
    u = draws(seed, rep, 1, Nn, Nn)
    cum = np.cumsum(hist_u)
    b = np.searchsorted(cum, u, side="right")                                    # entries of cum that are <= u
    below = np.maximum(b - 1, 0)
    tied = (b >= 1) & (u - (cum[b] - hist_u[b]) < hist_e[below])
    c_u = np.bincount(b, minlength=P + 1).astype(np.int64)
    c_e = np.bincount(b[tied] - 1, minlength=P + 1).astype(np.int64)
    return w, c_u, c_e


def terms(pos, w, c_u, c_e):
    """(AP* by fsum, num* as a python integer) of three histograms."""
    P = len(pos)
    Nn = int(c_u.sum())
    s, e = runs(pos)
    w = np.asarray(w[:P], dtype=np.int64)
    L = np.cumsum(c_u)[:P]
    suffix = np.concatenate([np.cumsum(w[::-1])[::-1], [0]])
    tp = suffix[s]
    den = tp + Nn - L
    drawn = w != 0
    q = np.zeros(P, dtype=np.float64)
    q[drawn] = (w[drawn] * tp[drawn]).astype(np.float64) / den[drawn].astype(np.float64)
    num = sum(int(v) for v in (w * (2 * L + c_e[e])).tolist())
    return math.fsum(q.tolist()) / P, num


def status_of(s, y, pos_cap=None):
    s, y = np.asarray(s), np.asarray(y)
    if (y > 1).any():
        return 4
    if np.isnan(s).any():
        return 3
    p = int((y == 1).sum())
    if pos_cap is not None and p > pos_cap:
        return 2
    if p == 0 or p == len(y):
        return 1
    if p > MAX_POS:
        return TOO_MANY
    if p < 2 or len(y) - p < 2:
        return TOO_FEW
    return 0


def bootstrap(s, y, seed, reps, keep_hist=True):
    """dict(P, Nn, pos, hist_u, hist_e, ap float64[reps], num int64[reps], auc float64[reps], hist int64[reps, 3, P + 1] or None)."""
    pos, hist_u, hist_e = bins(s, y)[:3]
    P, Nn = len(pos), int(hist_u.sum())
    ap, num = np.empty(reps, dtype=np.float64), np.empty(reps, dtype=np.int64)
    hist = np.empty((reps, 3, P + 1), dtype=np.int64) if keep_hist else None
    for r in range(reps):
        h = replicate(seed, r, hist_u, hist_e)
        ap[r], num[r] = terms(pos, *h)
        if keep_hist:
            hist[r] = h
    return dict(P=P, Nn=Nn, pos=pos, hist_u=hist_u, hist_e=hist_e, ap=ap, num=num, auc=num.astype(np.float64) / float(2 * P * Nn), hist=hist)


def summary(point, reps, level):
    """(lo, hi, se, bias) of a replicate array around its point estimate, as `metrics.ap_ci` states them."""
    reps = np.asarray(reps, dtype=np.float64)
    lo, hi = np.quantile(reps, [(1 - level) / 2, (1 + level) / 2])
    return float(lo), float(hi), float(reps.std(ddof=1)) if len(reps) > 1 else float("nan"), float(reps.mean() - point)


def element_weights(s, y, w, c_u, c_e):
    """One weight per element that stands for the replicate: the positive of sorted rank k weighs w[k]; the tied negatives of bin b
    share cE[b - 1] and its other negatives cU[b] - cE[b - 1] (each part's weight on its first element: inside a part the places are
    exchangeable for every rank metric)."""
    pos, hist_u, hist_e, order, ub, tie = bins(s, y)
    out = np.zeros(len(np.asarray(y)), dtype=np.float64)
    out[order] = w[:len(pos)]
    ineg = np.flatnonzero(np.asarray(y) != 1)
    for part, weight in ((tie, lambda b: c_e[b - 1]), (~tie, lambda b: c_u[b] - (c_e[b - 1] if b >= 1 else 0))):
        idx, bb = ineg[part], ub[part]
        first = np.unique(bb, return_index=True)
        for b, at in zip(*first):
            out[idx[at]] = weight(int(b))
    return out
