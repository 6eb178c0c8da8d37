"""The reference of `ggad_rank_delong_f32` and `ggad_rank_delong_pair_f32` (csrc/rank_metrics.hip), numpy and python integers on the host.
With +-0 folded together, m positives x, n negatives y and the doubled placements

    a_i = 2 #{y < x_i} + #{y == x_i}        b_j = 2 #{x > y_j} + #{x == y_j}

(`placements`, by `searchsorted`), S1 = sum a = sum b, S2 = sum a^2, T2 = sum b^2, C10 = sum_i a_i^A a_i^B and C01 = sum_j b_j^A b_j^B
are exact python integers (`dot`: chunked int64 partials of 16-bit halves, so no intermediate overflows), and the variances are
`Fraction`s of them as include/ggad_hip.h states.  `brute` is the O(mn) definition with psi in {0, 1/2, 1} in `Fraction`s, for small
inputs.  tests/test_delong_cpu.py holds one against the other and against the midrank form; tests/test_delong_gpu.py holds the kernels
against `single` and `pair`."""
from fractions import Fraction

import numpy as np


def fold(s):
    s = np.asarray(s, dtype=np.float32)
    return np.where(s == 0, np.float32(0.0), s)


def placements(s, y):
    """(a int64 per positive, b int64 per negative), in the order of the elements."""
    s, y = fold(s), np.asarray(y)
    x, z = s[y == 1], s[y == 0]
    ox, oz = np.argsort(x, kind="stable"), np.argsort(z, kind="stable")
    xs, zs = x[ox], z[oz]                                         # (sorted queries: the searches walk the table once)
    a, b = np.empty(len(x), dtype=np.int64), np.empty(len(z), dtype=np.int64)
    a[ox] = np.searchsorted(zs, xs, side="left") + np.searchsorted(zs, xs, side="right")
    b[oz] = 2 * len(x) - np.searchsorted(xs, zs, side="left") - np.searchsorted(xs, zs, side="right")
    return a, b


def dot(u, v, chunk=1 << 14):
    """sum u v as a python integer; u, v int64 in [0, 2^33).  Each factor is split in 16-bit halves (the top one < 2^17): a product
    is < 2^34 and a chunk of 2^14 of them sums below 2^48."""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    pad = (-len(u)) % chunk
    if pad:
        u, v = np.concatenate([u, np.zeros(pad, np.int64)]), np.concatenate([v, np.zeros(pad, np.int64)])
    u, v = u.reshape(-1, chunk), v.reshape(-1, chunk)
    total = 0
    for i, ui in enumerate((u & 0xFFFF, u >> 16)):
        for j, vj in enumerate((v & 0xFFFF, v >> 16)):
            total += sum(int(p) for p in (ui * vj).sum(axis=1)) << (16 * (i + j))
    return total


def isum(u):
    return sum(int(p) for p in np.add.reduceat(np.asarray(u, dtype=np.int64), np.arange(0, len(u), 1 << 20))) if len(u) else 0


def _bad_status(s, y, pos_cap):
    """1..4 as ggad_rank_wide_f32 states them, else 0."""
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
    return 0


def _terms(num10, num01, m, n):
    """(positive-side, negative-side) Fractions of a pair of numerators."""
    return Fraction(num10, 4 * n * n * m * m * (m - 1)), Fraction(num01, 4 * m * m * n * n * (n - 1))


def single(s, y, pos_cap=None):
    """dict(status, m, n, S1, S2, T2, N10, N01, sums = the ten limb words and two zeros, auc, var, v10, v01 as Fractions or None)."""
    status = _bad_status(s, y, pos_cap)
    if status:
        return dict(status=status, sums=[0] * 12, var=None)
    a, b = placements(s, y)
    m, n = len(a), len(b)
    S1, S2, T2 = isum(a), dot(a, a), dot(b, b)
    assert isum(b) == S1
    N10, N01 = m * S2 - S1 * S1, n * T2 - S1 * S1
    out = dict(status=0, m=m, n=n, S1=S1, S2=S2, T2=T2, N10=N10, N01=N01, sums=limbs([S1, S2, T2, N10, N01], 12),
               auc=Fraction(S1, 2 * m * n), var=None, v10=None, v01=None)
    if m < 2 or n < 2:
        out["status"] = 6
        return out
    out["v10"], out["v01"] = _terms(N10, N01, m, n)
    out["var"] = out["v10"] + out["v01"]
    return out


def pair(sa, sb, y, pos_cap=None):
    """dict(status, the ten integers, sums = the twenty limb words and four zeros, var_a, var_b, cov, cov10, cov01, var_diff, diff as
    Fractions or None)."""
    status = _bad_status(sa, y, pos_cap) or _bad_status(sb, y, pos_cap)
    if status:
        return dict(status=status, sums=[0] * 24)
    aa, ba = placements(sa, y)
    ab, bb = placements(sb, y)
    m, n = len(aa), len(ba)
    S1A, S1B = isum(aa), isum(ab)
    S2A, S2B, C10 = dot(aa, aa), dot(ab, ab), dot(aa, ab)
    T2A, T2B, C01 = dot(ba, ba), dot(bb, bb), dot(ba, bb)
    D = S1A - S1B
    ND10, ND01 = m * (S2A + S2B - 2 * C10) - D * D, n * (T2A + T2B - 2 * C01) - D * D
    out = dict(status=0, m=m, n=n, S1A=S1A, S1B=S1B, S2A=S2A, S2B=S2B, C10=C10, T2A=T2A, T2B=T2B, C01=C01, ND10=ND10, ND01=ND01,
               sums=limbs([S1A, S1B, S2A, S2B, C10, T2A, T2B, C01, ND10, ND01], 24), diff=Fraction(D, 2 * m * n))
    if m < 2 or n < 2:
        out["status"] = 6
        return out
    out["var_a"] = sum(_terms(m * S2A - S1A * S1A, n * T2A - S1A * S1A, m, n))
    out["var_b"] = sum(_terms(m * S2B - S1B * S1B, n * T2B - S1B * S1B, m, n))
    out["cov10"], out["cov01"] = _terms(m * C10 - S1A * S1B, n * C01 - S1A * S1B, m, n)
    out["cov"] = out["cov10"] + out["cov01"]
    out["var_diff"] = sum(_terms(ND10, ND01, m, n))
    if ND10 == 0 and ND01 == 0:
        out["status"] = 7
    return out


def limbs(values, words):
    """lo, hi of each non-negative integer as signed int64 words, zero-padded to `words`."""
    out = []
    for v in values:
        assert 0 <= v < 1 << 128
        out += [_signed(v & (2 ** 64 - 1)), _signed(v >> 64)]
    return out + [0] * (words - len(out))


def _signed(w):
    return w - 2 ** 64 if w >= 2 ** 63 else w


def brute(s, y):
    """(auc, var) as Fractions by the definition: psi(x, y) = 1, 1/2, 0 for x >, ==, < y; V10_i and V01_j its means over the other
    class; var = S10 / m + S01 / n with the unbiased sample variances.  var is None when m < 2 or n < 2."""
    s, y = fold(s), np.asarray(y)
    x, z = [float(v) for v in s[y == 1]], [float(v) for v in s[y == 0]]
    m, n = len(x), len(z)
    half = Fraction(1, 2)
    psi = [[Fraction(1) if xi > zj else (half if xi == zj else Fraction(0)) for zj in z] for xi in x]
    v10 = [sum(row) / n for row in psi]
    v01 = [sum(psi[i][j] for i in range(m)) / m for j in range(n)]
    theta = sum(v10) / m
    if m < 2 or n < 2:
        return theta, None
    s10 = sum((v - theta) ** 2 for v in v10) / (m - 1)
    s01 = sum((v - theta) ** 2 for v in v01) / (n - 1)
    return theta, s10 / m + s01 / n


def brute_cov(sa, sb, y):
    """The covariance of the two AUROCs by the same definition (m, n >= 2)."""
    y = np.asarray(y)
    out = []
    for s in (sa, sb):
        s = fold(s)
        x, z = [float(v) for v in s[y == 1]], [float(v) for v in s[y == 0]]
        m, n = len(x), len(z)
        half = Fraction(1, 2)
        psi = [[Fraction(1) if xi > zj else (half if xi == zj else Fraction(0)) for zj in z] for xi in x]
        out.append(([sum(row) / n for row in psi], [sum(psi[i][j] for i in range(m)) / m for j in range(n)]))
    (va10, va01), (vb10, vb01) = out
    ta, tb = sum(va10) / m, sum(vb10) / m
    c10 = sum((p - ta) * (q - tb) for p, q in zip(va10, vb10)) / (m - 1)
    c01 = sum((p - ta) * (q - tb) for p, q in zip(va01, vb01)) / (n - 1)
    return c10 / m + c01 / n
