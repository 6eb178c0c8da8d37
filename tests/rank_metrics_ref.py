"""Numpy restatement of the counting formulas behind `ggad_rank_metrics_f32` (csrc/rank_metrics.hip): AUROC, average precision
and the confusion counts of `score >= thres` from float32 scores and 0/1 labels, with scikit-learn's definitions (distinct
thresholds, tied scores) as exact integer counts.  With P positives, Nn negatives and pos[] the sorted positive scores,

    L_k = negatives with score <  pos[k]      E_k = negatives with score == pos[k]      G_k = positives with score >= pos[k]
    AUROC = sum_k (2 L_k + E_k) / (2 P Nn)                       (an exact fraction)
    AP    = (1 / P) sum_k G_k / (G_k + Nn - L_k)

tests/test_eval_cache_cpu.py holds this against sklearn; tests/test_eval_cache_gpu.py holds the kernels against this."""
import math
from fractions import Fraction

import numpy as np


def counts(scores, labels):
    """(L, E, G, P, Nn): int64 arrays over the positives in ascending score order."""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels)
    pos = np.sort(s[y == 1])
    neg = np.sort(s[y != 1])
    L = np.searchsorted(neg, pos, side="left").astype(np.int64)                  # (-0.0 == +0.0 for searchsorted, as for sklearn)
    E = np.searchsorted(neg, pos, side="right").astype(np.int64) - L
    G = len(pos) - np.searchsorted(pos, pos, side="left").astype(np.int64)
    return L, E, G, len(pos), len(neg)


def auroc_fraction(scores, labels) -> Fraction:
    L, E, _, P, Nn = counts(scores, labels)
    return Fraction(int((2 * L + E).sum()), 2 * P * Nn)


def ap_terms(scores, labels):
    """The P terms G_k / (G_k + Nn - L_k) as float64."""
    L, _, G, _, Nn = counts(scores, labels)
    return G.astype(np.float64) / (G + Nn - L).astype(np.float64)


def average_precision(scores, labels) -> float:
    t = ap_terms(scores, labels)
    return math.fsum(t.tolist()) / len(t) if len(t) else 0.0


def confusion(scores, labels, thres):
    """(tp, fp, fn, tn) of `score >= float32(thres)`."""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels) == 1
    pred = s >= np.float32(thres)
    return int((pred & y).sum()), int((pred & ~y).sum()), int((~pred & y).sum()), int((~pred & ~y).sum())


def finite_image(scores):
    """The scores with +-inf replaced by finite values beyond every other score: a monotone map that keeps every tie, so every
    rank metric is unchanged (scikit-learn refuses infinite scores)."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    fin = s[np.isfinite(s)]
    lo, hi = (fin.min() - 1.0, fin.max() + 1.0) if len(fin) else (-1.0, 1.0)
    return np.where(s == np.inf, hi, np.where(s == -np.inf, lo, s))


def cases(cap: int):
    """(name, scores float32, labels uint8, thres): the smallest inputs at which each branch of the kernels can go wrong."""
    rng = np.random.default_rng(20)

    def rand(n, p):                        # n scores, exactly p positives at random places
        y = np.zeros(n, dtype=np.uint8)
        y[rng.choice(n, p, replace=False)] = 1
        return rng.random(n).astype(np.float32), y

    out = [("tiny", np.array([0.25, 0.75], dtype=np.float32), np.array([1, 0], dtype=np.uint8), 0.5)]
    for n in (63, 64, 65):
        out.append((f"n{n}", *rand(n, n // 3), 0.5))
    out.append(("lone_positive", *rand(4097, 1), 0.5))
    out.append(("lone_negative", *rand(4097, 4096), 0.5))
    for p in (1, 2, 3, 1023, 1025):
        out.append((f"pad_p{p}", *rand(3000, p), 0.4))
    out.append(("at_cap", *rand(cap + 3000, cap), 0.5))
    s, y = rand(3001, 700)
    out.append(("heavy_ties", (np.floor(s * 5) / 5).astype(np.float32), y, 0.4))
    out.append(("all_tied", np.full(1500, 0.5, dtype=np.float32), rand(1500, 300)[1], 0.5))
    s, y = rand(2049, 500)
    s[::3] = np.float32(0.4)
    out.append(("at_threshold", s, y, 0.4))
    s, y = rand(1300, 300)
    s = s - np.float32(0.5)
    s[::4] = np.float32(-0.0)
    s[1::4] = np.float32(0.0)
    out.append(("signed_zero", s.astype(np.float32), y, 0.0))
    s, y = rand(1100, 250)
    s[::7] = np.inf
    s[3::11] = -np.inf
    out.append(("infinity", s, y, 0.5))
    # the edges of the sorted runs of 2,048 keys (appended last: the cases above keep their draws from the one generator): one short
    # run, one full run, a second run of one key, three runs (an unpaired run in the first merge pass), four runs (two passes)
    for p in (2047, 2048, 2049, 4097, 6145):
        out.append((f"p{p}", *rand(p + 900, p), 0.5))
    s, y = rand(5000, 4100)
    out.append(("ties_across_runs", (np.floor(s * 3) / 3).astype(np.float32), y, 0.4))   # runs of equal keys longer than a sorted run
    return out
