"""The reference of `ggad_rank_operating_f32` (csrc/rank_metrics.hip), numpy on the host: the candidates are the distinct scores of the
positives (+-0 folded together), tp and fp of `score >= candidate` come from `searchsorted` on the sorted positives and negatives, and
the best candidate is taken as the header states it: `f1` and `gmean` by exact integer comparison, `f1_macro` in float64 by the formula
of `metrics._confusion_scores`, `precision` and `fpr` by their float64 inequality; equal values go to the higher threshold.
`brute_force` is the same choice by a loop over EVERY distinct score with python integers and `Fraction`s, for small inputs: it shows
that the positives' scores are the complete candidate set.  tests/test_operating_point_cpu.py holds one against the other,
tests/test_operating_point_gpu.py holds the kernels against `choose` and `curve`."""
from fractions import Fraction

import numpy as np

CRITERIA = ("f1", "f1_macro", "gmean", "precision", "fpr")
# the (criterion, param) pairs every case is run with
COMBOS = (("f1", None), ("f1_macro", None), ("gmean", None), ("precision", 0.9), ("precision", 0.5), ("fpr", 0.01), ("fpr", 0.0))


def fold(s):
    s = np.asarray(s, dtype=np.float32)
    return np.where(s == 0, np.float32(0.0), s)


def candidates(s, y):
    """(cand float32 ascending, tp int64, fp int64, P, Nn): the confusion counts of `score >= cand[i]`."""
    s, y = fold(s), np.asarray(y)
    pos, neg = np.sort(s[y == 1]), np.sort(s[y == 0])
    cand = np.unique(pos)
    tp = len(pos) - np.searchsorted(pos, cand, side="left")
    fp = len(neg) - np.searchsorted(neg, cand, side="left")
    return cand, tp.astype(np.int64), fp.astype(np.int64), len(pos), len(neg)


def macro_f1(tp, fp, P, Nn):
    tp, fp = np.asarray(tp, dtype=np.int64), np.asarray(fp, dtype=np.int64)
    fn, tn = P - tp, Nn - fp
    d1, d0 = 2 * tp + fp + fn, 2 * tn + fn + fp
    f1 = np.where(d1 > 0, 2.0 * tp / np.maximum(d1, 1), 0.0)
    f0 = np.where(d0 > 0, 2.0 * tn / np.maximum(d0, 1), 0.0)
    return 0.5 * (f1 + f0)


def value_from_counts(criterion, tp, fp, P, Nn):
    """out16[13] recomputed from the chosen counts, in float64."""
    fn, tn = P - tp, Nn - fp
    if criterion == "f1":
        return 2.0 * tp / (2 * tp + fp + fn)
    if criterion == "f1_macro":
        return float(macro_f1(tp, fp, P, Nn))
    if criterion == "gmean":
        return float(np.sqrt(np.float64(tp * tn) / np.float64(P * Nn)))
    return tp / P


def _exact_argmax(approx, exact_of):
    """The last (= highest threshold) index among the exact maxima; only candidates within 1e-9 of the float64 maximum are compared
    exactly."""
    near = np.flatnonzero(approx >= approx.max() - 1e-9)
    best = None
    for i in near:                                                  # ascending: >= lets a later equal value win
        v = exact_of(int(i))
        if best is None or v >= best[0]:
            best = (v, int(i))
    return best[1]


def choose(s, y, criterion, param=None, cached=None):
    """dict(thres np.float32, tp, fp, fn, tn, value, n_candidates, status) as out16[8..15] states it.  `cached`: `candidates(s, y)`."""
    cand, tp, fp, P, Nn = cached if cached is not None else candidates(s, y)
    fn, tn = P - tp, Nn - fp
    if criterion == "f1":
        i = _exact_argmax(2.0 * tp / (2 * tp + fp + fn), lambda k: Fraction(2 * int(tp[k]), int(2 * tp[k] + fp[k] + fn[k])))
    elif criterion == "gmean":
        i = _exact_argmax(tp.astype(np.float64) * tn / (float(P) * float(Nn)), lambda k: int(tp[k]) * int(tn[k]))
    elif criterion == "f1_macro":
        v = macro_f1(tp, fp, P, Nn)
        i = int(np.flatnonzero(v == v.max())[-1])
    else:
        if criterion == "precision":
            ok = tp.astype(np.float64) >= np.float64(param) * (tp + fp).astype(np.float64)
        elif criterion == "fpr":
            ok = fp.astype(np.float64) <= np.float64(param) * np.float64(Nn)
        else:
            raise ValueError(criterion)
        if not ok.any():
            return dict(thres=np.float32(np.inf), tp=0, fp=0, fn=P, tn=Nn, value=0.0, n_candidates=len(cand), status=5)
        i = int(np.flatnonzero(ok)[0])                               # ascending candidates, descending tp: the greatest recall
    t, f = int(tp[i]), int(fp[i])
    return dict(thres=np.float32(cand[i]), tp=t, fp=f, fn=P - t, tn=Nn - f, value=value_from_counts(criterion, t, f, P, Nn),
                n_candidates=len(cand), status=0)


def curve(s, y):
    """(thres float32[P], tp int64[P], fp int64[P]): entry j = the run that holds the j-th highest positive."""
    cand, tp, fp, P, _ = candidates(s, y)
    pos = np.sort(fold(s)[np.asarray(y) == 1])[::-1]
    idx = np.searchsorted(cand, pos)
    return cand[idx], tp[idx], fp[idx]


def brute_force(s, y, criterion, param=None):
    """(thres, tp, fp) or None: the best threshold among ALL distinct scores at which at least one positive alerts, python numbers
    only; equal values go to the higher threshold."""
    s, y = fold(s), np.asarray(y)
    P, Nn = int((y == 1).sum()), int((y == 0).sum())
    best = None
    for t in np.unique(s):                                           # ascending
        pred = s >= t
        tp, fp = int((pred & (y == 1)).sum()), int((pred & (y == 0)).sum())
        if tp == 0:
            continue
        fn, tn = P - tp, Nn - fp
        if criterion == "f1":
            v = Fraction(2 * tp, 2 * tp + fp + fn)
        elif criterion == "f1_macro":
            v = float(macro_f1(tp, fp, P, Nn))
        elif criterion == "gmean":
            v = tp * tn
        elif criterion == "precision":
            if not float(tp) >= param * float(tp + fp):
                continue
            v = tp
        else:
            if not float(fp) <= param * float(Nn):
                continue
            v = tp
        if best is None or v >= best[0]:
            best = (v, np.float32(t), tp, fp)
    return None if best is None else best[1:]


# ---- inputs whose labels depend on the scores (the maxima of tests/rank_wide_ref.py's cases sit at the ends)
def separable(p, n=20000, seed=5, quantise=None, saturate=False):
    """positives N(1, 1), negatives N(0, 1), shuffled; `quantise`: floor to multiples of 1 / quantise; `saturate`: the sigmoid
    1 / (1 + exp(-8 x)) in float32, thousands of scores at exactly 1.0."""
    rng = np.random.default_rng(seed)
    y = np.zeros(n, dtype=np.uint8)
    y[rng.choice(n, p, replace=False)] = 1
    x = rng.standard_normal(n) + (y == 1)
    if quantise:
        x = np.floor(x * quantise) / quantise
    x = x.astype(np.float32)
    if saturate:
        x = (np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-8.0) * x))).astype(np.float32)
    return x, y


def separable_cases():
    return (("sep_p600", *separable(600)), ("sep_p8192", *separable(8192)), ("sep_p8193", *separable(8193)),
            ("sep_p16385", *separable(16385)), ("sep_q64_p600", *separable(600, quantise=64)),
            ("sep_q64_p8193", *separable(8193, quantise=64)), ("sep_sat_p600", *separable(600, saturate=True)),
            ("sep_sat_p16385", *separable(16385, saturate=True)))


def tie_by_hand():
    """F1 1/2 at 0.9, 4/9 at 0.7, 1/2 at 0.5: the call must return 0.9 with (tp, fp) = (1, 0)."""
    s = np.array([0.9, 0.7, 0.5] + [0.8] * 4 + [0.6] * 2 + [0.1] * 100, dtype=np.float32)
    y = np.array([1, 1, 1] + [0] * 106, dtype=np.uint8)
    return s, y


def tie_by_hand_padded():
    """`tie_by_hand` below 8,191 more positives above 0.95, each followed by two negatives: the k-th highest of them has F1
    2k / (3k + 8,192) < 1/2, and with P = 8,194 and 16,382 negatives above 0.9 the three old candidates keep 1/2, < 1/2, 1/2
    (16,384 / 32,768, 16,386 / 32,773, 16,388 / 32,776).  The positives fill one tile of 8,192 and two entries of the next.
    Expected: 0.9 with (tp, fp) = (8,192, 16,382)."""
    s0, y0 = tie_by_hand()
    pad = (0.95 + 0.04 * (np.arange(1, 8192) / 8192.0))              # 8,191 distinct float32 values in (0.95, 0.99)
    below = pad - 0.04 / 16384.0                                     # two negatives under each, above the next one down
    pad32, below32 = pad.astype(np.float32), below.astype(np.float32)
    assert len(np.unique(pad32)) == 8191 and (below32 < pad32).all() and (below32[1:] > pad32[:-1]).all() and below32[0] > 0.9
    s = np.concatenate([s0, pad32, below32, below32])
    y = np.concatenate([y0, np.ones(8191, dtype=np.uint8), np.zeros(2 * 8191, dtype=np.uint8)])
    order = np.random.default_rng(3).permutation(len(s))
    return s[order], y[order]


def tie_across_sorted_tiles():
    """A G-mean tie whose two candidates sit in different tiles of the ASCENDING sorted positives (the order the kernels tile in):
    8,190 positives below 0.05 take sorted places 0..8,189, then 0.5, 0.7 | 0.9.  Negatives: four at 0.8, two at 0.3; P = 8,193,
    Nn = 6.  tp tn: 0.9 -> 1 x 6, 0.7 -> 2 x 2, 0.5 -> 3 x 2 = 6, every padding positive -> tn = 0.  Expected: 0.9, (1, 0)."""
    pad = (0.04 * np.arange(1, 8191) / 8192.0).astype(np.float32)
    assert len(np.unique(pad)) == 8190 and pad.max() < 0.05
    s = np.concatenate([np.array([0.9, 0.7, 0.5], dtype=np.float32), pad, np.array([0.8] * 4 + [0.3] * 2, dtype=np.float32)])
    y = np.concatenate([np.ones(3 + 8190, dtype=np.uint8), np.zeros(6, dtype=np.uint8)])
    order = np.random.default_rng(4).permutation(len(s))
    return s[order], y[order]
