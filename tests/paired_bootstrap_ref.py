"""The reference of `ggad_rank_bootstrap_pair_f32` (csrc/rank_metrics.hip; the scheme is stated in include/ggad_hip.h), numpy on the
host, on tests/bootstrap_ref.py's `philox4x32_10`, `draws`, `bins` and `terms`.

A replicate draws ELEMENTS: positive numbers (the j-th element with label 1 in position order) on stream 0, negative numbers (the
u-th with label 0) on stream 1; `tables` gives, per model, where each numbered element falls -- the positive's lower-bound rank in
the model's sorted positives, the negative's `ub` and `tie` --, `replicate` bins one replicate's draws into one model's (w, cU, cE)
and `element_counts` says how often each element of the list was drawn, which is the `sample_weight` both models share.
tests/test_paired_bootstrap_cpu.py holds this against scikit-learn and DeLong; tests/test_paired_bootstrap_gpu.py holds the kernels
against it."""
import numpy as np

import bootstrap_ref as BR

MAX_POS, MAX_REPS, TOO_FEW, TOO_MANY = BR.MAX_POS, BR.MAX_REPS, BR.TOO_FEW, BR.TOO_MANY


def tables(s, y):
    """dict(pos, rank[P] by positive number, ub[Nn], tie[Nn] by negative number, P, Nn) of one model."""
    s, y = BR.fold(s), np.asarray(y)
    pos, _, _, _, ub, tie = BR.bins(s, y)
    rank = np.searchsorted(pos, s[np.flatnonzero(y == 1)], side="left").astype(np.int64)
    return dict(pos=pos, rank=rank, ub=ub, tie=np.asarray(tie, dtype=bool), P=len(pos), Nn=len(ub))


def drawn(seed, rep, P, Nn):
    """(positive numbers, negative numbers) of replicate `rep`: the same for every model."""
    return BR.draws(seed, rep, 0, P, P), BR.draws(seed, rep, 1, Nn, Nn)


def replicate(T, j, u):
    """(w, cU, cE), each int64[P + 1], of the drawn numbers (j, u) under the model of `T`."""
    P = T["P"]
    w = np.bincount(T["rank"][j], minlength=P + 1).astype(np.int64)
    ub = T["ub"][u]
    c_u = np.bincount(ub, minlength=P + 1).astype(np.int64)
    c_e = np.bincount(ub[T["tie"][u]] - 1, minlength=P + 1).astype(np.int64)
    return w, c_u, c_e


def element_counts(y, j, u):
    """How often each element of the list was drawn (float64[n]): scikit-learn's `sample_weight` of the replicate, for both models."""
    y = np.asarray(y)
    out = np.zeros(len(y), dtype=np.float64)
    np.add.at(out, np.flatnonzero(y == 1)[j], 1.0)
    np.add.at(out, np.flatnonzero(y != 1)[u], 1.0)
    return out


def status_of(sa, sb, y, pos_cap=None):
    """out24[23]: the first non-zero chain status, 8, 9, else 0."""
    for s in (sa, sb):
        st = BR.status_of(s, y, pos_cap)
        if st in (1, 2, 3, 4):
            return st
    p = int((np.asarray(y) == 1).sum())
    if p < 2 or len(y) - p < 2:
        return TOO_FEW
    return TOO_MANY if p > MAX_POS else 0


def bootstrap(sa, sb, y, seed, reps, which=None, keep_hist=True):
    """dict(P, Nn, ap float64[2, reps], num int64[2, reps], auc float64[2, reps], hist int64[reps, 2, 3, P + 1] or None); model A is
    index 0.  `which`: the replicates to make (the others stay NaN / 0)."""
    T = (tables(sa, y), tables(sb, y))
    P, Nn = T[0]["P"], T[0]["Nn"]
    ap, num = np.full((2, reps), np.nan), np.zeros((2, reps), dtype=np.int64)
    hist = np.zeros((reps, 2, 3, P + 1), dtype=np.int64) if keep_hist else None
    for r in (range(reps) if which is None else which):
        j, u = drawn(seed, r, P, Nn)
        for m in range(2):
            h = replicate(T[m], j, u)
            ap[m, r], num[m, r] = BR.terms(T[m]["pos"], *h)
            if keep_hist:
                hist[r, m] = h
    return dict(P=P, Nn=Nn, ap=ap, num=num, auc=num.astype(np.float64) / float(2 * P * Nn), hist=hist)


def p_value(d):
    """The two-sided bootstrap p-value of replicate differences d: min(1, 2 min((1 + #{d <= 0}) / (B + 1), (1 + #{d >= 0}) / (B + 1)))."""
    d = np.asarray(d)
    B = len(d)
    return min(1.0, 2.0 * min((1 + int((d <= 0).sum())) / (B + 1), (1 + int((d >= 0).sum())) / (B + 1)))


def summary(d, level):
    """(lo, hi, se) of replicate differences, as `metrics.compare_ap` states them."""
    d = np.asarray(d, dtype=np.float64)
    lo, hi = np.quantile(d, [(1 - level) / 2, (1 + level) / 2])
    return float(lo), float(hi), float(d.std(ddof=1)) if len(d) > 1 else float("nan")
