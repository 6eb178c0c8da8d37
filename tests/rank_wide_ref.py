"""The cases of `ggad_rank_wide_f32` (csrc/rank_metrics.hip): the smallest inputs at which each branch of the tiled kernels can go wrong.
The formulas are those of tests/rank_metrics_ref.py, imported: this file holds cases only.  Each case is (name, scores float32,
labels uint8, thres), seeded.  tests/test_rank_wide_cpu.py holds the list against scikit-learn; tests/test_rank_wide_gpu.py holds the
kernels against the formulas on it."""
import functools

import numpy as np

import rank_metrics_ref as RM

TILE = 8192


def _rand(rng, n, p):                      # n scores, exactly p positives at random places
    y = np.zeros(n, dtype=np.uint8)
    y[rng.choice(n, p, replace=False)] = 1
    return rng.random(n).astype(np.float32), y


@functools.lru_cache(maxsize=None)
def cases():
    """Built once per process and shared: nobody writes into the arrays."""
    rng = np.random.default_rng(21)
    out = list(RM.cases(TILE))                                                   # the wide route answers the narrow cases too
    out.append(("p8193", *_rand(rng, 8193 + 3000, 8193), 0.5))                   # the second tile holds one key
    out.append(("p16384", *_rand(rng, 16384 + 3000, 16384), 0.5))                # the tile edge
    out.append(("p16385", *_rand(rng, 16385 + 3000, 16385), 0.5))                # three tiles: a merge pass with an unpaired run
    out.append(("p24581", *_rand(rng, 3 * TILE + 5 + 3000, 3 * TILE + 5), 0.5))
    out.append(("five_tiles", *_rand(rng, 70000, 40000), 0.5))
    out.append(("lone_negative", *_rand(rng, 20001, 20000), 0.5))
    s, y = _rand(rng, 30000, 20000)
    out.append(("heavy_ties", (np.floor(s * 5) / 5).astype(np.float32), y, 0.4))  # runs of thousands of equal positives cross tile edges
    out.append(("all_tied", np.full(12000, 0.5, dtype=np.float32), _rand(rng, 12000, 9000)[1], 0.5))
    s, y = _rand(rng, 40000, 20000)
    out.append(("quantised", (np.floor(s * 4096) / 4096).astype(np.float32), y, 0.5))   # many negatives equal positives
    # a run of equal positives across the edge of tile 0, negatives on it, beside it, below and above everything
    p = 16390
    pos = (np.arange(1, p + 1, dtype=np.float64) / 32768).astype(np.float32)     # distinct, ascending
    v = pos[8190]
    before, after = pos[8189], pos[8196]
    pos[8190:8196] = v
    neg = np.concatenate([np.full(50, x, dtype=np.float32) for x in (v, before, after, np.float32(-1.0), np.float32(2.0))])
    s = np.concatenate([pos, neg])
    y = np.concatenate([np.ones(p, dtype=np.uint8), np.zeros(len(neg), dtype=np.uint8)])
    order = rng.permutation(len(s))
    out.append(("boundary_run", s[order], y[order], 0.25))
    s, y = _rand(rng, 9000 + 2500, 9000)
    s = s - np.float32(0.5)
    s[::4] = np.float32(-0.0)
    s[1::4] = np.float32(0.0)
    out.append(("signed_zero", s.astype(np.float32), y, 0.0))
    s, y = _rand(rng, 9000 + 2500, 9000)
    s[::7] = np.inf
    s[3::11] = -np.inf
    out.append(("infinity", s, y, 0.5))
    out.append(("dgraph_like", *_rand(rng, 1736598, 8313), 0.5))                 # every range of the scan loops: the shape this is for
    out.append(("at_wide_cap", *_rand(rng, (1 << 20) + 3000, 1 << 20), 0.5))
    names = [c[0] for c in out]
    names = [n if names.index(n) == i else n + "_wide" for i, n in enumerate(names)]     # (lone_negative, heavy_ties, ... come twice)
    out = [(n, *c[1:]) for n, c in zip(names, out)]
    for c in out:
        c[1].setflags(write=False)
        c[2].setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(auroc as the float of the exact fraction, AP by fsum, sklearn's auroc, sklearn's AP, confusion, P) of a case, computed once."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    _, s, y, thres = next(c for c in cases() if c[0] == name)
    sk = RM.finite_image(s)
    return (float(RM.auroc_fraction(s, y)), RM.average_precision(s, y), float(roc_auc_score(y, sk)),
            float(average_precision_score(y, sk)), RM.confusion(s, y, thres), int(y.sum()))
