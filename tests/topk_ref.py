"""Numpy statement of the ranking behind `ggad_topk_f32` (csrc/topk.hip) and `metrics.top_k`: score descending, equal scores by
ascending position in the input, -0.0 tied with +0.0, +-inf ordinary values:

    order = np.argsort(-s.astype(np.float64), kind="stable")[:k]

and what follows from it: the running count of label-1 elements, the positives among all n, and how many elements tie with the
last rank's score but were left out.  tests/test_topk_cpu.py holds this against a brute-force python sort; tests/test_topk_gpu.py
holds the kernels against this."""
import numpy as np


def reference(scores, labels, k):
    """dict(pos int32 (m,), score float32 (m,), cum_pos int32 (m,), m, n_pos, tied_left_out); labels None: cum_pos zeros, n_pos 0."""
    s = np.asarray(scores, dtype=np.float32)
    n = len(s)
    order = np.argsort(-s.astype(np.float64), kind="stable")[:k]
    m = len(order)
    y = np.zeros(n, dtype=np.int64) if labels is None else (np.asarray(labels) == 1).astype(np.int64)
    left = 0
    if m:
        last = s[order[-1]]
        left = int((s == last).sum()) - int((s[order] == last).sum())          # (== : -0.0 equals +0.0)
    return dict(pos=order.astype(np.int32), score=s[order], cum_pos=np.cumsum(y[order]).astype(np.int32), m=m, n_pos=int(y.sum()),
                tied_left_out=left)


def padded(ref, k):
    """The k-long output arrays of the C entry point: entries m..k hold pos -1, score 0, cum_pos of the last rank (0 when m = 0)."""
    m = ref["m"]
    pos = np.full(k, -1, dtype=np.int32)
    score = np.zeros(k, dtype=np.float32)
    cum = np.full(k, ref["cum_pos"][-1] if m else 0, dtype=np.int32)
    pos[:m], score[:m], cum[:m] = ref["pos"], ref["score"], ref["cum_pos"]
    return pos, score, cum


def sigmoid32(x):
    return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)


def cases(cap: int):
    """(name, scores float32, labels uint8, k): the smallest inputs at which each branch of the kernels can go wrong.  The passes
    over the scores run min(256, ceil(n / 1024)) workgroups, each over a contiguous range of ceil(n / workgroups) positions, in
    chunks of 1,024."""
    rng = np.random.default_rng(31)

    def lab(n, p):
        y = np.zeros(n, dtype=np.uint8)
        y[rng.choice(n, p, replace=False)] = 1
        return y

    def rand(n, p):
        return rng.random(n).astype(np.float32), lab(n, p)

    out = [("n1", np.array([0.25], dtype=np.float32), np.array([1], dtype=np.uint8), 1)]
    for n in (63, 64, 65):
        out.append((f"n{n}", *rand(n, n // 3), n // 2))
    out.append(("k1", *rand(3000, 40), 1))
    out.append(("k_is_n", *rand(1300, 100), 1300))
    out.append(("k_above_n", *rand(70, 9), 200))
    out.append(("n0", np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint8), 5))
    out.append(("all_tied", np.full(1500, 0.5, dtype=np.float32), lab(1500, 300), 700))
    # n = 5,000: 5 workgroups over the ranges [0, 1000), [1000, 2000), ... .  One tie run of 100 members (0.75) at positions
    # 3, 53, 103, ...: 20 in each of the five ranges; 30 scores lie above it.  k = 30 + 47 takes the 20 ties of range 0, the 20 of
    # range 1 and the first 7 of range 2; the other 13 of range 2 and all of ranges 3 and 4 are left out (53).
    s, y = rand(5000, 120)
    s *= np.float32(0.5)
    s[3::50] = np.float32(0.75)
    free = np.setdiff1d(np.arange(5000), np.arange(3, 5000, 50))
    s[rng.choice(free, 30, replace=False)] = (0.9 + 0.1 * rng.random(30)).astype(np.float32)
    out.append(("tie_across_ranges", s, y, 77))
    # keys that share the upper 22 bits (digits 0 and 1): only the last radix pass separates them
    j = rng.permutation(900)
    out.append(("low_byte_only", (np.float32(0.5) + j.astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32), lab(900, 90), 333))
    # many exponents, negatives included: the first pass decides, and negative keys are the inverted bit patterns
    e = rng.integers(-30, 30, 2500)
    s = (np.where(rng.random(2500) < 0.5, -1.0, 1.0) * (1.0 + rng.random(2500)) * 2.0 ** e).astype(np.float32)
    out.append(("high_byte_only", s, lab(2500, 250), 1600))                  # (the cut falls among the negatives)
    s, y = rand(1300, 300)
    s = s - np.float32(0.5)
    s[::4] = np.float32(-0.0)
    s[1::4] = np.float32(0.0)
    out.append(("signed_zero", s.astype(np.float32), y, 500))                # (about 325 above zero: the cut falls among the zeros)
    s, y = rand(1100, 250)
    s[::7] = np.inf
    s[3::11] = -np.inf
    out.append(("infinity", s, y, 100))                                     # (158 +inf: the cut falls among them)
    out.append(("minus_infinity", s.copy(), y.copy(), 1050))                 # (the cut falls among the -inf at the bottom)
    # 270,000 scores: 256 ranges of 1,055 positions = two chunks each (1,024 + 31); sigmoid saturates to exactly 1.0f above ~17
    s = sigmoid32(rng.normal(0.0, 10.0, 270000))
    assert int((s == np.float32(1.0)).sum()) > 5000
    out.append(("saturated", s, lab(270000, 1350), 5000))
    s = sigmoid32(rng.normal(0.0, 10.0, 4000))
    assert 100 < int((s == np.float32(1.0)).sum()) < 4000
    out.append(("saturated_small", s, lab(4000, 40), 100))
    out.append(("at_cap", *rand(cap + 3000, 200), cap))
    out.append(("large", *rand(300000, 1500), 8192))
    return out
