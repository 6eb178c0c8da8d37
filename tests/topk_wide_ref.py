"""The cases of `ggad_topk_wide_f32` (csrc/topk.hip): the ranking is the one tests/topk_ref.py states (`reference`, `padded`); this
module adds the smallest inputs at which each branch the wide route adds can go wrong.  The candidates are sorted in runs of 2,048
(one workgroup each) and merged in ceil(log2(runs)) passes, an unpaired last run copied through; the running positives are scanned
per block of 1,024 ranks.  tests/test_topk_wide_cpu.py holds the small ones against a brute-force python sort,
tests/test_topk_wide_gpu.py holds the kernels against `padded(reference(...))`."""
import numpy as np

from topk_ref import padded, reference, sigmoid32  # noqa: F401  (re-exported: the tests take all three from here)

RUN = 2048
STATUS_ONLY = {"label_two": 4, "nan_score": 3}        # refused inputs: only the status word is specified


def cases_wide(narrow_cap: int, wide_cap: int):
    """(name, scores float32, labels uint8 or None, k).  `narrow_cap` / `wide_cap`: ggad_topk_max_k() / ggad_topk_wide_max_k()."""
    rng = np.random.default_rng(47)

    def lab(n, p):
        y = np.zeros(n, dtype=np.uint8)
        y[rng.choice(n, p, replace=False)] = 1
        return y

    def rand(n, p):
        return rng.random(n).astype(np.float32), lab(n, p)

    out = []
    # run edges: one short run, one full run, a second run of one word
    for m in (RUN - 1, RUN, RUN + 1):
        out.append((f"m{m}", *rand(m + 700, 90), m))
    # three and five runs: an unpaired last run at the first and at the second pass
    out.append(("runs3", *rand(2 * RUN + 17 + 700, 150), 2 * RUN + 17))
    out.append(("runs5", *rand(4 * RUN + 1 + 3000, 300), 4 * RUN + 1))
    # nine runs, the last one unpaired through three passes: the first k the narrow call refuses, on n = k + 3,000 and on n = k
    assert narrow_cap == 8 * RUN
    out.append(("runs9_first_wide_k", *rand(narrow_cap + 1 + 3000, 400), narrow_cap + 1))
    out.append(("k_is_n", *rand(narrow_cap + 1, 400), narrow_cap + 1))
    out.append(("k_above_n", *rand(20000, 300), 50000))
    out.append(("all_tied", np.full(40000, 0.5, dtype=np.float32), lab(40000, 900), 25000))
    # n = 70,000: 69 ranges of 1,015 positions.  1,500 scores above a block of 10,000 equal ones (0.75, every 7th position: members in
    # every range), which so holds ranks 1,500 .. 11,499 across the run edges 2,048 .. 10,240; then a block of 25,000 equal scores
    # (0.45, ranks 11,500 .. 36,499) that k = 30,000 cuts: 6,500 left out; everything else lies below 0.4
    n = 70000
    s = (rng.random(n) * 0.4).astype(np.float32)
    first = np.arange(3, n, 7)
    assert len(first) == 10000
    s[first] = np.float32(0.75)
    free = np.setdiff1d(np.arange(n), first)
    pick = rng.permutation(free)
    s[pick[:1500]] = (0.9 + 0.1 * rng.random(1500)).astype(np.float32)
    s[pick[1500:26500]] = np.float32(0.45)
    out.append(("ties_across_runs_and_cut", s, lab(n, 700), 30000))
    s = sigmoid32(rng.normal(0.0, 10.0, 270000))
    assert int((s == np.float32(1.0)).sum()) > 5000
    out.append(("saturated", s, lab(270000, 1350), 100000))
    # about 12,000 scores above zero, 1,000 of them +inf; 24,000 zeros of both signs, which k = 30,000 cuts; 1,000 -inf at the bottom
    n = 50000
    s = (rng.random(n) - 0.5).astype(np.float32)
    s[::4] = np.float32(-0.0)
    s[1::4] = np.float32(0.0)
    s[5::50] = np.inf
    s[7::50] = -np.inf
    assert int((s > 0).sum()) < 30000 < int((s >= 0).sum())
    out.append(("zeros_and_infinities", s, lab(n, 500), 30000))
    out.append(("no_labels", rng.random(23000).astype(np.float32), None, 20000))
    s, y = rand(20000, 200)
    y[777] = 2
    out.append(("label_two", s, y, 17000))
    s, y = rand(20000, 200)
    s[4242] = np.nan
    out.append(("nan_score", s, y, 17000))
    out.append(("at_cap", *rand(wide_cap + 3000, 2000), wide_cap))
    return out
