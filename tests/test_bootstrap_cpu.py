"""tests/bootstrap_ref.py, the reference of `ggad_rank_bootstrap_f32`, on the CPU: Philox against Random123's known answers, the
replicates against scikit-learn's `sample_weight`, the terms against the point estimates, the invariants of every replicate, and the
bootstrap's AUROC standard error against DeLong's."""
import functools
import math

import numpy as np
import pytest

import bootstrap_ref as BR
import delong_ref as DL
import rank_metrics_ref as RM

SEED = 0x1234_5678_9ABC_DEF0


def _words(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter, key, want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = BR.philox4x32_10(_words(counter), _words(key))
    assert [int(c[0]) for c in got] == _words(want)


def test_draw_rule():
    """Call j gives draws 2j and 2j + 1; an odd count uses half of the last call; mulhi64 is the high word of the 128-bit product."""
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 64, 1000, dtype=np.uint64)
    for m in (1, 2, 3, 9216, 1736598 - 8313, (1 << 31) - 1, (1 << 32) - 1):
        assert BR.mulhi64(x, m).tolist() == [(int(v) * m) >> 64 for v in x]
    seven, eight = BR.draws(SEED, 3, 1, 7, 1000), BR.draws(SEED, 3, 1, 8, 1000)
    assert seven.tolist() == eight[:7].tolist() and 0 <= eight.min() and eight.max() < 1000
    c = BR.philox4x32_10((2, 0, 3, 1), (SEED & 0xFFFFFFFF, SEED >> 32))
    assert int(eight[4]) == ((int(c[0][0]) | int(c[1][0]) << 32) * 1000) >> 64
    assert int(eight[5]) == ((int(c[2][0]) | int(c[3][0]) << 32) * 1000) >> 64
    assert BR.draws(SEED, 3, 0, 8, 1000).tolist() != eight.tolist() and BR.draws(SEED, 4, 1, 8, 1000).tolist() != eight.tolist()


@functools.lru_cache(maxsize=None)
def _cases():
    rng = np.random.default_rng(5)
    out = [c[:3] for c in RM.cases(8192) if c[0] in ("n63", "heavy_ties", "all_tied", "at_threshold", "signed_zero", "infinity", "pad_p2")]
    y = np.zeros(900, dtype=np.uint8)
    y[rng.choice(900, 120, replace=False)] = 1
    out.append(("quantised", (np.floor(rng.random(900) * 64) / 64).astype(np.float32), y))
    return out


@pytest.mark.parametrize("name", [c[0] for c in _cases()])
def test_replicates_against_sklearn_sample_weight(name):
    from sklearn.metrics import average_precision_score, roc_auc_score
    _, s, y = next(c for c in _cases() if c[0] == name)
    image = RM.finite_image(BR.fold(s))
    b = BR.bootstrap(s, y, SEED, 6)
    worst = 0.0
    for r in range(6):
        w, c_u, c_e = b["hist"][r]
        # the invariants of a replicate
        assert w.sum() == b["P"] and c_u.sum() == b["Nn"] and (c_e[:-1] <= c_u[1:]).all() and c_e[-1] == 0 and w[-1] == 0
        wt = BR.element_weights(s, y, w, c_u, c_e)
        assert wt[np.asarray(y) == 1].sum() == b["P"] and wt[np.asarray(y) != 1].sum() == b["Nn"]
        ap, auc = average_precision_score(y, image, sample_weight=wt), roc_auc_score(y, image, sample_weight=wt)
        worst = max(worst, abs(ap - b["ap"][r]), abs(auc - b["auc"][r]))
    print(f"[{name}] worst |reference - sklearn| over 6 replicates: {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", [c[0] for c in _cases()])
def test_unit_weights_give_the_point_estimates(name):
    _, s, y = next(c for c in _cases() if c[0] == name)
    pos, hist_u, hist_e = BR.bins(s, y)[:3]
    P, Nn = len(pos), int(hist_u.sum())
    ap, num = BR.terms(pos, np.ones(P + 1, dtype=np.int64), hist_u, hist_e)
    assert abs(ap - RM.average_precision(BR.fold(s), y)) <= 4 * 2.0 ** -53 * 2
    assert num == RM.auroc_fraction(BR.fold(s), y) * 2 * P * Nn


def test_invariants_of_many_replicates():
    _, s, y = next(c for c in _cases() if c[0] == "heavy_ties")
    b = BR.bootstrap(s, y, 7, 64)
    h = b["hist"]
    assert (h[:, 0].sum(axis=1) == b["P"]).all() and (h[:, 1].sum(axis=1) == b["Nn"]).all()
    assert (h[:, 2, :-1] <= h[:, 1, 1:]).all() and (h >= 0).all()
    assert len({tuple(r) for r in h[:, 0].tolist()}) == 64                        # no two replicates drew the same positives
    assert np.isfinite(b["ap"]).all() and ((b["auc"] >= 0) & (b["auc"] <= 1)).all()


def test_all_equal_and_separated():
    y = np.zeros(300, dtype=np.uint8)
    y[::7] = 1
    P, Nn = int(y.sum()), 300 - int(y.sum())
    b = BR.bootstrap(np.full(300, 0.25, dtype=np.float32), y, 3, 16)
    assert (b["num"] == P * Nn).all() and np.abs(b["ap"] - P / (P + Nn)).max() <= 4 * 2.0 ** -53
    b = BR.bootstrap(y.astype(np.float32) + np.linspace(0, 0.5, 300, dtype=np.float32), y, 3, 16)
    assert (b["num"] == 2 * P * Nn).all() and (b["ap"] == 1.0).all()


def test_bootstrap_standard_error_against_delong():
    """4,000 scores, 200 positives shifted by one standard deviation, B = 512 Philox replicates.  A standard error from 512
    replicates carries about 3 % noise and the two estimators differ by O(1 / sqrt(P)), so the band is [0.8, 1.25].
    Measured on the CPU with this list and Philox seed 0: bootstrap se 0.018040 / DeLong se 0.018515 = 0.974."""
    rng = np.random.default_rng(2024)
    y = np.zeros(4000, dtype=np.uint8)
    y[rng.choice(4000, 200, replace=False)] = 1
    s = (rng.standard_normal(4000) + y).astype(np.float32)
    b = BR.bootstrap(s, y, 0, 512, keep_hist=False)
    d = DL.single(s, y)
    ratio = b["auc"].std(ddof=1) / math.sqrt(float(d["var"]))
    print(f"[boot/delong] bootstrap se {b['auc'].std(ddof=1)!r} DeLong se {math.sqrt(float(d['var']))!r} ratio {ratio:.4f}")
    assert 0.8 <= ratio <= 1.25
    lo, hi, se, bias = BR.summary(float(d["auc"]), b["auc"], 0.95)
    assert lo < float(d["auc"]) < hi and abs(bias) < se
