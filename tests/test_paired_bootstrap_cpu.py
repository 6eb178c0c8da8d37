"""tests/paired_bootstrap_ref.py, the reference of `ggad_rank_bootstrap_pair_f32`, on the CPU: its replicates against scikit-learn
under ONE weight vector per replicate shared by both models (the draw counts per element: that is the pairing), two equal lists, and
the paired bootstrap's standard error of the AUROC difference against DeLong's paired one."""
import math

import numpy as np
import pytest

import delong_ref as DL
import paired_bootstrap_ref as PR
import rank_metrics_ref as RM
from bootstrap_ref import fold
from test_bootstrap_cpu import _cases

SEED = 0x1234_5678_9ABC_DEF0


def _second(s):
    """Another model's scores of the same elements with the ties, zeros and infinities of `s`: the list read backwards."""
    return np.ascontiguousarray(np.asarray(s)[::-1])


@pytest.mark.parametrize("name", [c[0] for c in _cases()])
def test_replicates_against_sklearn_with_shared_weights(name):
    from sklearn.metrics import average_precision_score, roc_auc_score
    _, sa, y = next(c for c in _cases() if c[0] == name)
    sb = _second(sa)
    images = (RM.finite_image(fold(sa)), RM.finite_image(fold(sb)))
    b = PR.bootstrap(sa, sb, y, SEED, 6)
    P, Nn = b["P"], b["Nn"]
    worst = 0.0
    for r in range(6):
        j, u = PR.drawn(SEED, r, P, Nn)
        wt = PR.element_counts(y, j, u)                                            # one vector for both models
        assert wt[np.asarray(y) == 1].sum() == P and wt[np.asarray(y) != 1].sum() == Nn
        for m in range(2):
            w, c_u, c_e = b["hist"][r, m]
            assert w.sum() == P and c_u.sum() == Nn and (c_e[:-1] <= c_u[1:]).all() and c_e[-1] == 0 and w[-1] == 0
            ap = average_precision_score(y, images[m], sample_weight=wt)
            auc = roc_auc_score(y, images[m], sample_weight=wt)
            worst = max(worst, abs(ap - b["ap"][m, r]), abs(auc - b["auc"][m, r]))
    print(f"[{name}] worst |reference - sklearn| over 6 replicates and both models: {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", [c[0] for c in _cases()])
def test_the_same_list_twice_differs_by_exactly_zero(name):
    _, s, y = next(c for c in _cases() if c[0] == name)
    b = PR.bootstrap(s, s.copy(), y, SEED, 6)
    assert (b["ap"][0] - b["ap"][1] == 0.0).all() and (b["num"][0] == b["num"][1]).all() and (b["hist"][:, 0] == b["hist"][:, 1]).all()
    assert PR.p_value(b["ap"][0] - b["ap"][1]) == 1.0


def test_p_value():
    assert PR.p_value([1.0, 2.0, 3.0]) == 2 * 1 / 4 and PR.p_value([-1.0, 2.0, 3.0, 4.0]) == 2 * 2 / 5
    assert PR.p_value([0.0, 0.0]) == 1.0 and PR.p_value([-1.0, 1.0]) == 1.0


def test_paired_standard_error_against_delong():
    """4,000 scores, 200 positives, two correlated models, B = 512 Philox replicates with seed 0.  The band [0.8, 1.25] is that of
    test_bootstrap_cpu.py::test_bootstrap_standard_error_against_delong, for its reason.  Measured on the CPU: paired bootstrap se of
    the AUROC difference 0.016833 / DeLong's paired se 0.016740 = 1.0055, and sqrt(var_a + var_b) = 0.0270 is 1.60 times the
    bootstrap's: a bootstrap that lost its pairing would sit there and fail the second assertion."""
    rng = np.random.default_rng(2024)
    n = 4000
    y = np.zeros(n, dtype=np.uint8)
    y[rng.choice(n, 200, replace=False)] = 1
    z = rng.standard_normal(n)
    sa = (z + y).astype(np.float32)
    sb = (0.7 * z + 0.7 * rng.standard_normal(n) + 0.8 * y).astype(np.float32)
    b = PR.bootstrap(sa, sb, y, 0, 512, keep_hist=False)
    d = DL.pair(sa, sb, y)
    se = float((b["auc"][0] - b["auc"][1]).std(ddof=1))
    paired, unpaired = math.sqrt(float(d["var_diff"])), math.sqrt(float(d["var_a"]) + float(d["var_b"]))
    print(f"[paired boot/delong] bootstrap se {se!r} DeLong paired se {paired!r} ratio {se / paired:.4f}; unpaired {unpaired!r} "
          f"ratio {unpaired / se:.4f}")
    assert 0.8 <= se / paired <= 1.25
    assert unpaired / se > 1.25
