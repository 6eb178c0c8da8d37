"""Exact rank metrics above 8,192 positives (csrc/rank_metrics.hip, `metrics.rank_report_wide`, config key `rank_wide`), without a GPU.

  1. the binding holds the three entry points; the cap is 2^20; `ggad_rank_wide_workspace_elems` is 0 for every refused argument,
     positive and non-decreasing in `n` and in `pos_cap` otherwise, and a function of the two alone; out-of-bounds calls are refused
     before any launch;
  2. `rank_report_wide` refuses CPU tensors and wrong dtypes with `rank_report`'s `ValueError`s;
  3. `rank_wide: true` without `eval_cache: true` is a config error; `src/dgraph.yml` carries the key, off;
  4. the cases of tests/rank_wide_ref.py against scikit-learn within 1e-12 by the numpy restatement: this guards the cases."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import rank_wide_ref as RW

NAMES = [c[0] for c in RW.cases()]


def test_the_binding_holds_the_three_entry_points():
    from ggad_amd import _lib
    for name in ("ggad_rank_wide_max_pos", "ggad_rank_wide_workspace_elems", "ggad_rank_wide_f32"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ggad_rank_wide_f32"][1]) == 8                 # seven arguments and the stream
    lib = _lib.load()
    assert int(lib.ggad_rank_wide_max_pos()) == 1 << 20
    assert int(lib.ggad_rank_metrics_max_pos()) == 8192                       # (the narrow cap stays where it is)
    assert _lib.ABI_VERSION == 11


def test_workspace_elems():
    from ggad_amd import _lib
    lib = _lib.load()
    cap = 1 << 20
    ws = lambda n, p: int(lib.ggad_rank_wide_workspace_elems(n, p))            # noqa: E731
    for n, p in ((-1, 5), (2 ** 31, 5), (100, 0), (100, -1), (100, cap + 1), (2 ** 31, cap + 1)):
        assert ws(n, p) == 0, (n, p)
    ns = [0, 1, 2, 63, 1023, 1024, 1025, 2048, 2049, 3071, 3073, 8192, 8193, 20000, 262143, 262144, 262145, cap, cap + 3000, 1736598,
          10 ** 7, 2 ** 31 - 1]
    assert ns == sorted(ns)
    ps = [1, 2, 520, 600, 8191, 8192, 8193, 8313, 16384, 16385, 65536, cap - 1, cap]
    table = np.array([[ws(n, p) for p in ps] for n in ns], dtype=np.int64)
    assert (table > 0).all()
    assert (np.diff(table, axis=0) >= 0).all()                                # non-decreasing in n
    assert (np.diff(table, axis=1) >= 0).all()                                # ... and in pos_cap
    assert ws(1000, 100) < ws(1000000, 100) and ws(1000000, 100) < ws(1000000, 100000)
    again = np.array([[ws(n, p) for p in ps] for n in ns], dtype=np.int64)    # a function of (n, pos_cap) alone
    assert np.array_equal(table, again)
    rng = np.random.default_rng(0)
    for _ in range(300):                                                      # dense around the places where the scan's grid grows
        n = int(rng.integers(0, 300000))
        p = int(rng.integers(1, 30000))
        assert 0 < ws(n, p) <= ws(n + 1, p) and ws(n, p) <= ws(n, p + 1), (n, p)


def test_out_of_bounds_calls_are_refused_before_any_launch():
    from ggad_amd import _lib
    lib = _lib.load()
    cap = int(lib.ggad_rank_wide_max_pos())
    assert lib.ggad_rank_wide_f32(1, 1, 10, 0, 0.5, 1, 1, None) == -1
    assert lib.ggad_rank_wide_f32(1, 1, 10, cap + 1, 0.5, 1, 1, None) == -1
    assert lib.ggad_rank_wide_f32(1, 1, -1, 5, 0.5, 1, 1, None) == -1
    assert lib.ggad_rank_wide_f32(1, 1, 2 ** 31, 5, 0.5, 1, 1, None) == -1
    assert lib.ggad_rank_wide_f32(None, 1, 10, 5, 0.5, 1, 1, None) == -1
    assert lib.ggad_rank_wide_f32(1, 1, 10, 5, 0.5, None, 1, None) == -1
    assert lib.ggad_rank_wide_f32(1, 1, 10, 5, 0.5, 1, None, None) == -1


def test_rank_report_wide_argument_checks_need_no_gpu():
    from ggad_amd.metrics import rank_report, rank_report_wide
    s, y = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    for args in ((s.double(), y), (s, y.long()), (s.view(2, 2), y.view(2, 2)), (s, y[:3]), (s, y)):      # (the last: CPU tensors)
        with pytest.raises(ValueError) as want:
            rank_report(*args, 0.5)
        with pytest.raises(ValueError) as got:
            rank_report_wide(*args, 0.5)
        assert str(got.value) == str(want.value)
        with pytest.raises(ValueError) as got:
            rank_report_wide(*args, 0.5, pos_cap=9000)
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match="float32"):
        rank_report_wide(s.double(), y, 0.5)
    with pytest.raises(ValueError, match="GPU"):
        rank_report_wide(s, y, 0.5)


def test_rank_wide_without_eval_cache_is_a_config_error():
    from ggad_amd.model_handler import ModelHandler
    cfg = dict(data_name="synthetic", data_dir="", seed=72, model="GCN")
    with pytest.raises(ValueError, match="rank_wide.*eval_cache"):
        ModelHandler(dict(cfg, rank_wide=True))
    with pytest.raises(ValueError, match="rank_wide.*eval_cache"):
        ModelHandler(dict(cfg, rank_wide=True, eval_cache=False))
    with pytest.raises(ValueError, match="data_name"):                        # both on: the check passes (and the loader objects)
        ModelHandler(dict(cfg, rank_wide=True, eval_cache=True))
    with pytest.raises(ValueError, match="data_name"):                        # key off: nothing to check
        ModelHandler(dict(cfg, rank_wide=False))


def test_dgraph_yml_carries_the_key_off():
    import yaml
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["rank_wide"] is False and cfg["eval_cache"] is False


def test_the_case_list():
    cs = RW.cases()
    assert len(set(NAMES)) == len(NAMES)
    by = {c[0]: c for c in cs}
    want_p = dict(p8193=8193, p16384=16384, p16385=16385, p24581=3 * 8192 + 5, five_tiles=40000, lone_negative_wide=20000,
                  heavy_ties_wide=20000, all_tied_wide=9000, quantised=20000, boundary_run=16390, signed_zero_wide=9000,
                  infinity_wide=9000, dgraph_like=8313, at_wide_cap=1 << 20, at_cap=8192,
                  p2047=2047, p2048=2048, p2049=2049, p4097=4097, p6145=6145, ties_across_runs=4100)
    want_n = dict(five_tiles=70000, lone_negative_wide=20001, heavy_ties_wide=30000, all_tied_wide=12000, quantised=40000,
                  dgraph_like=1736598, at_wide_cap=(1 << 20) + 3000, p8193=8193 + 3000,
                  p2047=2047 + 900, p2048=2048 + 900, p2049=2049 + 900, p4097=4097 + 900, p6145=6145 + 900, ties_across_runs=5000)
    for name, p in want_p.items():
        assert int(by[name][2].sum()) == p, name
    for name, n in want_n.items():
        assert len(by[name][1]) == n, name
    for _, s, y, _ in cs:
        assert s.dtype == np.float32 and y.dtype == np.uint8 and s.shape == y.shape and set(np.unique(y)) <= {0, 1}
    _, s, y, _ = by["boundary_run"]
    pos = np.sort(s[y == 1])
    v = pos[8190]
    assert (pos[8190:8196] == v).all() and pos[8189] < v < pos[8196] and len(np.unique(pos)) == 16390 - 5
    neg = s[y == 0]
    assert [int((neg == x).sum()) for x in (v, pos[8189], pos[8196])] == [50, 50, 50]
    assert int((neg < pos[0]).sum()) == 50 and int((neg > pos[-1]).sum()) == 50
    _, s, y, _ = by["heavy_ties_wide"]
    assert np.unique(s[y == 1], return_counts=True)[1].min() > 2000          # runs of thousands of equal positives
    _, s, y, _ = by["quantised"]
    assert np.isin(s[y == 0], s[y == 1]).mean() > 0.5                         # many negatives equal positives


@pytest.mark.parametrize("name", NAMES)
def test_the_cases_against_sklearn(name):
    auroc, ap, sk_auroc, sk_ap, conf, p = RW.expected(name)
    _, s, y, thres = next(c for c in RW.cases() if c[0] == name)
    print(f"\n[{name}] n {len(s)} P {p}: auroc - sklearn {auroc - sk_auroc:.3g}, ap - sklearn {ap - sk_ap:.3g}")
    assert abs(auroc - sk_auroc) <= 1e-12 and abs(ap - sk_ap) <= 1e-12
    assert sum(conf) == len(s) and conf[0] + conf[2] == p
