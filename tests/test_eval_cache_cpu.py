"""Config key `eval_cache` and the counting formulas of the rank metrics, without a GPU.

  1. the two `ValueError`s of the switch (`ModelHandler.__init__`): another model, a `torch.distributed` world above 1;
  2. `src/dgraph.yml` still loads and the key defaults to false;
  3. tests/rank_metrics_ref.py (the numpy restatement the GPU tests hold the kernels against) against scikit-learn over random and
     tied inputs and over the edge cases of the GPU test."""
import math
import os

import numpy as np
import pytest
from sklearn.metrics import average_precision_score, confusion_matrix, roc_auc_score

from conftest import ROOT
import rank_metrics_ref as RM


def test_eval_cache_with_another_model_is_a_config_error():
    from ggad_amd.model_handler import ModelHandler
    cfg = dict(data_name="synthetic", data_dir="", seed=72, eval_cache=True)
    for model in ("SAGE", "PCGNN"):
        with pytest.raises(ValueError, match="eval_cache.*GCN"):
            ModelHandler(dict(cfg, model=model))
    with pytest.raises(ValueError, match="data_name"):                     # with model 'GCN' the check passes (and the loader objects)
        ModelHandler(dict(cfg, model="GCN"))
    with pytest.raises(ValueError, match="data_name"):                     # key off: nothing to check
        ModelHandler(dict(cfg, model="SAGE", eval_cache=False))


def test_eval_cache_under_a_distributed_world_is_a_config_error(monkeypatch):
    import torch
    from ggad_amd.model_handler import ModelHandler
    cfg = dict(data_name="synthetic", data_dir="", seed=72, model="GCN", eval_cache=True)
    monkeypatch.setattr(torch.distributed, "is_available", lambda: True)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError, match="eval_cache.*one GPU"):
        ModelHandler(cfg)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 1)
    with pytest.raises(ValueError, match="data_name"):                     # a world of one is a single GPU
        ModelHandler(cfg)


def test_dgraph_yml_loads_and_the_key_is_off():
    import yaml
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["eval_cache"] is False
    assert cfg["model"] == "GCN" and cfg["valid_epochs"] == 5 and cfg["batch_size"] == 150


def _against_sklearn(name, s, y, thres):
    auc = float(RM.auroc_fraction(s, y))
    ap = RM.average_precision(s, y)
    sk = RM.finite_image(s)                                                 # (scikit-learn refuses +-inf; the image keeps order and ties)
    assert abs(auc - roc_auc_score(y, sk)) <= 1e-12, name
    assert abs(ap - average_precision_score(y, sk)) <= 1e-12, name
    tp, fp, fn, tn = RM.confusion(s, y, thres)
    pred = (s >= np.float32(thres)).astype(np.int64)
    assert (tn, fp, fn, tp) == tuple(int(v) for v in confusion_matrix(y, pred, labels=[0, 1]).ravel()), name


def test_counting_formulas_against_sklearn_random_and_tied():
    rng = np.random.default_rng(7)
    worst = 0.0
    for it in range(300):
        n = int(rng.integers(2, 400))
        y = (rng.random(n) < rng.uniform(0.05, 0.6)).astype(np.uint8)
        y[0], y[1] = 0, 1
        s = rng.random(n).astype(np.float32)
        if it % 2:
            s = (np.floor(s * int(rng.integers(1, 8))) / 8).astype(np.float32)          # heavy ties
        _against_sklearn(f"random {it}", s, y, 0.4)
        worst = max(worst, abs(float(RM.auroc_fraction(s, y)) - roc_auc_score(y, s)), abs(RM.average_precision(s, y) - average_precision_score(y, s)))
    print(f"\n[rank_metrics_ref vs sklearn] largest difference over 300 cases: {worst:.3g}")


@pytest.mark.parametrize("case", RM.cases(8192), ids=lambda c: c[0])
def test_counting_formulas_against_sklearn_on_the_edge_cases(case):
    _against_sklearn(*case)


def test_average_precision_without_positives_is_zero():
    assert RM.average_precision(np.array([0.1, 0.2], dtype=np.float32), np.array([0, 0])) == 0.0
    assert math.isclose(RM.average_precision(np.array([0.1, 0.2], dtype=np.float32), np.array([1, 1])), 1.0)
