"""Top-k ranking (csrc/topk.hip, `metrics.top_k`, config keys `top_k` / `top_k_out`), the parts that need no GPU:

  1. tests/topk_ref.py (the numpy statement the GPU tests hold the kernels against) against a brute-force python sort by
     (-score, position) on its small cases;
  2. `precision_recall_at` on hand-made `Ranked` values;
  3. the four `ValueError`s of the config keys (`ModelHandler.__init__`): another model, `top_k_out` without `top_k`, K above the
     cap, a `torch.distributed` world above 1 -- all raised before anything touches a GPU;
  4. the binding holds the three entry points; the cap and the workspace size answer without a GPU; `src/dgraph.yml` carries the keys,
     off."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import topk_ref as TK


def _cap():
    from ggad_amd import _lib
    return int(_lib.load().ggad_topk_max_k())


# ------------------------------------------------------------------ 1: the reference
def _brute(s, y, k):
    idx = sorted(range(len(s)), key=lambda i: (-float(s[i]), i))[:k]          # (-(-0.0) == 0.0 in python too; inf compares fine)
    cum, run = [], 0
    for i in idx:
        run += int(y[i] == 1)
        cum.append(run)
    left = 0
    if idx:
        last = float(s[idx[-1]])
        left = sum(1 for v in s if float(v) == last) - sum(1 for i in idx if float(s[i]) == last)
    return idx, cum, left


@pytest.mark.parametrize("case", [c for c in TK.cases(16384) if len(c[1]) <= 5000], ids=lambda c: c[0])
def test_reference_against_a_brute_force_sort(case):
    name, s, y, k = case
    r = TK.reference(s, y, k)
    idx, cum, left = _brute(s, y, k)
    assert r["m"] == min(k, len(s)) == len(idx)
    assert r["pos"].tolist() == idx and r["cum_pos"].tolist() == cum
    assert np.array_equal(r["score"].view(np.int32), s[idx].view(np.int32))
    assert (r["n_pos"], r["tied_left_out"]) == (int(y.sum()), left)
    if name == "all_tied":
        assert idx == list(range(700)) and left == 800
    if name == "tie_across_ranges":
        tied = [i for i in idx if s[i] == np.float32(0.75)]
        assert len(tied) == 47 and sorted({i // 1000 for i in tied}) == [0, 1, 2] and left == 53
    if name in ("infinity", "signed_zero", "saturated_small", "minus_infinity"):
        assert left > 0                                                      # the cut falls inside the tie it is meant to hit
    pos, score, cum_k = TK.padded(r, k)
    assert len(pos) == len(score) == len(cum_k) == k
    assert (pos[r["m"]:] == -1).all() and (score[r["m"]:] == 0).all() and (cum_k[r["m"]:] == (cum[-1] if cum else 0)).all()


def test_reference_without_labels():
    s = np.array([0.5, 0.9, 0.5, 0.1], dtype=np.float32)
    r = TK.reference(s, None, 3)
    assert r["pos"].tolist() == [1, 0, 2] and r["cum_pos"].tolist() == [0, 0, 0] and r["n_pos"] == 0 and r["tied_left_out"] == 0
    assert TK.reference(s, None, 2)["tied_left_out"] == 1


# ------------------------------------------------------------------ 2: precision / recall
def test_precision_recall_at_on_hand_made_rankings():
    from ggad_amd.metrics import Ranked, precision_recall_at
    r = Ranked(pos=torch.tensor([4, 0, 2, 9], dtype=torch.int32), ids=torch.tensor([14, 10, 12, 19]),
               scores=torch.tensor([0.9, 0.8, 0.8, 0.1]), cum_pos=torch.tensor([1, 1, 2, 2], dtype=torch.int32), m=4, n_pos=5,
               tied_left_out=0)
    assert precision_recall_at(r, 1) == (1.0, 1 / 5)
    assert precision_recall_at(r, 2) == (1 / 2, 1 / 5)
    assert precision_recall_at(r, 3) == (2 / 3, 2 / 5)
    assert precision_recall_at(r, 4) == (2 / 4, 2 / 5)
    for j in (0, 5, -1):
        with pytest.raises(ValueError, match="outside 1..m"):
            precision_recall_at(r, j)
    none = Ranked(pos=r.pos, ids=r.ids, scores=r.scores, cum_pos=torch.zeros(4, dtype=torch.int32), m=4, n_pos=0, tied_left_out=3)
    p, rec = precision_recall_at(none, 4)
    assert p == 0.0 and math.isnan(rec)
    unlabelled = Ranked(pos=r.pos, ids=r.ids, scores=r.scores, cum_pos=None, m=4, n_pos=0, tied_left_out=0)
    with pytest.raises(ValueError, match="labels"):
        precision_recall_at(unlabelled, 1)


# ------------------------------------------------------------------ 3: the config keys
BASE = dict(data_name="synthetic", data_dir="", seed=72)


def test_top_k_with_another_model_is_a_config_error():
    from ggad_amd.model_handler import ModelHandler
    for model in ("SAGE", "PCGNN"):
        for extra in (dict(top_k=10), dict(top_k=10, top_k_out="r.npz")):
            with pytest.raises(ValueError, match="top_k.*model: 'GCN'"):
                ModelHandler(dict(BASE, model=model, **extra))
        with pytest.raises(ValueError, match="data_name"):                   # keys off: the constructor goes on to the loader
            ModelHandler(dict(BASE, model=model, top_k=0, top_k_out=""))


def test_top_k_out_without_top_k_is_a_config_error():
    from ggad_amd.model_handler import ModelHandler
    with pytest.raises(ValueError, match="top_k_out.*top_k"):
        ModelHandler(dict(BASE, model="GCN", top_k=0, top_k_out="r.npz"))
    with pytest.raises(ValueError, match="top_k_out.*top_k"):
        ModelHandler(dict(BASE, model="GCN", top_k_out="r.npz"))


def test_top_k_above_the_cap_is_a_config_error():
    from ggad_amd.model_handler import ModelHandler
    cap = _cap()
    for k in (cap + 1, -3):
        with pytest.raises(ValueError, match=r"ggad_topk_max_k\(\)"):
            ModelHandler(dict(BASE, model="GCN", top_k=k))
    with pytest.raises(ValueError, match="data_name"):                       # the cap itself is legal
        ModelHandler(dict(BASE, model="GCN", top_k=cap))


def test_top_k_under_a_distributed_world_is_a_config_error(monkeypatch):
    from ggad_amd.model_handler import ModelHandler
    cfg = dict(BASE, model="GCN", top_k=100)
    monkeypatch.setattr(torch.distributed, "is_available", lambda: True)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError, match="top_k.*one GPU"):
        ModelHandler(cfg)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 1)
    with pytest.raises(ValueError, match="data_name"):                       # a world of one is a single GPU
        ModelHandler(cfg)


# ------------------------------------------------------------------ 4: binding, cap, workspace, yml
def test_the_binding_holds_the_three_entry_points():
    from ggad_amd import _lib
    for name in ("ggad_topk_max_k", "ggad_topk_workspace_elems", "ggad_topk_f32"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ggad_topk_f32"][1]) == 10                    # nine arguments and the stream
    lib = _lib.load()
    cap = int(lib.ggad_topk_max_k())
    assert cap >= 8192
    assert lib.ggad_topk_workspace_elems(0, 1) > 0 and lib.ggad_topk_workspace_elems(2 ** 31 - 1, cap) > 0
    assert lib.ggad_topk_workspace_elems(1000, 100) < lib.ggad_topk_workspace_elems(1000000, 100)
    for n, k in ((-1, 5), (2 ** 31, 5), (100, 0), (100, cap + 1), (100, -1)):
        assert lib.ggad_topk_workspace_elems(n, k) == 0
    # out of bounds: refused before any launch (no GPU is needed to be told so)
    assert lib.ggad_topk_f32(1, None, 10, 0, 1, 1, None, 1, 1, None) == -1
    assert lib.ggad_topk_f32(1, None, 10, cap + 1, 1, 1, None, 1, 1, None) == -1
    assert lib.ggad_topk_f32(None, None, 10, 5, 1, 1, None, 1, 1, None) == -1


def test_top_k_argument_checks_need_no_gpu():
    from ggad_amd.metrics import top_k
    with pytest.raises(ValueError, match="float32"):
        top_k(torch.zeros(4, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="GPU"):
        top_k(torch.zeros(4), 2)


def test_dgraph_yml_carries_the_keys_off():
    import yaml
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["top_k"] == 0 and cfg["top_k_out"] == ""
