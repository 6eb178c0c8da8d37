"""`explain` without a GPU (tests/test_explain_gpu.py runs the kernel):
  1. the four symbols of csrc/explain.hip are bound, the ABI version stays 11, the caps answer and the workspace size is monotone;
     an unsupported (D, F, m) is GGAD_E_UNSUPPORTED before anything is launched;
  2. the argument errors of `explain.explain` and of the config keys `explain` / `explain_out`; `src/dgraph.yml` carries both, off;
  3. the float64 reference of tests/explain_ref.py is complete on every fixture: per feature and per neighbour it adds up to z;
  4. the condition on the fixtures: no explained row has an undecided ReLU unit (a fixture that needed slack for a flipped unit
     would let a wrong mask through), and rows with z = 0 are among them;
  5. `write_explained` twice gives byte-equal files."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from ggad_amd import _lib
from ggad_amd import explain as E
import explain_ref as X


def test_the_symbols_are_bound_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ("ggad_explain_f32", "ggad_explain_workspace_elems", "ggad_explain_max_nbrs", "ggad_explain_lds_rows"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ggad_abi_version() == _lib.ABI_VERSION == 11
    text = open(os.path.join(ROOT, "include", "ggad_hip.h")).read()
    assert "ggad_explain_f32(" in text and "ggad_explain_workspace_elems(" in text


def test_caps_and_workspace_size():
    lib = _lib.load()
    cap, m_max = int(lib.ggad_explain_lds_rows()), int(lib.ggad_explain_max_nbrs())
    assert cap > 0 and m_max > 0
    # ids, counters and contributions of the LDS branch fit the 160 KB of a workgroup
    assert 12 * cap < 160 * 1024
    ws = lib.ggad_explain_workspace_elems
    base = int(ws(100, 10, 5))
    assert base > 0
    assert int(ws(101, 10, 5)) >= base and int(ws(100, 11, 5)) >= base and int(ws(100, 10, 6)) >= base
    assert int(ws(cap + 1, 10, 5)) > int(ws(cap, 10, 5)) and int(ws(100, 8192, 5)) > int(ws(100, 100, 5))
    # the dump of every row: two words per entry at least
    assert base >= 2 * 100 * 10
    assert int(ws(0, 10, 5)) == 0 and int(ws(100, -1, 5)) == 0 and int(ws(100, 10, 0)) == 0 and int(ws(100, 10, m_max + 1)) == 0
    assert int(ws(100, 10, m_max)) > 0


def test_an_unsupported_shape_launches_nothing():
    lib = _lib.load()
    nul = [None] * 10
    m_max = int(lib.ggad_explain_max_nbrs())
    for d, f, m in ((257, 17, 5), (0, 17, 5), (64, 1025, 5), (64, 0, 5), (64, 17, 0), (64, 17, m_max + 1)):
        assert lib.ggad_explain_f32(None, None, 10, None, None, d, f, None, 0, 1, None, 0, m, 1, *nul) == _lib.GGAD_E_UNSUPPORTED
    assert lib.ggad_explain_f32(None, None, 10, None, None, 64, 17, None, 0, 1, None, 0, 5, 1, *nul) == _lib.GGAD_E_INVALID


def test_argument_errors_of_explain():
    cap = int(_lib.load().ggad_explain_max_nbrs())
    ids = np.arange(20)
    for m in (0, -1, cap + 1, 2.5):
        with pytest.raises(ValueError, match="ggad_explain_max_nbrs"):
            E.explain(None, ids, 7, [0, 1], m)
    with pytest.raises(ValueError, match="batch_size"):
        E.explain(None, ids, 0, [0, 1], 5)
    with pytest.raises(ValueError, match="on a GPU"):
        E.explain(None, ids, 7, torch.tensor([0, 1], dtype=torch.int32), 5)          # a CPU tensor of positions
    with pytest.raises(ValueError, match="on a GPU"):
        E.explain(None, torch.arange(20), 7, [0, 1], 5)                              # a CPU tensor of ids
    with pytest.raises(ValueError, match="on a GPU"):
        E.explain(None, ids, 7, SimpleNamespace(pos=torch.tensor([0], dtype=torch.int32)), 5)      # a `Ranked` held on the CPU
    for bad in ([0, 20], [-1], [5, 3, 400]):
        with pytest.raises(ValueError, match="outside the scored list"):
            E.explain(None, ids, 7, bad, 5)
    with pytest.raises(ValueError, match="mini-batch GGAD model"):
        E.explain(object(), ids, 7, [0, 19], 5)                                      # not a GCN with its engine


def _config(**kw):
    from ggad_amd import synth
    rowptr, col = synth.make_graph(300, 2000, 3, kind="powerlaw", max_degree=40)
    data = ((rowptr, col), synth.make_features(300, 17, 3), synth.make_labels(300, 0.1, 3))
    cfg = dict(data_name="synthetic", data_dir="", data=data, seed=72, model="GCN", multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005,
               weight_decay=0.007, batch_size=60, num_epochs=1, valid_epochs=1, num_batches=2, n_pseudo=20, save_dir="unused/",
               test_ratio=0.67, device=0)
    cfg.update(kw)
    return cfg


def test_config_key_errors():
    from ggad_amd.model_handler import ModelHandler
    with pytest.raises(ValueError, match=r"`explain`.*`top_k"):
        ModelHandler(_config(explain=5))                             # explain without top_k: both keys are named
    with pytest.raises(ValueError, match=r"`explain`.*`top_k"):
        ModelHandler(_config(explain_out="e.npz"))
    with pytest.raises(ValueError, match=r"`explain_out` needs `explain"):
        ModelHandler(_config(top_k=20, explain_out="e.npz"))
    with pytest.raises(ValueError, match="ggad_explain_max_nbrs"):
        ModelHandler(_config(top_k=20, explain=int(_lib.load().ggad_explain_max_nbrs()) + 1))
    with pytest.raises(ValueError, match="model: 'GCN'"):
        ModelHandler(_config(model="SAGE", top_k=20, explain=5))
    h = ModelHandler(_config(top_k=20, explain=5, explain_out="e.npz"))
    assert h.explained is None and h.ranked is None
    assert ModelHandler(_config()).explained is None


def test_dgraph_yml_carries_the_keys_off():
    import yaml
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["explain"] == 0 and cfg["explain_out"] == ""


@pytest.mark.parametrize("variant", X.VARIANTS)
def test_the_reference_is_complete_and_no_unit_is_undecided(variant):
    seen_zero = 0
    for d, f in X.shapes():
        for bs in X.BATCH_SIZES:
            ref = X.reference(d, f, bs, variant)
            assert set(ref) == set(X.positions(bs))
            for p, v in ref.items():
                what = (d, f, bs, p)
                assert v["r"] == len(v["nbr"]) == len(v["c"]) and (v["c"] >= 1).all(), what
                assert abs(v["feature"].sum() - v["z"]) <= 1e-12 * v["s_feature"].sum() + 1e-300, what
                assert abs(v["t"].sum() - v["z"]) <= 1e-12 * v["s_t"].sum() + 1e-300, what
                assert not v["undecided"].any(), (what, int(v["undecided"].sum()))
                seen_zero += v["z"] == 0.0
                if variant == "dead":
                    assert v["z"] == 0.0 and not v["mask"].any() and not v["t"].any(), what
    assert (seen_zero > 0) == (variant == "dead")


def test_the_fixture_holds_what_the_gpu_test_needs():
    cap = X.caps()[0]
    ids = X.cases()
    assert len(ids) % 7 and len(ids) % 150
    assert ids[2] == ids[5] and ids[10] == ids[300]
    for bs in X.BATCH_SIZES:
        pos = X.positions(bs)
        ref = X.rows(17, bs)
        sizes = {ref[p]["r"] for p in pos}
        assert {1, 2, 64, 65, cap, cap + 1} <= sizes
        assert 0 in pos and len(ids) - 1 in pos and bs - 1 in pos and bs in pos
        assert len(X.positions_twice(bs)) == len(pos) + 1
        if bs > 1:
            # the repeated id counts twice in its slice; the id of two slices has another count in each
            assert (ref[2]["c"][ref[2]["nbr"] == ids[2]] >= 2).all()
            assert ref[10]["r"] == ref[300]["r"] and not np.array_equal(ref[10]["c"], ref[300]["c"])
            assert ref[20]["c"].max() > 1                            # hub A: some of its columns stand in other rows of the slice
        else:
            assert all((v["c"] == 1).all() for v in ref.values())


def test_write_explained_twice_gives_equal_bytes(tmp_path):
    rng = np.random.default_rng(3)
    k, f, m = 6, 17, 5
    ranked = SimpleNamespace(ids=torch.from_numpy(rng.integers(0, 1000, k)), scores=torch.from_numpy(rng.random(k).astype(np.float32)))

    def make():
        r = np.random.default_rng(4)
        nbr = r.integers(0, 1000, (k, m))
        nbr[0, 3:] = -1
        return E.Explanation(pos=torch.arange(k, dtype=torch.int32), logit=torch.from_numpy(r.standard_normal(k).astype(np.float32)),
                             feature=torch.from_numpy(r.standard_normal((k, f)).astype(np.float32)),
                             closed_size=torch.from_numpy(r.integers(1, 50, k).astype(np.int32)), nbr_id=torch.from_numpy(nbr),
                             nbr_contrib=torch.from_numpy(r.standard_normal((k, m)).astype(np.float32)),
                             nbr_colcount=torch.from_numpy(r.integers(0, 9, (k, m)).astype(np.int32)),
                             rest=torch.from_numpy(r.standard_normal(k).astype(np.float32)), m=m, rows=k, rows_workspace=0,
                             workspace=torch.zeros(1, dtype=torch.int32), stride=1)

    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    E.write_explained(a, ranked, make())
    E.write_explained(b, ranked, make())
    assert open(a, "rb").read() == open(b, "rb").read()
    z = np.load(a)
    assert sorted(z.files) == sorted(["node", "score", "logit", "feature", "closed_size", "nbr_id", "nbr_contrib", "nbr_colcount", "rest"])
    assert z["node"].dtype == np.int64 and z["nbr_id"].dtype == np.int64 and z["feature"].shape == (k, f) and z["nbr_contrib"].shape == (k, m)
    np.testing.assert_array_equal(z["node"], ranked.ids.numpy())
    with pytest.raises(ValueError, match="row for row"):
        E.write_explained(a, SimpleNamespace(ids=ranked.ids[:3], scores=ranked.scores[:3]), make())
