"""What the full-graph entry scripts share (`ggad_amd/fullgraph_script.py`), without a GPU: the loader against digests recorded from
the four loaders of the commit before the scripts shared one (tests/golden/fullgraph_script_loader_83a285a.json), every script's
command line and per-dataset defaults against the values of that commit written out here, and `prepare` on a small graph."""
import hashlib
import json
import os
import random
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT

DATASETS = ("reddit", "Amazon", "photo", "t_finance", "elliptic")


# ------------------------------------------------------------------------------------------------ the loader
def _sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=dtype)).tobytes()).hexdigest()


def _load(fn, dataset):
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    return fn(types.SimpleNamespace(dataset=dataset, synthetic=True, seed=0, quiet=True))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "fullgraph_script_loader_83a285a.json")) as fh:
        return json.load(fh)["datasets"]


@pytest.mark.parametrize("dataset", ["reddit", "photo"])
def test_loader_returns_what_the_four_loaders_returned(dataset, recorded):
    import run
    from ggad_amd.fullgraph_script import Graph, load_graph
    rec = recorded[dataset]
    g = _load(load_graph, dataset)
    assert isinstance(g, Graph)
    assert g._fields == ("adj", "feat", "ano_label", "all_idx", "idx_train", "idx_val", "idx_test", "normal_idx", "abn_idx")
    adj = g.adj.tocsr()
    assert [adj.shape[0], adj.nnz, g.feat.shape[1]] == rec["shape"]
    assert _sha(adj.indptr, np.int64) == rec["adj.indptr"]
    assert _sha(adj.indices, np.int64) == rec["adj.indices"]
    assert _sha(g.feat.todense(), np.float64) == rec["feat"]
    assert _sha(g.ano_label, np.int64) == rec["ano_label"]
    for k in ("all_idx", "idx_train", "idx_val", "idx_test", "normal_idx", "abn_idx"):
        assert _sha(getattr(g, k), np.int64) == rec[k], k
    # run.load: the 6-tuple (adj, feat, ano_label, idx_test, normal_idx, abn_idx), in that order
    t = _load(run.load, dataset)
    assert len(t) == 6
    assert _sha(t[0].tocsr().indices, np.int64) == rec["adj.indices"] and _sha(t[1].todense(), np.float64) == rec["feat"]
    assert [_sha(v, np.int64) for v in t[2:]] == [rec[k] for k in ("ano_label", "idx_test", "normal_idx", "abn_idx")]


# ------------------------------------------------------------------------------------------------ the command lines
COMMON = dict(weight_decay=0.0, seed=0, embedding_dim=300, drop_prob=0.0, readout="avg", auc_test_rounds=256, negsamp_ratio=1,
              synthetic=False, device=0, quiet=False, no_graph=False)
SAMPLING = dict(batch_size=300, subgraph_size=4)
RECON = {"reddit": (1e-3, 500), "Amazon": (1e-3, 800), "photo": (3e-3, 500), "t_finance": (5e-4, 1500), "elliptic": (3e-3, 500)}
# script -> (default dataset, its own options with their defaults, {dataset: (lr, num_epoch), None = no default},
#            (lr, num_epoch) of a dataset it has no entry for, None = an error)
SCRIPTS = {
    "run": ("reddit", dict(mean=0.0, var=0.0, device_noise=False),
            {"reddit": (1e-3, 300), "Amazon": (1e-3, 800), "photo": (1e-3, 100), "t_finance": (1e-3, 500), "elliptic": (1e-3, 150)},
            (1e-3, 100)),
    "ocgnn": ("t_finance", dict(SAMPLING),
              {"reddit": (1e-3, 500), "Amazon": (1e-3, 800), "photo": (1e-3, 600), "t_finance": (5e-4, 1500), "elliptic": (1e-3, 500)},
              (1e-3, 500)),
    "anomalyDAE": ("t_finance", dict(SAMPLING), RECON, None),
    "dominant": ("t_finance", dict(SAMPLING), RECON, None),
    "gaan": ("Amazon", dict(SAMPLING, device_noise=False),
             {"reddit": (1e-3, 500), "Amazon": (1e-3, 800), "photo": (1e-3, 300), "t_finance": (5e-4, 1500), "elliptic": (5e-3, 600)}, None),
    "aegis": ("reddit", dict(SAMPLING, device_noise=False, recon_num_epoch=10, affinity_dir=None),
              {"reddit": (1e-3, 500), "Amazon": (1e-3, 800), "photo": None, "t_finance": (5e-4, 1500), "elliptic": None}, None),
}
RUN_NOISE = {"reddit": (0.02, 0.01), "photo": (0.02, 0.01), "Amazon": (0.0, 0.0), "t_finance": (0.0, 0.0), "elliptic": (0.0, 0.0)}


def _no_default(parse, argv, dataset, capsys):
    with pytest.raises(SystemExit):
        parse(argv)
    assert "no default lr / num_epoch for dataset {!r}: pass --lr and --num_epoch".format(dataset) in capsys.readouterr().err


@pytest.mark.parametrize("script", sorted(SCRIPTS))
def test_defaults_are_the_parents(script, capsys):
    parse = __import__(script).parse
    default_dataset, own, table, elsewhere = SCRIPTS[script]
    assert sorted(table) == sorted(DATASETS)
    for ds, want in table.items():
        if want is None:
            _no_default(parse, ["--dataset", ds], ds, capsys)
            continue
        a = parse(["--dataset", ds])
        assert (a.lr, a.num_epoch) == want, ds
        if script == "run":
            assert (a.mean, a.var) == RUN_NOISE[ds], ds
    if elsewhere is None:
        _no_default(parse, ["--dataset", "x"], "x", capsys)
    else:
        a = parse(["--dataset", "x"])
        assert (a.lr, a.num_epoch) == elsewhere
    # every option the parent's parser had, with the parent's default -- and no other
    a = vars(parse(["--lr", "0.5", "--num_epoch", "3"]))
    want = dict(COMMON, **own, dataset=default_dataset, lr=0.5, num_epoch=3)
    if script == "run":
        want.update(mean=RUN_NOISE[default_dataset][0], var=RUN_NOISE[default_dataset][1])
    assert a == want
    # ... and every one of them is accepted
    given = dict(dataset="elliptic", lr=0.25, weight_decay=0.5, seed=3, embedding_dim=64, num_epoch=7, drop_prob=0.5, readout="max",
                 auc_test_rounds=2, negsamp_ratio=2, device=1, mean=1.0, var=2.0, batch_size=5, subgraph_size=6, recon_num_epoch=2,
                 affinity_dir="d")
    flags = ("synthetic", "quiet", "no_graph", "device_noise")
    argv = []
    for k in want:
        argv += ["--" + k] if k in flags else ["--" + k, str(given[k])]
    a = vars(parse(argv))
    want = {k: True if k in flags else given[k] for k in want}
    if script == "run":
        want.update(mean=0.0, var=0.0)              # (the reference overwrites what the command line gave)
    assert a == want


# ------------------------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("dataset,normalised", [("reddit", True), ("photo", False), ("t_finance", False)])
def test_prepare_normalises_only_the_listed_datasets(dataset, normalised):
    from ggad_amd.fullgraph_script import prepare
    from ggad_amd.utils import normalize_adj, preprocess_features
    rng = np.random.default_rng(0)
    n, f = 12, 5
    a = sp.triu(sp.random(n, n, 0.3, random_state=1), 1)
    adj = ((a + a.T) > 0).astype(np.float64).tocsr()
    feat = sp.lil_matrix(rng.random((n, f)) + 0.5)
    full, feats, ft_size = prepare(types.SimpleNamespace(dataset=dataset), adj, feat, torch.device("cpu"))
    assert ft_size == f and tuple(feats.shape) == (1, n, f) and feats.dtype == torch.float32
    want = preprocess_features(feat) if normalised else np.asarray(feat.todense())
    assert np.array_equal(feats[0].numpy(), np.asarray(want, dtype=np.float32))
    assert normalised == (not np.array_equal(feats[0].numpy(), np.asarray(feat.todense(), dtype=np.float32)))
    assert full.n == n
    assert abs(full.A.host - (normalize_adj(adj) + sp.eye(n)).tocsr()).max() == 0
    assert abs(full.raw_host - (adj + sp.eye(n)).tocsr()).max() == 0


# ------------------------------------------------------------------------------------------------ the ticket block
def test_ticket_block_refuses_to_allocate_inside_a_capture(monkeypatch):
    """`fullgraph.ticket_block` with nothing cached and a capture under way raises before it touches the device (here there is no
    such device: reaching it would raise another error); built eagerly first -- what `FullGraphAdj.__init__` does -- the same call
    inside the capture returns the block that exists."""
    from ggad_amd import fullgraph as FG
    monkeypatch.setattr(FG, "_TICKET_BLOCKS", {})
    monkeypatch.setattr(FG, "_capturing", lambda dev: True)
    with pytest.raises(RuntimeError, match="inside a stream capture"):
        FG.ticket_block("cuda:7")
    assert FG._TICKET_BLOCKS == {}
    monkeypatch.setattr(FG, "_capturing", lambda dev: False)
    a = sp.eye(5, format="csr")
    FG.FullGraphAdj(a, a, "cpu")
    block = FG._TICKET_BLOCKS["cpu"]
    assert block.dtype == torch.int32 and block.numel() % 4 == 0 and not block.any()
    lib = FG._lib.load()
    assert block.numel() >= max(int(lib.ggad_prelu_bwd_one_tickets()), int(lib.ggad_dominant_tickets()), 1)
    monkeypatch.setattr(FG, "_capturing", lambda dev: True)
    assert FG.ticket_block("cpu").data_ptr() == block.data_ptr()
