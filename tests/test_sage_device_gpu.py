"""GraphSAGE from a CSR graph in HBM (`ggad_amd/sage_device.py`, `csrc/sage.hip`, the native sampler of `csrc/sampler.cpp`): parity
with the imported reference, every kernel branch against the float64 restatement (tests/sage_fp64.py), determinism, the errors
raised before any launch, the one-call sweep and the `sage_device` switch of `ModelHandler`."""
import random

import numpy as np
import pytest
import torch

import sage_fp64
from conftest import load_golden
from ggad_amd import synth

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import Encoder, FeatureTable, GraphSage, MeanAggregator
    from ggad_amd.sage_device import SageDevice
    from ggad_amd.sampler import PyCompatRandom

DEV = "cuda:0"
N, K = 512, 10
HUB, D0, D1, D9, D10, D11, D85, D86 = 0, 511, 510, 509, 508, 507, 506, 505


def _branch_graph():
    """Directed.  Ids 0 .. 511 hold the rows under test: degree 0, 1, 9, 10, 11 (below, at and above k = 10), 85 and 86 (both sides
    of `random.sample`'s pool threshold at k = 10) and a hub.  512 ids cannot give one row over 1,000 distinct columns, so the
    ids 512 .. 1535 exist for the hub's columns alone (each points back at one node): the hub row has 1,535 entries."""
    rng = np.random.default_rng(4)
    n = 3 * N
    rows = []
    for v in range(n):
        if v == HUB:
            c = np.concatenate([np.arange(1, N), np.arange(N, n)])
        elif v >= N:
            c = np.array([v - N], dtype=np.int64)
        else:
            deg = {D0: 0, D1: 1, D9: 9, D10: 10, D11: 11, D85: 85, D86: 86}.get(v, int(rng.integers(2, 30)))
            c = np.sort(rng.choice(N, size=deg, replace=False))
        rows.append(c.astype(np.int32))
    rowptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum([len(c) for c in rows], out=rowptr[1:])
    col = np.concatenate(rows)
    deg = np.diff(rowptr)
    assert deg[HUB] > 1000 and [int(deg[v]) for v in (D0, D1, D9, D10, D11, D85, D86)] == [0, 1, 9, 10, 11, 85, 86]
    return rowptr, col


def _table(rowptr, col, nodes, seed):
    """A sample table drawn with numpy: k sorted ids of a row of degree >= k, the whole row otherwise, -1 padding."""
    rng = np.random.default_rng(seed)
    nbr = np.full((len(nodes), K), -1, dtype=np.int32)
    cnt = np.zeros(len(nodes), dtype=np.int32)
    for r, v in enumerate(nodes):
        row = col[rowptr[v]:rowptr[v + 1]]
        pick = np.sort(rng.choice(row, size=K, replace=False)) if len(row) >= K else row
        nbr[r, :len(pick)] = pick
        cnt[r] = len(pick)
    return nbr, cnt


def _batch_nodes(b):
    """The short row first (B = 1 has padding to skip), the hub twice, every special degree but 0, then random ids."""
    rng = np.random.default_rng(b)
    special = [D9, HUB, D1, D10, D11, D85, D86, HUB]
    rest = [int(v) for v in rng.choice(np.arange(1, 500), size=max(0, b - len(special)), replace=False)]
    return np.array((special + rest)[:b], dtype=np.int64)


@pytest.fixture(scope="module")
def branch():
    rowptr, col = _branch_graph()
    return {"rowptr": rowptr, "col": col, "graph": DeviceGraph(rowptr, col, DEV)}


def _weights(f, d, seed):
    rng = np.random.default_rng(seed)

    def xavier(r, c):
        a = np.sqrt(6.0 / (r + c))
        return rng.uniform(-a, a, (r, c)).astype(np.float32)
    return xavier(d, 2 * f), xavier(2, d)


def _device_step(dev, nodes, nbr, cnt, labels, w_enc, w_cls):
    we, wc = torch.from_numpy(w_enc).to(DEV), torch.from_numpy(w_cls).to(DEV)
    out = dev.forward(dev.upload(nodes, nbr, cnt, labels), we, wc)
    got = {k: out[k] for k in ("combined", "emb", "scores")}
    if labels is not None:
        got["loss"], got["dscores"] = out["loss"][:1], out["dscores"]
        got["grad.enc"], got["grad.cls"] = dev.backward(out["combined"], out["emb"], out["dscores"], wc)
    return {k: v.detach().cpu().numpy().copy() for k, v in got.items()}


CASES = [(b, 17, 64) for b in (1, 63, 64, 65, 200)] + [(b, f, d) for b in (1, 200) for f in (1, 64) for d in (1, 64)] + \
    [(65, 17, 33), (200, 64, 33), (1, 1, 33), (64, 17, 1)]


def test_reference_fixture_on_the_device_path(capsys):
    """The loop of `test_graphsage_training_loop_vs_reference_golden` (tests/test_dropin_gpu.py) with `Encoder` on a `DeviceGraph`
    and `SageDevice(rng=None)`: same batches, the position of python's `random` stream afterwards equal to the fixture's (every
    shuffle and every sample drawn the same way), losses within 2e-6, final weights and `to_prob` within 3e-6 -- the bounds of that
    test.  The set path runs beside it and both paths' errors against the fixture are printed; a quantity's bound is
    max(the bound above, 4 x the set path's own error): another summation order gets that margin and nothing wider.
    Figures of an MI355X run, device / set: losses 1.8e-7 / 1.8e-7, final encoder weight 5.2e-8 / 3.7e-8, final
    classifier weight 1.5e-8 / 1.5e-8, `to_prob` 6.0e-8 / 6.0e-8: no bound took the set-path margin."""
    g = load_golden("minibatch_sage.npz")
    f, d = int(g["f"]), int(g["d"])
    labels = g["labels"]
    errs = {}
    for path in ("set", "device"):
        feats = FeatureTable(torch.from_numpy(g["feat"]))
        graph = DeviceGraph(g["rowptr"], g["col"], DEV)
        idx_train = list(range(100, 700))
        idx_anomaly = [int(i) for i in np.nonzero(labels)[0][:60]]
        random.seed(72)
        agg = MeanAggregator(feats, cuda=True)
        if path == "device":
            enc = Encoder(feats, f, d, graph, agg, gcn=False, cuda=True, sage_device=SageDevice(graph, feats, f, d, 10, rng=None))
            assert enc.device_path is not None
        else:
            enc = Encoder(feats, f, d, synth.csr_to_adj_lists(g["rowptr"], g["col"]), agg, gcn=False, cuda=True)
        enc.num_samples = 5
        model = GraphSage(2, enc).to(DEV)
        with torch.no_grad():
            enc.weight.copy_(torch.from_numpy(g["init.enc.weight"]))
            model.weight.copy_(torch.from_numpy(g["init.weight"]))
        opt = FlatAdam([p for p in model.parameters() if p.requires_grad], lr=0.001, weight_decay=0.007)
        bs, nb, n_pseudo = 40, 4, 10
        losses, step = [], 0
        for epoch in range(2):
            random.shuffle(idx_train)
            for b in range(nb):
                batch_nodes = idx_train[b * bs:(b + 1) * bs]
                random.shuffle(idx_anomaly)
                batch_nodes = batch_nodes + idx_anomaly[:n_pseudo]
                assert np.array_equal(np.array(batch_nodes), g["batches"][step])
                opt.zero_grad()
                loss = model.loss(batch_nodes, torch.as_tensor(labels[np.array(batch_nodes)], device=DEV).long())
                loss.backward()
                opt.step()
                losses.append(loss.item())
                step += 1
        test_nodes = g["test_nodes"].tolist()
        with torch.no_grad():
            probs = torch.cat([model.to_prob(test_nodes[s:s + 30]) for s in range(0, 90, 30)]).cpu().numpy()
        assert np.array_equal(np.array(random.getstate()[1], dtype=np.uint64), g["py_random_after"]), path
        errs[path] = {"losses": float(np.abs(np.array(losses) - g["losses"]).max()),
                      "final.enc.weight": float(np.abs(enc.weight.detach().cpu().numpy() - g["final.enc.weight"]).max()),
                      "final.weight": float(np.abs(model.weight.detach().cpu().numpy() - g["final.weight"]).max()),
                      "to_prob": float(np.abs(probs - g["test_probs"]).max())}
    project = {"losses": 2e-6, "final.enc.weight": 3e-6, "final.weight": 3e-6, "to_prob": 3e-6}
    failures = []
    with capsys.disabled():
        for key, bound in project.items():
            final = max(bound, 4.0 * errs["set"][key])
            print(f"\n[sage fixture] {key}: device {errs['device'][key]:.3e} set {errs['set'][key]:.3e} bound {final:.3e}", end="")
            if errs["device"][key] > final:
                failures.append((key, errs["device"][key], final))
        print()
    assert not failures, failures


@pytest.mark.parametrize("b,f,d", CASES)
def test_every_kernel_branch_against_the_float64_restatement(branch, b, f, d, capsys):
    """combined, emb, scores, the loss, dscores and both gradients on the branch graph, labels mixed and all one class: the device's
    error against the float64 restatement is at most 4 x the error of the SAME restatement in float32 on the CPU, or 1e-6 x the
    quantity's largest magnitude where that is more (the rule of tests/test_pcgnn_device_gpu.py).  Then the same batch with the row of
    degree 0 appended, unlabelled: the other rows keep their bits, the empty row is NaN exactly where the restatement's is.
    Every ratio is printed.  On an MI355X the largest ratio over the cases is 1.33 (combined), 1.29 (emb), 1.39 (grad.enc) and 3.57
    (grad.cls); scores 4.5, loss 11.0 and dscores 7.9 occur at B = 1, F = 1 (and the loss at B = 63, one class), where the float32
    restatement lands within a few 1e-9 of float64: the device error there is at most 0.12 of the 1e-6 x magnitude limb."""
    nodes = _batch_nodes(b)
    nbr, cnt = _table(branch["rowptr"], branch["col"], nodes, 100 + b)
    assert cnt[0] == 9 and (nbr[0, 9:] == -1).all()
    feat = synth.make_features(3 * N, f, 21)
    w_enc, w_cls = _weights(f, d, 100 * f + d)
    dev = SageDevice(branch["graph"], FeatureTable(torch.from_numpy(feat)), f, d, K)
    failures = []
    with capsys.disabled():
        for tag, labels in (("mixed", (np.arange(b) % 3 == 0).astype(np.int64)), ("one class", np.ones(b, dtype=np.int64))):
            want = sage_fp64.evaluate(feat, nodes, nbr, cnt, w_enc, w_cls, labels, torch.float64)
            yard = sage_fp64.evaluate(feat, nodes, nbr, cnt, w_enc, w_cls, labels, torch.float32)
            got = _device_step(dev, nodes, nbr, cnt, labels, w_enc, w_cls)
            for key in sage_fp64.KEYS:
                assert got[key].shape == want[key].shape and np.isfinite(got[key]).all(), key
                err = float(np.abs(got[key] - want[key]).max())
                err32 = float(np.abs(yard[key] - want[key]).max())
                bound = max(4.0 * err32, 1e-6 * float(np.abs(want[key]).max()))
                print(f"\n[sage branches B={b} F={f} D={d} {tag}] {key}: device {err:.3e} float32 {err32:.3e} "
                      f"ratio {err / max(err32, 1e-30):.2f} bound {bound:.3e}", end="")
                if err > bound:
                    failures.append((tag, key, err, err32, bound))
        print()
    assert not failures, failures
    nodes0 = np.concatenate([nodes, [D0]])
    nbr0, cnt0 = np.concatenate([nbr, np.full((1, K), -1, dtype=np.int32)]), np.concatenate([cnt, [0]]).astype(np.int32)
    got0 = _device_step(dev, nodes0, nbr0, cnt0, None, w_enc, w_cls)
    want0 = sage_fp64.evaluate(feat, nodes0, nbr0, cnt0, w_enc, w_cls, None, torch.float64)
    for key in ("combined", "emb", "scores"):
        assert np.array_equal(got0[key][:b], got[key]), key
        assert np.array_equal(np.isnan(got0[key][b]), np.isnan(want0[key][b])), key
    assert np.array_equal(got0["combined"][b, :f], feat[D0]) and np.isnan(got0["combined"][b, f:]).all()


def test_same_batch_gives_the_same_bits_and_padding_is_not_read(branch):
    """The same batch launched twice and from a fresh object: equal bits; the -1 padding of the short rows replaced by another
    invalid id: equal bits again."""
    f, d, b = 17, 64, 200
    nodes = _batch_nodes(b)
    nbr, cnt = _table(branch["rowptr"], branch["col"], nodes, 7)
    labels = (np.arange(b) % 3 == 0).astype(np.int64)
    feat = synth.make_features(3 * N, f, 21)
    w_enc, w_cls = _weights(f, d, 3)
    dev = SageDevice(branch["graph"], FeatureTable(torch.from_numpy(feat)), f, d, K)
    first = _device_step(dev, nodes, nbr, cnt, labels, w_enc, w_cls)
    other = _batch_nodes(65)
    _device_step(dev, other, *_table(branch["rowptr"], branch["col"], other, 8), np.zeros(65, dtype=np.int64), w_enc, w_cls)
    second = _device_step(dev, nodes, nbr, cnt, labels, w_enc, w_cls)
    fresh = _device_step(SageDevice(branch["graph"], FeatureTable(torch.from_numpy(feat)), f, d, K), nodes, nbr, cnt, labels, w_enc,
                         w_cls)
    assert (nbr == -1).sum() > 0
    poisoned = np.where(nbr == -1, np.int32(2 ** 30), nbr)
    padded = _device_step(dev, nodes, poisoned, cnt, labels, w_enc, w_cls)
    for key in sage_fp64.KEYS:
        for name, other_run in (("second", second), ("fresh", fresh), ("padding", padded)):
            assert np.array_equal(first[key], other_run[key]), (key, name)


def test_errors_raise_before_any_launch(branch):
    graph = branch["graph"]
    wide = FeatureTable(torch.from_numpy(synth.make_features(3 * N, 65, 1)))
    feats = FeatureTable(torch.from_numpy(synth.make_features(3 * N, 17, 1)))
    with pytest.raises(ValueError, match="feat_dim <= 64"):
        SageDevice(graph, wide, 65, 64, K)
    with pytest.raises(ValueError, match="embed_dim <= 64"):
        SageDevice(graph, feats, 17, 65, K)
    with pytest.raises(ValueError, match="2 classes"):
        SageDevice(graph, feats, 17, 64, K, num_classes=3)
    with pytest.raises(ValueError, match="gcn"):
        SageDevice(graph, feats, 17, 64, K, gcn=True)
    with pytest.raises(ValueError, match="num_sample"):
        SageDevice(graph, feats, 17, 64, None)
    agg = MeanAggregator(feats, cuda=True)
    with pytest.raises(ValueError):
        Encoder(feats, 17, 64, graph, agg, gcn=True, cuda=True, sage_device=True)
    with pytest.raises(ValueError):
        Encoder(feats, 17, 64, graph, agg, num_sample=None, cuda=True, sage_device=True)
    enc = Encoder(feats, 17, 64, graph, agg, cuda=True, sage_device=True)
    with pytest.raises(ValueError, match="2 classes"):
        GraphSage(3, enc)
    model = GraphSage(2, enc)
    state = random.getstate()
    for bad in ([3 * N], [-1], [5, 3 * N + 7]):
        with pytest.raises(ValueError):
            model.to_prob(bad)
        with pytest.raises(ValueError):
            model.loss(bad, np.zeros(len(bad), dtype=np.int64))
    assert random.getstate() == state                                     # nothing was drawn for a refused batch
    dev = enc.device_path
    nodes = _batch_nodes(8)
    nbr, cnt = _table(branch["rowptr"], branch["col"], nodes, 1)
    bad_nbr = nbr.copy()
    bad_nbr[1, 0] = 3 * N
    with pytest.raises(ValueError):
        dev.upload(nodes, bad_nbr, cnt)
    with pytest.raises(ValueError):
        dev.upload(nodes, nbr, cnt + K)
    with pytest.raises(ValueError):
        dev.upload(nodes, nbr, cnt, labels=np.full(8, 2))
    w_enc, w_cls = (torch.from_numpy(w).to(DEV) for w in _weights(17, 64, 1))
    batch = dev.upload(nodes, nbr, cnt)
    with pytest.raises(ValueError):
        dev.forward(batch, w_enc.double(), w_cls)                         # wrong dtype
    with pytest.raises(ValueError):
        dev.forward(batch, w_enc.t().contiguous().t(), w_cls)             # not contiguous
    with pytest.raises(ValueError):
        dev.forward(batch, w_enc, w_cls.cpu())                            # not on the GPU
    batch.nodes = batch.nodes.long()
    with pytest.raises(ValueError):
        dev.forward(batch, w_enc, w_cls)                                  # int64 ids
    batch = dev.upload(nodes, nbr, cnt)
    batch.cnt = torch.zeros(16, dtype=torch.int32, device=DEV)[::2]
    with pytest.raises(ValueError):
        dev.forward(batch, w_enc, w_cls)                                  # a strided view


def test_one_call_sweep_equals_chunked_to_prob(branch):
    """`to_prob` over 333 nodes in one call == chunks of 60 bit for bit, and python's `random` stream ends at the same position."""
    f, d = 17, 64
    feats = FeatureTable(torch.from_numpy(synth.make_features(3 * N, f, 5)))
    graph = branch["graph"]
    torch.manual_seed(5)
    enc = Encoder(feats, f, d, graph, MeanAggregator(feats, cuda=True), cuda=True, sage_device=True)
    model = GraphSage(2, enc).to(DEV)
    sweep = [int(v) for v in np.random.default_rng(2).integers(0, 505, 333)] + [HUB, D85, D86, HUB]
    with torch.no_grad():
        random.seed(11)
        whole = model.to_prob(sweep).cpu().numpy()
        after_whole = random.getstate()
        random.seed(11)
        parts = torch.cat([model.to_prob(sweep[s:s + 60]) for s in range(0, len(sweep), 60)]).cpu().numpy()
    assert random.getstate() == after_whole
    assert whole.shape == (len(sweep), 2) and np.isfinite(whole).all() and np.array_equal(whole, parts)


def _handler_run(tmp_path, tag, device_path, perturb=0.0):
    import ggad_amd.model_handler as mh
    n = 3000
    rowptr, col = synth.make_graph(n, 30000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab.copy()), seed=72, model="SAGE",
               multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=3,
               valid_epochs=2, num_batches=6, n_pseudo=20, save_dir=str(tmp_path) + f"/{tag}/", test_ratio=0.67, device=0)
    if device_path:
        cfg["sage_device"] = True
    random.seed(72)
    np.random.seed(72)
    torch.manual_seed(72)
    original = mh.GraphSage

    class Perturbed(original):               # the sensitivity probe: the same run from initial weights moved by 1e-7 relative
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            gen = torch.Generator().manual_seed(1)
            with torch.no_grad():
                for p in self.parameters():
                    if p.requires_grad:
                        p.mul_((1 + perturb * torch.randn(p.shape, generator=gen)).to(p.device))
    if perturb:
        mh.GraphSage = Perturbed
    try:
        h = mh.ModelHandler(cfg)
        res = h.train()
    finally:
        mh.GraphSage = original
    sd = {k: v.detach().cpu().numpy().copy() for k, v in h.model.state_dict().items()}
    return h, res, np.array(h.sage_losses), sd, random.getstate()


def test_model_handler_trains_from_csr_on_the_device_path(tmp_path, capsys):
    """`sage_device=True` with `data=((rowptr, col), feat, lab)` on the configuration of `test_model_handler_sage_runs_end_to_end`: the
    5-tuple, 18 losses, the loss falling, "Restore model"; two runs bit-identical; python's `random` stream after `train()` where
    the set path leaves it; the first loss within 1e-5 and the final AUC within 1e-4 of the set path's; the other 17 losses within
    4 x max(e_t, 1e-6 |loss_t|), e_t the set path's own deviation after its initial weights moved by 1e-7 relative.  The three
    series are printed."""
    dev_runs = [_handler_run(tmp_path, f"dev{rep}", True) for rep in range(2)]
    for h, res, ls, sd, _ in dev_runs:
        assert h.model.enc.device_path is not None
        assert len(res) == 5 and all(np.isfinite(r) for r in res[:4]) and 0.0 <= res[3] <= 1.0
        assert ls.shape == (18,) and np.isfinite(ls).all() and ls[-6:].mean() < ls[:6].mean()
    assert "Restore model from epoch" in capsys.readouterr().out
    assert np.array_equal(dev_runs[0][2], dev_runs[1][2]) and dev_runs[0][1] == dev_runs[1][1]
    for k in dev_runs[0][3]:
        assert np.array_equal(dev_runs[0][3][k], dev_runs[1][3][k]), k
    h_set, res_set, ls_set, _, state_set = _handler_run(tmp_path, "set", False)
    assert getattr(h_set.model.enc, "device_path", None) is None
    assert dev_runs[0][4] == state_set
    _, _, ls_probe, _, _ = _handler_run(tmp_path, "probe", False, perturb=1e-7)
    ls_dev, res_dev = dev_runs[0][2], dev_runs[0][1]
    diff = np.abs(ls_dev - ls_set)
    e_t = np.abs(ls_probe - ls_set)
    bound = 4.0 * np.maximum(e_t, 1e-6 * np.abs(ls_set))
    with capsys.disabled():
        print("\n[sage handler] |device - set| per step:\n", diff)
        print("[sage handler] set path's own deviation e_t after a 1e-7 relative move of its initial weights:\n", e_t)
        print("[sage handler] bound 4 max(e_t, 1e-6 |loss_t|):\n", bound)
        print(f"[sage handler] maxima: |device - set| {diff.max():.3e}, e_t {e_t.max():.3e}, AUC device {res_dev[3]:.6f} "
              f"set {res_set[3]:.6f}")
    np.testing.assert_allclose(ls_dev[0], ls_set[0], atol=1e-5, rtol=0)
    assert abs(res_dev[3] - res_set[3]) <= 1e-4
    assert (diff[1:] <= bound[1:]).all(), (diff[1:] - bound[1:]).max()
    capsys.readouterr()
