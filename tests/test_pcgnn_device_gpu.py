"""PC-GNN from CSR relation graphs in HBM (`ggad_amd/pcgnn_device.py`, `csrc/pcgnn.hip`): parity with the imported reference, the
integer plan against numpy, every kernel branch against the float64 restatement (tests/pcgnn_fp64.py), determinism with clean
scratch, and the `pcgnn_device` switch of `ModelHandler`."""
import random

import numpy as np
import pytest
import torch

import pcgnn_fp64
from conftest import load_golden
from ggad_amd import synth

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import FeatureTable
    from ggad_amd.layers import InterAgg, IntraAgg, PCALayer
    from ggad_amd.pcgnn_device import RelationState

DEV = "cuda:0"
N = 1200
HUB, TWICE, LOOP_ONLY = 0, 200, 777
ROW1, ROW63, ROW64, ROW65 = 1199, 1101, 1102, 1103


def _csr(dense):
    rows, cols = np.nonzero(dense)
    rowptr = np.zeros(len(dense) + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=len(dense)), out=rowptr[1:])
    return rowptr, cols.astype(np.int32)


def _branch_relations():
    """Relation A, symmetric: a hub of degree 1,106 (split over the four waves in both hops), rows of degree exactly 1, 63, 64 and 65
    (below, at and above one wave of entries), self loops.  Relation B, directed: 1 to 12 random columns per row and one row of 300.
    Relation C, symmetric and sparse: rows without an edge hold only their own diagonal entry, LOOP_ONLY among them."""
    rng = np.random.default_rng(5)
    a = np.zeros((N, N), dtype=bool)
    a[HUB, 1:1101] = True
    a[ROW63, 200:263] = a[ROW64, 200:264] = a[ROW65, 200:265] = True
    ring = np.arange(1104, 1198)
    a[ring, ring + 1] = True                                     # 1104 - ... - 1198
    a[ROW1, 1198] = True
    i, j = rng.integers(1, 1101, 1500), rng.integers(1, 1101, 1500)
    a[i[i != j], j[i != j]] = True
    a |= a.T
    for v in (HUB, 5, 6, 300, 1150):
        a[v, v] = True
    b = np.zeros((N, N), dtype=bool)
    for r in range(N):
        b[r, rng.choice(N, size=300 if r == 40 else int(rng.integers(1, 13)), replace=False)] = True
    c = np.zeros((N, N), dtype=bool)
    i, j = rng.integers(0, N, 700), rng.integers(0, N, 700)
    c[i[i != j], j[i != j]] = True
    c[LOOP_ONLY, :] = False
    c[:, LOOP_ONLY] = False
    c |= c.T
    lonely = np.flatnonzero(c.sum(1) == 0)
    c[lonely, lonely] = True
    rels = [_csr(m) for m in (a, b, c)]
    deg = np.diff(rels[0][0])
    assert deg[HUB] > 1024 and (deg[ROW1], deg[ROW63], deg[ROW64], deg[ROW65]) == (1, 63, 64, 65)
    assert not np.array_equal(b, b.T) and b.sum(1).min() >= 1 and LOOP_ONLY in lonely and len(lonely) > 3
    return rels


def _batches():
    """B = 1, and B = 48 with the hub, TWICE listed twice, neighbours of other batch nodes (1198 and 1199; 5 is the hub's), the rows of
    degree 1 / 63 / 64 / 65, the long row of relation B and a diagonal-only row of relation C."""
    rng = np.random.default_rng(9)
    fixed = [HUB, TWICE, TWICE, 1198, ROW1, ROW63, ROW64, ROW65, 5, 40, LOOP_ONLY, 1150]
    rest = [int(v) for v in rng.choice(np.arange(1, N), size=48 - len(fixed), replace=False)]
    return {1: np.array([TWICE]), 48: np.array(fixed + rest)}


@pytest.fixture(scope="module")
def branch():
    rels = _branch_relations()
    return {"rels": rels, "graphs": [DeviceGraph(rp, ci, DEV) for rp, ci in rels], "batches": _batches()}


def _weights(f, d, seed):
    rng = np.random.default_rng(seed)

    def xavier(r, c):
        a = np.sqrt(6.0 / (r + c))
        return rng.uniform(-a, a, (r, c)).astype(np.float32)
    w = {"inter1.weight": xavier(3 * d, d), "weight": xavier(2, d)}
    w.update({f"inter1.intra_agg{k}.weight": xavier(f, d) for k in (1, 2, 3)})
    return w


def _model(graphs, feat, f, d, weights):
    feats = FeatureTable(torch.from_numpy(feat))
    intras = [IntraAgg(feats, f, d, [], 0.5, cuda=True) for _ in range(3)]
    inter = InterAgg(feats, f, d, [], graphs, intras, inter="GNN", cuda=True)
    model = PCALayer(2, inter, 2)
    sd = model.state_dict()
    with torch.no_grad():
        for k in pcgnn_fp64.PARAMS:
            sd[k].copy_(torch.from_numpy(weights[k]))
    return inter, model


def _scratch_is_clean(st):
    """pos all -1, counts all 0, no bit left in the bitmap words that cover the N nodes."""
    words = (st.graph.n + 31) // 32
    return int((st.pos != -1).sum()) == 0 and int(st.cnt.abs().sum()) == 0 and int(st.scan[:words].abs().sum()) == 0


def _probe(scores, affinity):
    """Finite scalar of a batch that has one label only (B = 1): the squared scores plus the affinity.  Every term is >= 0 (the
    affinity is the cosine of two vectors that went through a ReLU), so nothing cancels and the floor of 1e-6 x |value| is 1e-6 of
    what was added up.  A signed linear probe can cancel to a fraction of its terms, and then one or two float32 roundings of a
    term, which no float32 path avoids, already exceed 1e-6 of the difference."""
    return (scores * scores).sum() + affinity.sum()


def _device_outputs(model, nodes, labels, objective=None):
    model.zero_grad()
    lab = torch.from_numpy(labels).to(DEV)
    with torch.no_grad():
        emb, aff = model.inter1.forward(nodes.tolist(), lab, True)
    if objective is None:
        loss, con = model.loss(nodes.tolist(), lab, True)
    else:
        loss, con = objective(*model.forward(nodes.tolist(), lab, True)), torch.zeros((), device=DEV)
    loss.backward()
    out = {"combined": emb.t(), "affinity": aff, "loss": torch.stack([loss.detach().reshape(()), con.detach().reshape(())])}
    out.update({"grad." + k: p.grad for k, p in model.named_parameters() if k in pcgnn_fp64.PARAMS})
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def test_reference_parity_on_device_graph_relations():
    """`InterAgg` + `PCALayer` on `DeviceGraph` relations against the imported reference classes (tests/golden/minibatch_pcgnn.npz),
    the assertions and bounds of the set path's test (test_dropin_gpu.py)."""
    g = load_golden("minibatch_pcgnn.npz")
    f, d = int(g["f"]), int(g["d"])
    graphs = [DeviceGraph(g[f"rowptr{k}"], g[f"col{k}"], DEV) for k in range(3)]
    inter, model = _model(graphs, g["feat"], f, d, {k: g["init." + k] for k in pcgnn_fp64.PARAMS})
    assert inter.device_path is not None
    nodes, labels = g["nodes"].tolist(), torch.from_numpy(g["labels"]).to(DEV)
    emb, aff = inter.forward(nodes, labels, True)
    np.testing.assert_allclose(emb.detach().cpu().numpy(), g["combined"], atol=3e-6, rtol=0)
    np.testing.assert_allclose(aff.detach().cpu().numpy(), g["affinity"], atol=3e-6, rtol=0)
    loss, lcon = model.loss(nodes, labels, True)
    np.testing.assert_allclose([loss.item(), lcon.item()], g["loss"], atol=1e-5, rtol=0)
    loss.backward()
    params = dict(model.named_parameters())
    for k in pcgnn_fp64.PARAMS:
        np.testing.assert_allclose(params[k].grad.cpu().numpy(), g["grad." + k], atol=4e-6, rtol=2e-4, err_msg=k)
    assert inter.features.weight.grad is None and inter.label_clf.weight.grad is None
    with torch.no_grad():
        pg, pl = model.to_prob(nodes, labels, False)
    np.testing.assert_allclose(pg.cpu().numpy(), g["prob_gnn"], atol=3e-6, rtol=0)
    np.testing.assert_allclose(pl.cpu().numpy(), g["prob_label"], atol=3e-6, rtol=0)


@pytest.mark.parametrize("b", [1, 48])
def test_plan_integers_equal_numpy(branch, b):
    """unique, pos, row_count and col_count of every branch relation, bit for bit; the scratch is clean again after release."""
    nodes = branch["batches"][b]
    for (rowptr, col), graph in zip(branch["rels"], branch["graphs"]):
        st = RelationState(graph)
        cap = st.capacity(nodes)
        assert cap == min(N, int(np.diff(rowptr)[nodes].sum()))
        plan = st.plan(st.upload(nodes), cap)
        unique, pos, row_count, col_count = pcgnn_fp64.plan_numpy(rowptr, col, nodes)
        nu = int(plan.n_unique.item())
        assert nu == len(unique) <= cap
        assert np.array_equal(plan.unique.cpu().numpy()[:nu], unique) and (plan.unique.cpu().numpy()[nu:] == -1).all()
        assert np.array_equal(plan.row_count.cpu().numpy()[:nu], row_count) and (plan.row_count.cpu().numpy()[nu:] == 0).all()
        assert np.array_equal(plan.pos.cpu().numpy(), pos)
        assert np.array_equal(plan.col_count.cpu().numpy(), col_count)
        plan.release()
        assert _scratch_is_clean(st)


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("f", [10, 17, 64])
@pytest.mark.parametrize("b", [1, 48])
def test_every_kernel_branch_against_the_float64_restatement(branch, b, f, d):
    """combined, affinity, loss and the five gradients on the branch graphs: the device's error against the float64 restatement is at
    most 4 x the error of the SAME restatement evaluated in float32 on the CPU, or 1e-6 x the quantity's largest magnitude where
    that is more (the split-row combine and the GEMM order differ from torch's; the hub row adds over a thousand terms).  B = 1 has
    one label, so the PC-GNN loss is 0 / 0 there: a fixed probe of scores and affinity whose terms cannot cancel (`_probe`) is
    differentiated instead.
    Every figure is printed before the assertion.  Ratios device error / float32-restatement error: not yet recorded on an MI355X
    (DESIGN 4d); the kernels' arithmetic run lane by lane on the host gives 0.1 to 1.5 at (B, F, D) = (48, 17, 64) and (1, 10, 32)."""
    nodes = branch["batches"][b]
    labels = (np.arange(b) % 3 == 0).astype(np.int64)
    feat = synth.make_features(N, f, 21)
    weights = _weights(f, d, 100 * f + d)
    objective = _probe if b == 1 else None
    want = pcgnn_fp64.evaluate(branch["rels"], feat, nodes, labels, weights, torch.float64, objective)
    yard = pcgnn_fp64.evaluate(branch["rels"], feat, nodes, labels, weights, torch.float32, objective)
    _, model = _model(branch["graphs"], feat, f, d, weights)
    got = _device_outputs(model, nodes, labels, objective)
    failures = []
    for key in ["combined", "affinity", "loss"] + ["grad." + k for k in pcgnn_fp64.PARAMS]:
        assert got[key].shape == want[key].shape and np.isfinite(got[key]).all(), key
        err = float(np.abs(got[key] - want[key]).max())
        err32 = float(np.abs(yard[key] - want[key]).max())
        bound = max(4.0 * err32, 1e-6 * float(np.abs(want[key]).max()))
        print(f"[pcgnn branches B={b} F={f} D={d}] {key}: device {err:.3e} float32 {err32:.3e} ratio {err / max(err32, 1e-30):.2f} "
              f"bound {bound:.3e}")
        if err > bound:
            failures.append((key, err, err32, bound))
    assert not failures, failures


def test_same_batch_gives_the_same_bits_and_padding_rows_are_zero(branch):
    """Batch X, then Y, then X again: the first and third results are bit-identical, and identical to a freshly constructed model's
    (nothing of a batch is left in the scratch); the rows past |U| of A2, T2 and dZ2 are zeros."""
    f, d = 17, 64
    feat = synth.make_features(N, f, 21)
    weights = _weights(f, d, 3)
    x, y = branch["batches"][48], np.array([HUB, 40, 3, 900, 901, 1198])
    lx, ly = (np.arange(48) % 3 == 0).astype(np.int64), np.array([0, 1, 0, 1, 0, 0])
    _, model = _model(branch["graphs"], feat, f, d, weights)
    first = _device_outputs(model, x, lx)
    for st in model.inter1.device_path.states:
        last = st.last
        rows, nu = last["batch_rows"], int(last["plan"].n_unique.item())
        assert nu < last["plan"].cap                                   # (there are padding rows to look at)
        for name in ("a", "t", "dz"):
            assert last[name].shape[0] == rows + last["plan"].cap
            assert float(last[name][rows + nu:].abs().max()) == 0.0, name
            assert float(last[name][rows:rows + nu].abs().max()) > 0.0, name
        assert _scratch_is_clean(st)
    _device_outputs(model, y, ly)
    third = _device_outputs(model, x, lx)
    _, fresh_model = _model(branch["graphs"], feat, f, d, weights)
    fresh = _device_outputs(fresh_model, x, lx)
    for key in first:
        assert np.array_equal(first[key], third[key]), key
        assert np.array_equal(first[key], fresh[key]), key


def test_shapes_outside_the_hop_kernel_and_bad_tensors_raise(branch):
    feat = synth.make_features(N, 65, 1)
    with pytest.raises(ValueError, match="feat_dim <= 64"):
        _model(branch["graphs"], feat, 65, 64, _weights(65, 64, 1))
    with pytest.raises(ValueError, match="embed_dim <= 64"):
        _model(branch["graphs"], feat[:, :17].copy(), 17, 128, _weights(17, 128, 1))
    st = RelationState(branch["graphs"][0])
    with pytest.raises(ValueError):
        st.plan(torch.arange(4, device=DEV), 4)                           # int64 ids
    with pytest.raises(ValueError):
        st.plan(torch.arange(8, dtype=torch.int32, device=DEV)[::2], 4)   # not contiguous
    with pytest.raises(ValueError):
        st.upload(np.array([N]))
    assert _scratch_is_clean(st)


def _handler_run(tmp_path, tag, rels, device_path, perturb=0.0):
    import ggad_amd.layers as layers
    from ggad_amd.model_handler import ModelHandler
    n = 3000
    rp0, ci0 = synth.make_graph(n, 30000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    cfg = dict(data_name="synthetic", data_dir="", data=(synth.csr_to_adj_lists(rp0, ci0), feat, lab.copy()), relations=rels, seed=72,
               model="PCGNN", multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60,
               num_epochs=3, valid_epochs=2, num_batches=5, n_pseudo=20, save_dir=str(tmp_path) + f"/{tag}/", test_ratio=0.67,
               device=0, rho=0.5, alpha=2)
    if device_path:
        cfg["pcgnn_device"] = True
    random.seed(72)
    np.random.seed(72)
    torch.manual_seed(72)
    original = layers.PCALayer

    class Perturbed(original):               # the sensitivity probe: the same run from initial weights moved by 1e-7 relative
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            gen = torch.Generator().manual_seed(1)
            with torch.no_grad():
                for p in self.parameters():
                    if p.requires_grad:
                        p.mul_((1 + perturb * torch.randn(p.shape, generator=gen)).to(p.device))
    if perturb:
        layers.PCALayer = Perturbed
    try:
        h = ModelHandler(cfg)
        res = h.train()
    finally:
        layers.PCALayer = original
    return h, res, np.array(h.pcgnn_losses), {k: v.detach().cpu().numpy().copy() for k, v in h.model.state_dict().items()}, cfg


def test_model_handler_trains_from_csr_relations_on_the_device_path(tmp_path, capsys):
    """`pcgnn_device=True` with (rowptr, col) relations on the configuration of the set path's handler test: the same self-consistency
    checks, two runs bit-identical, the first loss pair within 1e-5 and the final AUC within 1e-4 of the set path's; the other 14
    loss pairs within 4 x max(e_t, 1e-6 |loss_t|) of it, e_t the set path's own deviation after its initial weights moved by 1e-7
    relative.  The three series and their maxima are printed."""
    from ggad_amd.model_handler import ModelHandler
    n = 3000
    rels = [synth.make_graph(n, 20000 + 5000 * k, 11 + k, kind="powerlaw", max_degree=150) for k in range(3)]
    sets = [synth.csr_to_adj_lists(rp, ci) for rp, ci in rels]
    dev_runs = [_handler_run(tmp_path, f"dev{rep}", rels, True) for rep in range(2)]
    for h, res, ls, sd, _ in dev_runs:
        assert h.model.inter1.device_path is not None
        assert len(res) == 5 and all(np.isfinite(r) for r in res[:4]) and 0.0 <= res[3] <= 1.0
        assert ls.shape == (15, 2) and np.isfinite(ls).all() and (ls[:, 0] >= 5 * ls[:, 1] - 1e-5).all()
        for k in pcgnn_fp64.PARAMS:
            assert k in sd
    out = capsys.readouterr().out
    assert "Restore model from epoch" in out and "loss_constraint" in out
    assert np.array_equal(dev_runs[0][2], dev_runs[1][2])
    for k in dev_runs[0][3]:
        assert np.array_equal(dev_runs[0][3][k], dev_runs[1][3][k]), k
    _, res_set, ls_set, _, _ = _handler_run(tmp_path, "set", sets, False)
    _, _, ls_probe, _, _ = _handler_run(tmp_path, "probe", sets, False, perturb=1e-7)
    ls_dev, res_dev = dev_runs[0][2], dev_runs[0][1]
    diff = np.abs(ls_dev - ls_set)
    e_t = np.abs(ls_probe - ls_set)
    bound = 4.0 * np.maximum(e_t, 1e-6 * np.abs(ls_set))
    with capsys.disabled():
        print("\n[pcgnn handler] |device - set| per step (total, constraint):\n", diff)
        print("[pcgnn handler] set path's own deviation e_t after a 1e-7 relative move of its initial weights:\n", e_t)
        print("[pcgnn handler] bound 4 max(e_t, 1e-6 |loss_t|):\n", bound)
        print(f"[pcgnn handler] maxima: |device - set| {diff.max():.3e}, e_t {e_t.max():.3e}, AUC device {res_dev[3]:.6f} "
              f"set {res_set[3]:.6f}")
    np.testing.assert_allclose(ls_dev[0], ls_set[0], atol=1e-5, rtol=0)
    assert abs(res_dev[3] - res_set[3]) <= 1e-4
    assert (diff[1:] <= bound[1:]).all(), (diff[1:] - bound[1:]).max()
    capsys.readouterr()
    rp, ci = rels[1]
    row = 17
    a, b = int(rp[row]), int(rp[row + 1])
    rp_bad = rp.copy()
    rp_bad[row + 1:] -= b - a
    bad = [rels[0], (rp_bad, np.concatenate([ci[:a], ci[b:]])), rels[2]]
    cfg = dict(dev_runs[0][4], relations=bad)
    random.seed(72)
    with pytest.raises(ValueError, match=f"row {row} is empty"):
        ModelHandler(cfg).train()
