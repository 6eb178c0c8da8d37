"""The fused HIP head of the PC-GNN device path (`csrc/pcgnn_head.hip`, `pcgnn_device.PcgnnHeadFn`, config key `pcgnn_fused`):
parity with the imported reference, every branch against the float64 restatement (tests/pcgnn_head_fp64.py), determinism into
poisoned buffers, the forward-only mode, the handler switch and the errors raised before a launch."""
import random

import numpy as np
import pytest
import torch

import pcgnn_fp64
import pcgnn_head_fp64 as H
from conftest import load_golden
from ggad_amd import synth

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd import _lib
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import FeatureTable
    from ggad_amd.layers import InterAgg, IntraAgg, PCALayer
    from ggad_amd.pcgnn_device import PcgnnHeadFn, pcgnn_head_forward

DEV = "cuda:0"


def _model(graphs, feat, f, d, weights, fused=True):
    feats = FeatureTable(torch.from_numpy(feat))
    intras = [IntraAgg(feats, f, d, [], 0.5, cuda=True) for _ in range(3)]
    inter = InterAgg(feats, f, d, [], graphs, intras, inter="GNN", cuda=True, fused=fused)
    model = PCALayer(2, inter, 2)
    sd = model.state_dict()
    with torch.no_grad():
        for k in pcgnn_fp64.PARAMS:
            sd[k].copy_(torch.from_numpy(weights[k]))
    return inter, model


def _golden_model(fused=True):
    g = load_golden("minibatch_pcgnn.npz")
    f, d = int(g["f"]), int(g["d"])
    graphs = [DeviceGraph(g[f"rowptr{k}"], g[f"col{k}"], DEV) for k in range(3)]
    inter, model = _model(graphs, g["feat"], f, d, {k: g["init." + k] for k in pcgnn_fp64.PARAMS}, fused)
    return g, inter, model


def test_reference_parity_with_the_fused_head():
    """`InterAgg` + `PCALayer` on `DeviceGraph` relations with `fused` on against the imported reference classes
    (tests/golden/minibatch_pcgnn.npz): the embeddings and the affinity the head computed, the (loss, margin term) pair, the gradient
    of every parameter and both `to_prob` outputs, with the bounds of test_reference_parity_on_device_graph_relations."""
    g, inter, model = _golden_model()
    dp = inter.device_path
    assert dp is not None and dp.fused
    nodes, labels = g["nodes"].tolist(), torch.from_numpy(g["labels"]).to(DEV)
    b, d = len(nodes), int(g["d"])
    loss, lcon = model.loss(nodes, labels, True)
    combined = dp.last_head["ws"][:b * d].view(b, d)
    np.testing.assert_allclose(combined.t().cpu().numpy(), g["combined"], atol=3e-6, rtol=0)
    np.testing.assert_allclose(dp.last_head["affinity"].cpu().numpy(), g["affinity"], atol=3e-6, rtol=0)
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


def _run_head(t1s, nbs, w, w_cls, y, buffers=None):
    """The head function fed directly; returns numpy arrays over H.KEYS (gradients of the total, incoming gradient 1)."""
    dev = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (t1s[0], nbs[0], t1s[1], nbs[1], t1s[2], nbs[2], w, w_cls)]
    total, con, scores, affinity = PcgnnHeadFn.apply(*dev, torch.from_numpy(y).to(DEV), buffers)
    assert total.shape == con.shape == (1,) and not con.requires_grad and not scores.requires_grad and not affinity.requires_grad
    total.backward()
    out = {"scores": scores, "affinity": affinity, "loss": torch.cat([total, con]), "d_w": dev[6].grad, "d_cls": dev[7].grad}
    for r in range(3):
        out[f"d_t1_{r}"], out[f"d_nb_{r}"] = dev[2 * r].grad, dev[2 * r + 1].grad
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


@pytest.mark.parametrize("d", [1, 33, 64])
@pytest.mark.parametrize("b", [1, 2, 63, 64, 65, 200, 257])
def test_every_branch_against_the_float64_restatement(b, d):
    """B below, at and above one wave of rows and one group of four, B not a multiple of the eight row ranges, D = 1, odd and full;
    mixed labels, one class only (its other mean is 0 / 0: NaN in the loss pair, finite gradients), exactly one positive, a row whose
    `combined` is all zero and one whose `neigh` is.  The device's error against the float64 restatement is at most 4 x the error of
    the SAME restatement in float32, or 1e-6 x the quantity's largest magnitude where that is more (the rule of
    tests/test_sage_device_gpu.py); NaN positions coincide.  Every figure is printed before the assertion.  On an MI355X the device
    error is at most 0.6 x that bound (scores 0.59, dW 0.47, the dT1 0.38, the dNB 0.29, dW_cls 0.28, affinity 0.21, the loss pair
    0.14)."""
    failures = []
    for name, t1s, nbs, w, w_cls, y in H.cases(b, d, 1000 * b + d):
        want = H.head(t1s, nbs, w, w_cls, y, np.float64)
        yard = H.head(t1s, nbs, w, w_cls, y, np.float32)
        got = _run_head(t1s, nbs, w, w_cls, y)
        for key in H.KEYS:
            assert got[key].shape == want[key].shape and got[key].dtype == np.float32, (name, key)
            nan = np.isnan(want[key])
            assert np.array_equal(np.isnan(got[key]), nan), (name, key)
            if key != "loss":
                assert not nan.any(), (name, key)
            if nan.all():
                print(f"[pcgnn head B={b} D={d} {name}] {key}: NaN on both sides")
                continue
            err = float(np.abs(got[key] - want[key])[~nan].max())
            err32 = float(np.abs(yard[key].astype(np.float64) - want[key])[~nan].max())
            bound = max(4.0 * err32, 1e-6 * float(np.abs(want[key][~nan]).max()))
            print(f"[pcgnn head B={b} D={d} {name}] {key}: device {err:.3e} float32 {err32:.3e} ratio {err / max(err32, 1e-30):.2f} "
                  f"bound {bound:.3e}")
            if err > bound:
                failures.append((name, key, err, err32, bound))
    assert not failures, failures


def _poisoned(b, d, value):
    lib = _lib.load()
    sizes = {"scores": 2 * b, "affinity": b, "loss": 2, "grads": 6 * b * d + 3 * d * d + 2 * d,
             "ws": int(lib.ggad_pcgnn_head_workspace_elems(b, d))}
    return {k: torch.full((n,), value, dtype=torch.float32, device=DEV) for k, n in sizes.items()}


def test_same_inputs_give_the_same_bits_into_poisoned_buffers():
    """Two training calls on the same inputs, the outputs, gradients and workspace pre-filled with 1e30 the first time and with NaN
    the second: every result is bit-equal and finite (nothing is read before it is written, every element is written).  Then the
    forward-only entry with poisoned gradient and workspace buffers handed in: scores and affinity equal the training call's bits,
    the loss, the gradients and the workspace keep the poison."""
    b, d = 65, 33
    _, t1s, nbs, w, w_cls, y = H.cases(b, d, 4)[0]
    bufs = [_poisoned(b, d, 1e30), _poisoned(b, d, float("nan"))]
    runs = [_run_head(t1s, nbs, w, w_cls, y, bf) for bf in bufs]
    for k in H.KEYS:
        assert np.isfinite(runs[0][k]).all() and np.array_equal(runs[0][k], runs[1][k]), k
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bufs[0]["grads"]).all()) and torch.equal(bufs[0]["grads"], bufs[1]["grads"])
    assert bool(torch.isfinite(bufs[0]["ws"]).all()) and torch.equal(bufs[0]["ws"], bufs[1]["ws"])
    dev = [torch.from_numpy(a).to(DEV) for a in (*t1s, *nbs, w, w_cls)]
    p = _poisoned(b, d, 7.0)
    offs = np.concatenate([[0], np.cumsum([b * d] * 6 + [3 * d * d, 2 * d])])[:8]
    _lib.call("ggad_pcgnn_head_f32", *[t.data_ptr() for t in dev], 0, b, d, p["scores"].data_ptr(), p["affinity"].data_ptr(), 0,
              *[p["grads"].data_ptr() + 4 * int(o) for o in offs], p["ws"].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(p["scores"].view(b, 2).cpu().numpy(), runs[0]["scores"])
    assert np.array_equal(p["affinity"].cpu().numpy(), runs[0]["affinity"])
    for k in ("loss", "grads", "ws"):
        assert bool((p[k] == 7.0).all()), k
    scores, affinity = pcgnn_head_forward(dev[:3], dev[3:6], dev[6], dev[7])
    assert np.array_equal(scores.cpu().numpy(), runs[0]["scores"]) and np.array_equal(affinity.cpu().numpy(), runs[0]["affinity"])


def test_to_prob_equals_the_training_forward():
    """`to_prob` with `fused` on (one forward-only launch behind the relations) gives the scores and the affinity of the training call
    on the same batch, bit for bit; with `fused` off the same model gives them to float32 rounding."""
    g, inter, model = _golden_model()
    nodes, labels = g["nodes"].tolist(), torch.from_numpy(g["labels"]).to(DEV)
    model.loss(nodes, labels, True)
    last = inter.device_path.last_head
    scores, affinity = last["scores"].view(-1, 2).clone(), last["affinity"].clone()
    with torch.no_grad():
        pg, pl = model.to_prob(nodes, labels, False)
        s2, a2 = inter.device_path.head_forward(inter, model.weight, nodes)
    assert torch.equal(s2, scores) and torch.equal(a2, affinity)
    assert torch.equal(pg, torch.sigmoid(scores)) and torch.equal(pl, torch.sigmoid(affinity))
    inter.device_path.fused = False
    with torch.no_grad():
        s3, a3 = model.forward(nodes, labels, False)
    np.testing.assert_allclose(s3.cpu().numpy(), scores.cpu().numpy(), atol=3e-6, rtol=0)
    np.testing.assert_allclose(a3.cpu().numpy(), affinity.cpu().numpy(), atol=3e-6, rtol=0)


def _handler_run(tmp_path, tag, rels, fused, perturb=0.0):
    """The configuration of test_model_handler_trains_from_csr_relations_on_the_device_path, `pcgnn_device` on."""
    import ggad_amd.layers as layers
    from ggad_amd.model_handler import ModelHandler
    n = 3000
    rp0, ci0 = synth.make_graph(n, 30000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    cfg = dict(data_name="synthetic", data_dir="", data=(synth.csr_to_adj_lists(rp0, ci0), feat, lab.copy()), relations=rels, seed=72,
               model="PCGNN", multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60,
               num_epochs=3, valid_epochs=2, num_batches=5, n_pseudo=20, save_dir=str(tmp_path) + f"/{tag}/", test_ratio=0.67,
               device=0, rho=0.5, alpha=2, pcgnn_device=True)
    if fused:
        cfg["pcgnn_fused"] = True
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
    state = random.getstate()
    return h, res, np.array(h.pcgnn_losses), {k: v.detach().cpu().numpy().copy() for k, v in h.model.state_dict().items()}, state


def test_model_handler_with_the_fused_head(tmp_path, capsys):
    """`pcgnn_device + pcgnn_fused` against `pcgnn_device` alone: every loss pair within 4 x max(e_t, 1e-6 |loss_t|), e_t the unfused
    device path's own deviation after its initial weights moved by 1e-7 relative (measured here); the same five-tuple to 1e-4; the
    same python `random` state at the end; two fused runs bit-identical.  The series and their maxima are printed."""
    n = 3000
    rels = [synth.make_graph(n, 20000 + 5000 * k, 11 + k, kind="powerlaw", max_degree=150) for k in range(3)]
    fused_runs = [_handler_run(tmp_path, f"fused{rep}", rels, True) for rep in range(2)]
    for h, res, ls, sd, _ in fused_runs:
        assert h.model.inter1.device_path is not None and h.model.inter1.device_path.fused
        assert len(res) == 5 and all(np.isfinite(r) for r in res[:4]) and 0.0 <= res[3] <= 1.0
        assert ls.shape == (15, 2) and np.isfinite(ls).all() and (ls[:, 0] >= 5 * ls[:, 1] - 1e-5).all()
    assert np.array_equal(fused_runs[0][2], fused_runs[1][2])
    for k in fused_runs[0][3]:
        assert np.array_equal(fused_runs[0][3][k], fused_runs[1][3][k]), k
    h_dev, res_dev, ls_dev, _, state_dev = _handler_run(tmp_path, "dev", rels, False)
    assert not h_dev.model.inter1.device_path.fused
    _, _, ls_probe, _, _ = _handler_run(tmp_path, "probe", rels, False, perturb=1e-7)
    capsys.readouterr()
    ls_fused, res_fused = fused_runs[0][2], fused_runs[0][1]
    diff = np.abs(ls_fused - ls_dev)
    e_t = np.abs(ls_probe - ls_dev)
    bound = 4.0 * np.maximum(e_t, 1e-6 * np.abs(ls_dev))
    with capsys.disabled():
        print("\n[pcgnn fused handler] |fused - device| per step (total, constraint):\n", diff)
        print("[pcgnn fused handler] device path's own deviation e_t after a 1e-7 relative move of its initial weights:\n", e_t)
        print("[pcgnn fused handler] bound 4 max(e_t, 1e-6 |loss_t|):\n", bound)
        print(f"[pcgnn fused handler] maxima: |fused - device| {diff.max():.3e}, e_t {e_t.max():.3e}; five-tuple fused {res_fused} "
              f"device {res_dev}")
    assert (diff <= bound).all(), (diff - bound).max()
    np.testing.assert_allclose(np.array(res_fused, dtype=np.float64), np.array(res_dev, dtype=np.float64), atol=1e-4, rtol=0)
    assert fused_runs[0][4] == state_dev


def test_bad_shapes_and_tensors_raise_before_a_launch():
    b, d = 8, 16
    _, t1s, nbs, w, w_cls, y = H.cases(b, d, 2)[0]
    good = [torch.from_numpy(a).to(DEV) for a in (t1s[0], nbs[0], t1s[1], nbs[1], t1s[2], nbs[2], w, w_cls)]
    yd = torch.from_numpy(y).to(DEV)
    lib = _lib.load()
    assert lib.ggad_pcgnn_head_supported(1, 64) == 1 and lib.ggad_pcgnn_head_supported(1, 65) == 0
    assert lib.ggad_pcgnn_head_supported(0, 64) == 0 and lib.ggad_pcgnn_head_supported(5, 0) == 0
    assert lib.ggad_pcgnn_head_workspace_elems(5, 65) == 0
    assert lib.ggad_pcgnn_head_workspace_elems(b, d) == 4 * b * d + 3 * b + lib.ggad_pcgnn_head_parts() * (3 * d * d + 2 * d)
    wide = [torch.zeros(b, 65, device=DEV)] * 6 + [torch.zeros(195, 65, device=DEV), torch.zeros(2, 65, device=DEV)]
    with pytest.raises(ValueError, match="embed_dim <= 64"):
        PcgnnHeadFn.apply(*wide, yd)
    with pytest.raises(ValueError, match="embed_dim <= 64"):
        pcgnn_head_forward(wide[0:6:2], wide[1:6:2], wide[6], wide[7])
    p = [t.data_ptr() for t in wide]                                       # the C entry refuses the shape too, and launches nothing
    out = torch.full((4 * b,), 3.0, device=DEV)
    rc = lib.ggad_pcgnn_head_f32(*p, 0, b, 65, out.data_ptr(), out.data_ptr() + 8 * b, *([0] * 10), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == _lib.GGAD_E_UNSUPPORTED and bool((out == 3.0).all())
    for i, bad in ((0, good[0].t().contiguous().t()), (3, good[3].double()), (6, good[6][:, ::2]), (7, good[7].cpu()),
                   (2, good[2][:-1])):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            PcgnnHeadFn.apply(*args, yd)
    for bad_y in (yd[:-1], yd.int(), torch.cat([yd, yd])[::2], torch.cat([yd, yd[:1]])):
        with pytest.raises(ValueError):
            PcgnnHeadFn.apply(*good, bad_y)
    feats = FeatureTable(torch.zeros(4, 3))
    intras = [IntraAgg(feats, 3, 2, [], 0.5, cuda=True) for _ in range(3)]
    sets = [{i: {i} for i in range(4)} for _ in range(3)]
    with pytest.raises(ValueError, match="pcgnn_fused.*pcgnn_device"):
        InterAgg(feats, 3, 2, [], sets, intras, cuda=True, fused=True)
