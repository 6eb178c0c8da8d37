"""The GraphSAGE epoch path (`ggad_amd/sage_epoch.py`, `ggad_sage_sum_adam_f32` / `ggad_sage_epoch_f32` of `csrc/sage.hip`, config key
`sage_epoch`): the fused sum / loss / Adam kernel against the step path's three launches bit for bit and against float64, the
reference fixture through `SageEpoch`, the epoch path against the step path over three epochs (eager and captured), and the
switch of `ModelHandler`."""
import random

import numpy as np
import pytest
import torch

import sage_fp64
from conftest import load_golden
from ggad_amd import synth
from test_sage_device_gpu import D0, K, N, _batch_nodes, _branch_graph, _table, _weights

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd import _lib
    from ggad_amd._lib import call
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import Encoder, FeatureTable, GraphSage, MeanAggregator
    from ggad_amd.sage_device import SageDevice
    from ggad_amd.sage_epoch import SageEpoch
    from ggad_amd.sampler import PyCompatRandom

DEV = "cuda:0"
SHAPES = [(1, 1), (17, 64), (64, 64), (17, 33), (64, 1), (1, 64)]
BATCHES = (1, 63, 64, 65, 200)
LR = 0.005


@pytest.fixture(scope="module")
def branch():
    rowptr, col = _branch_graph()
    return {"rowptr": rowptr, "col": col, "graph": DeviceGraph(rowptr, col, DEV)}


def _inputs(branch, b, f, d):
    """The inputs of `test_every_kernel_branch_against_the_float64_restatement`, labels mixed."""
    nodes = _batch_nodes(b)
    nbr, cnt = _table(branch["rowptr"], branch["col"], nodes, 100 + b)
    feat = synth.make_features(3 * N, f, 21)
    w_enc, w_cls = _weights(f, d, 100 * f + d)
    return nodes, nbr, cnt, feat, w_enc, w_cls, (np.arange(b) % 3 == 0).astype(np.int64)


class _State:
    """Both weights, their moments and step counters as `ggad_sage_sum_adam_f32` takes them."""

    def __init__(self, w_enc, w_cls):
        self.w = [torch.as_tensor(w_enc, device=DEV).clone(), torch.as_tensor(w_cls, device=DEV).clone()]
        self.m = [torch.zeros_like(w) for w in self.w]
        self.v = [torch.zeros_like(w) for w in self.w]
        self.c = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in self.w]

    def clone(self):
        other = _State(self.w[0], self.w[1])
        other.m, other.v, other.c = [t.clone() for t in self.m], [t.clone() for t in self.v], [t.clone() for t in self.c]
        return other

    def sum_adam(self, ws, rowloss, b, f, d, lr, wd, loss_out):
        call("ggad_sage_sum_adam_f32", ws.data_ptr(), rowloss.data_ptr(), b, f, d, self.w[0].data_ptr(), self.m[0].data_ptr(),
             self.v[0].data_ptr(), self.c[0].data_ptr(), self.w[1].data_ptr(), self.m[1].data_ptr(), self.v[1].data_ptr(),
             self.c[1].data_ptr(), lr, wd, loss_out.data_ptr())


@pytest.mark.parametrize("f,d", SHAPES)
def test_sum_adam_kernel_equals_the_step_paths_three_launches(branch, f, d):
    """`ggad_sage_sum_adam_f32` on the workspace `ggad_sage_bwd_f32` filled == that call's own sum, `k_sage_loss` and `FlatAdam.step`:
    weights, both moments, both counters and the loss bit for bit over three consecutive steps, B in {1, 63, 64, 65, 200}, weight
    decay 0 and 0.007.  Every step is launched twice from the same state, the loss slot poisoned with NaN before each launch.
    (64, 64) has 8,320 parameters, more than 8 per thread of the kernel's one workgroup; (1, 1) has 4."""
    for b in BATCHES:
        nodes, nbr, cnt, feat, w_enc, w_cls, labels = _inputs(branch, b, f, d)
        dev = SageDevice(branch["graph"], FeatureTable(torch.from_numpy(feat)), f, d, K)
        batch = dev.upload(nodes, nbr, cnt, labels)
        for wd in (0.0, 0.007):
            pe = torch.nn.Parameter(torch.from_numpy(w_enc).to(DEV))
            pc = torch.nn.Parameter(torch.from_numpy(w_cls).to(DEV))
            opt = FlatAdam([pc, pe], lr=LR, weight_decay=wd)
            mine = _State(w_enc, w_cls)
            for step in range(3):
                assert torch.equal(mine.w[0], pe.data) and torch.equal(mine.w[1], pc.data)
                out = dev.forward(batch, pe.data, pc.data)
                pe.grad, pc.grad = dev.backward(out["combined"], out["emb"], out["dscores"], pc.data)
                runs = []
                for _ in range(2):
                    st = mine.clone()
                    loss = torch.full((3,), float("nan"), device=DEV)
                    st.sum_adam(dev.ws, out["loss"][1:], b, f, d, LR, wd, loss[1:2])
                    runs.append((st, loss.cpu().numpy()))
                opt.step()
                want_loss = out["loss"][:1].cpu().numpy()
                for st, loss in runs:
                    where = (b, wd, step)
                    assert np.isnan(loss[0]) and np.isnan(loss[2]) and np.array_equal(loss[1:2], want_loss), where
                    for i, p in enumerate((pe, pc)):
                        m, v, c = opt.state[p]
                        assert torch.equal(st.w[i], p.data) and torch.equal(st.m[i], m) and torch.equal(st.v[i], v), where + (i,)
                        assert int(st.c[i]) == int(c) == step + 1, where
                mine = runs[0][0]
            assert np.isfinite(mine.w[0].cpu().numpy()).all() and float(mine.v[0].abs().max()) > 0


def test_unsupported_shapes_launch_nothing():
    st = _State(np.zeros((64, 2), dtype=np.float32), np.zeros((2, 64), dtype=np.float32))
    buf = torch.zeros(4096, device=DEV)
    lib = _lib.load()
    for f, d in ((65, 64), (17, 65), (0, 64), (17, 0)):
        rc = lib.ggad_sage_sum_adam_f32(buf.data_ptr(), buf.data_ptr(), 4, f, d, st.w[0].data_ptr(), st.m[0].data_ptr(),
                                        st.v[0].data_ptr(), st.c[0].data_ptr(), st.w[1].data_ptr(), st.m[1].data_ptr(),
                                        st.v[1].data_ptr(), st.c[1].data_ptr(), LR, 0.0, buf.data_ptr(), 0)
        assert rc == -4, (f, d)
    torch.cuda.synchronize()
    assert int(st.c[0]) == 0 and int(st.c[1]) == 0


def _cpu_steps(feat, nodes, nbr, cnt, w_enc, w_cls, labels, dtype, wd, steps):
    """`steps` optimiser steps in torch on the CPU at `dtype`: tests/sage_fp64.evaluate for loss and gradients, torch.optim.Adam."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    pe, pc = (torch.from_numpy(w.astype(np_dtype)).requires_grad_(True) for w in (w_enc, w_cls))
    opt = torch.optim.Adam([pe, pc], lr=LR, weight_decay=wd)
    out = []
    for _ in range(steps):
        ev = sage_fp64.evaluate(feat, nodes, nbr, cnt, pe.detach().numpy(), pc.detach().numpy(), labels, dtype)
        pe.grad, pc.grad = torch.from_numpy(ev["grad.enc"]).to(dtype), torch.from_numpy(ev["grad.cls"]).to(dtype)
        opt.step()
        rec = {"loss": ev["loss"]}
        for name, p in (("enc", pe), ("cls", pc)):
            s = opt.state[p]
            rec["weight." + name] = p.detach().double().numpy().copy()
            rec["exp_avg." + name] = s["exp_avg"].double().numpy().copy()
            rec["exp_avg_sq." + name] = s["exp_avg_sq"].double().numpy().copy()
        out.append(rec)
    return out


@pytest.mark.parametrize("f,d", SHAPES)
def test_sum_adam_kernel_against_float64(branch, f, d, capsys):
    """Three steps (forward, partial backward, `ggad_sage_sum_adam_f32`) on the inputs of the branch test against the same steps in
    float64 on the CPU (tests/sage_fp64.evaluate, torch.optim.Adam): the loss, both weights, `exp_avg` and `exp_avg_sq` of every
    step within max(4 x the error of the same restatement in float32, 1e-6 x the quantity's largest magnitude).  Every ratio is
    printed.  lr 0.005, weight decay 0.007, B in {1, 63, 64, 65, 200}.
    On an MI355X the device error is at most 0.64 of the bound (a weight at B = 200, F = 17, D = 33); the largest ratios to the
    float32 restatement's error -- 144 on a loss (B = 63, F = 1, D = 64), 6.8 on a weight, 6.9 on `exp_avg`, 11.2 on `exp_avg_sq`
    (B = 64, F = D = 1) -- occur where that restatement lands within 1e-9 relative of float64 and the 1e-6 limb decides: the
    device error there is 0.09 to 0.40 of it."""
    wd, failures = 0.007, []
    with capsys.disabled():
        for b in BATCHES:
            nodes, nbr, cnt, feat, w_enc, w_cls, labels = _inputs(branch, b, f, d)
            want = _cpu_steps(feat, nodes, nbr, cnt, w_enc, w_cls, labels, torch.float64, wd, 3)
            yard = _cpu_steps(feat, nodes, nbr, cnt, w_enc, w_cls, labels, torch.float32, wd, 3)
            dev = SageDevice(branch["graph"], FeatureTable(torch.from_numpy(feat)), f, d, K)
            batch = dev.upload(nodes, nbr, cnt, labels)
            st = _State(w_enc, w_cls)
            loss = torch.zeros(3, device=DEV)
            for step in range(3):
                out = dev.forward(batch, st.w[0], st.w[1])
                dev.backward(out["combined"], out["emb"], out["dscores"], st.w[1])
                st.sum_adam(dev.ws, out["loss"][1:], b, f, d, LR, wd, loss[step:step + 1])
                got = {"loss": loss[step:step + 1]}
                for i, name in enumerate(("enc", "cls")):
                    got["weight." + name], got["exp_avg." + name], got["exp_avg_sq." + name] = st.w[i], st.m[i], st.v[i]
                for key, g in got.items():
                    g = g.cpu().numpy().astype(np.float64)
                    assert g.shape == want[step][key].shape and np.isfinite(g).all(), key
                    err = float(np.abs(g - want[step][key]).max())
                    err32 = float(np.abs(yard[step][key] - want[step][key]).max())
                    bound = max(4.0 * err32, 1e-6 * float(np.abs(want[step][key]).max()))
                    print(f"\n[sage sum_adam B={b} F={f} D={d} step {step}] {key}: device {err:.3e} float32 {err32:.3e} "
                          f"ratio {err / max(err32, 1e-30):.2f} bound {bound:.3e}", end="")
                    if err > bound:
                        failures.append((b, step, key, err, err32, bound))
        print()
    assert not failures, failures


def _fixture_model(g, path):
    f, d = int(g["f"]), int(g["d"])
    feats = FeatureTable(torch.from_numpy(g["feat"]))
    graph = DeviceGraph(g["rowptr"], g["col"], DEV)
    agg = MeanAggregator(feats, cuda=True)
    rng = None
    if path == "epoch":
        rng = PyCompatRandom.from_python_state(random.getstate())
        enc = Encoder(feats, f, d, graph, agg, gcn=False, cuda=True, sage_device=SageDevice(graph, feats, f, d, 10, rng=rng))
    else:
        enc = Encoder(feats, f, d, synth.csr_to_adj_lists(g["rowptr"], g["col"]), agg, gcn=False, cuda=True)
    enc.num_samples = 5
    model = GraphSage(2, enc).to(DEV)
    with torch.no_grad():
        enc.weight.copy_(torch.from_numpy(g["init.enc.weight"]))
        model.weight.copy_(torch.from_numpy(g["init.weight"]))
    opt = FlatAdam([p for p in model.parameters() if p.requires_grad], lr=0.001, weight_decay=0.007)
    return enc, model, opt, rng


def test_reference_fixture_on_the_epoch_path(capsys):
    """The two-epoch loop of `test_reference_fixture_on_the_device_path` through `SageEpoch` (epoch 0 eager, epoch 1 a replayed
    capture sampled ahead): the batches of the fixture, the `random` stream at the fixture's position after the three test chunks,
    losses within 2e-6, final weights and `to_prob` within 3e-6, each bound max(that, 4 x the set path's own error)."""
    g = load_golden("minibatch_sage.npz")
    labels = g["labels"]
    bs, nb, n_pseudo = 40, 4, 10
    errs = {}
    for path in ("set", "epoch"):
        random.seed(72)
        enc, model, opt, rng = _fixture_model(g, path)
        losses = []
        if path == "epoch":
            idx_train = np.arange(100, 700, dtype=np.int64)
            idx_anomaly = np.nonzero(labels)[0][:60].astype(np.int64)
            runner = SageEpoch(enc.device_path, enc.weight, model.weight, opt, idx_train, idx_anomaly, labels, bs, n_pseudo, nb)
            for epoch in range(2):
                losses.extend(float(l) for l in runner.run_epoch("epoch" if epoch == 0 else None))
                nodes = runner.table.view(nb, -1)[:, :bs + n_pseudo].cpu().numpy()
                assert np.array_equal(nodes, g["batches"][epoch * nb:(epoch + 1) * nb])
            assert runner.replays == 1 and runner.graph is not None
        else:
            idx_train = list(range(100, 700))
            idx_anomaly = [int(i) for i in np.nonzero(labels)[0][:60]]
            for epoch in range(2):
                random.shuffle(idx_train)
                for b in range(nb):
                    random.shuffle(idx_anomaly)
                    batch_nodes = idx_train[b * bs:(b + 1) * bs] + idx_anomaly[:n_pseudo]
                    opt.zero_grad()
                    loss = model.loss(batch_nodes, torch.as_tensor(labels[np.array(batch_nodes)], device=DEV).long())
                    loss.backward()
                    opt.step()
                    losses.append(loss.item())
        test_nodes = g["test_nodes"].tolist()
        with torch.no_grad():
            probs = torch.cat([model.to_prob(test_nodes[s:s + 30]) for s in range(0, 90, 30)]).cpu().numpy()
        state = rng.to_python_state() if rng is not None else random.getstate()
        assert np.array_equal(np.array(state[1], dtype=np.uint64), g["py_random_after"]), path
        errs[path] = {"losses": float(np.abs(np.array(losses) - g["losses"]).max()),
                      "final.enc.weight": float(np.abs(enc.weight.detach().cpu().numpy() - g["final.enc.weight"]).max()),
                      "final.weight": float(np.abs(model.weight.detach().cpu().numpy() - g["final.weight"]).max()),
                      "to_prob": float(np.abs(probs - g["test_probs"]).max())}
    project = {"losses": 2e-6, "final.enc.weight": 3e-6, "final.weight": 3e-6, "to_prob": 3e-6}
    failures = []
    with capsys.disabled():
        for key, bound in project.items():
            final = max(bound, 4.0 * errs["set"][key])
            print(f"\n[sage epoch fixture] {key}: epoch {errs['epoch'][key]:.3e} set {errs['set'][key]:.3e} bound {final:.3e}", end="")
            if errs["epoch"][key] > final:
                failures.append((key, errs["epoch"][key], final))
        print()
    assert not failures, failures


def _three_epochs(branch, mode):
    """Three epochs on the branch graph, F = 17, D = 64: 102 train ids (every special degree but 0, the hub twice) in batches of
    25 + 8 over 5 steps -- the last one short (2 + 8 rows) --, a pool of 12.  mode: "step" (the `sage_device` loop of the handler),
    "eager" or "captured" (`SageEpoch`)."""
    f, d, bs, nb, n_pseudo = 17, 64, 25, 5, 8
    from test_sage_epoch_cpu import _branch_lists
    train, pool = _branch_lists(False)
    train = np.ascontiguousarray(train[train != D0])
    assert len(train) == 102
    labels = (np.random.default_rng(3).random(3 * N) < 0.3).astype(np.int64)
    feats = FeatureTable(torch.from_numpy(synth.make_features(3 * N, f, 21)))
    rng = PyCompatRandom(5)
    sage = SageDevice(branch["graph"], feats, f, d, K, rng=rng)
    enc = Encoder(feats, f, d, branch["graph"], MeanAggregator(feats, cuda=True), gcn=False, cuda=True, sage_device=sage)
    model = GraphSage(2, enc).to(DEV)
    w_enc, w_cls = _weights(f, d, 9)
    with torch.no_grad():
        enc.weight.copy_(torch.from_numpy(w_enc))
        model.weight.copy_(torch.from_numpy(w_cls))
    opt = FlatAdam([p for p in model.parameters() if p.requires_grad], lr=LR, weight_decay=0.007)
    losses = []
    runner = None
    if mode != "step":
        runner = SageEpoch(sage, enc.weight, model.weight, opt, train, pool, labels, bs, n_pseudo, nb, capture=mode == "captured")
        assert runner.lens.tolist() == [33, 33, 33, 33, 10]
    for epoch in range(3):
        if runner is not None:
            losses.extend(float(l) for l in runner.run_epoch("epoch" if epoch < 2 else None))
            continue
        rng.shuffle(train)
        for b in range(nb):
            i0, i1 = b * bs, min((b + 1) * bs, len(train))
            rng.shuffle(pool)
            nodes = np.concatenate([train[i0:i1], pool[:n_pseudo]])
            opt.zero_grad()
            loss = model.loss(nodes, labels[nodes])
            loss.backward()
            opt.step()
            losses.append(float(loss.item()))
    got = {"losses": np.array(losses), "train": train, "pool": pool, "rng": np.array(rng.to_python_state()[1], dtype=np.uint64)}
    for name, p in (("enc", enc.weight), ("cls", model.weight)):
        m, v, c = opt.state[p]
        got.update({"w." + name: p.detach().cpu().numpy(), "m." + name: m.cpu().numpy(), "v." + name: v.cpu().numpy(),
                    "c." + name: c.cpu().numpy()})
    return got, runner


def test_epoch_path_equals_the_step_path_eager_and_captured(branch):
    """Every loss, both weights, both moments, the step counters, both shuffled lists and the generator state after three epochs:
    eager == step path and captured == eager, bit for bit.  The captured run samples epochs 1 and 2 ahead of the device."""
    step, _ = _three_epochs(branch, "step")
    eager, r_eager = _three_epochs(branch, "eager")
    captured, r_cap = _three_epochs(branch, "captured")
    assert r_eager.replays == 0 and r_eager.graph is None and r_cap.replays == 2 and r_cap.epochs_run == 3
    assert step["losses"].shape == (15,) and np.isfinite(step["losses"]).all()
    assert step["c.enc"].tolist() == [15] and step["c.cls"].tolist() == [15]
    for key in step:
        assert np.array_equal(step[key], eager[key]), ("eager", key)
        assert np.array_equal(eager[key], captured[key]), ("captured", key)


def _handler_run(tmp_path, tag, **keys):
    """The configuration of `test_model_handler_trains_from_csr_on_the_device_path` plus `keys`."""
    import ggad_amd.model_handler as mh
    n = 3000
    rowptr, col = synth.make_graph(n, 30000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab.copy()), seed=72, model="SAGE",
               multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=3,
               valid_epochs=2, num_batches=6, n_pseudo=20, save_dir=str(tmp_path) + f"/{tag}/", test_ratio=0.67, device=0, **keys)
    random.seed(72)
    np.random.seed(72)
    torch.manual_seed(72)
    h = mh.ModelHandler(cfg)
    res = h.train()
    sd = {k: v.detach().cpu().numpy().copy() for k, v in h.model.state_dict().items()}
    return h, res, np.array(h.sage_losses), sd, random.getstate()


def test_model_handler_switch(tmp_path, capsys):
    """`sage_epoch: true` beside `sage_device: true`: the runner exists and replayed epochs 1 and 2; the 18 losses, the 5-tuple, the
    state_dict and python's `random` state after `train()` equal the `sage_device` run's exactly; "Restore model" is printed;
    `sage_epoch` alone is a ValueError that names both keys."""
    h_dev, res_dev, ls_dev, sd_dev, state_dev = _handler_run(tmp_path, "dev", sage_device=True)
    assert getattr(h_dev, "sage_epoch", None) is None
    capsys.readouterr()
    h_ep, res_ep, ls_ep, sd_ep, state_ep = _handler_run(tmp_path, "epoch", sage_device=True, sage_epoch=True)
    assert "Restore model from epoch" in capsys.readouterr().out
    assert isinstance(h_ep.sage_epoch, SageEpoch) and h_ep.sage_epoch.epochs_run == 3 and h_ep.sage_epoch.replays == 2
    assert ls_ep.shape == (18,) and np.isfinite(ls_ep).all() and np.array_equal(ls_ep, ls_dev)
    assert len(res_ep) == 5 and res_ep == res_dev
    assert sd_ep.keys() == sd_dev.keys()
    for k in sd_dev:
        assert np.array_equal(sd_ep[k], sd_dev[k]), k
    assert state_ep == state_dev
    with pytest.raises(ValueError, match="(?s)sage_epoch.*sage_device"):
        _handler_run(tmp_path, "alone", sage_epoch=True)
