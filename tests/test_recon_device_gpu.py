"""The optimiser steps and the validation score of the mini-batch DOMINANT / AnomalyDAE handlers in the fused kernels of
`csrc/recon_mb.hip` (`ggad_amd/recon_device.py`): every branch of one step against the float64 restatement (tests/recon_mb_fp64.py), the
Adam update against `ggad_adam_multi_f32` bit for bit, the recorded five-step trajectory, ragged schedules, determinism, the scores,
the `recon_device` switch of the handlers, and the errors raised before any launch.

Yardstick of the measured bounds: on the same inputs e_def = the max-abs error of the default path (`LinearFn` + `ggad_recon_cols_f32`
+ `FlatAdam`) against the restatement; the device path must stay within max(4 e_def, 1e-6 max|reference|) -- the factor 4 for a
different summation order over at most 256 terms."""
import importlib
import random
import types

import numpy as np
import pytest
import torch

import recon_mb_fp64 as R
from conftest import load_golden
from ggad_amd import synth
from oracle import ggad_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd import graphsage_dominant as GD
    from ggad_amd._lib import load
    from ggad_amd.fullgraph import FlatAdam, LinearFn
    from ggad_amd.recon_device import ReconDevice
    from ggad_amd.sage_utils import recon_scores

DEV = "cuda:0"
KEYS = ("loss", "grad.w", "grad.fc", "w", "fc")
TAGS = [("dominant", "ggad_amd.graphsage_dominant", (1.0, 1.0)), ("anomalydae", "ggad_amd.graphsage_anomalydae", (0.5, 0.5))]


def _max_rows(f):
    return int(load().ggad_recon_mb_max_rows(f))


def _params(w, wfc, state, counts, wd):
    """The two tensors as parameters on the GPU with a `FlatAdam` whose state is (a copy of) `state` / `counts`."""
    W = torch.nn.Parameter(torch.from_numpy(np.asarray(w, dtype=np.float32).copy()).to(DEV))
    FC = torch.nn.Parameter(torch.from_numpy(np.asarray(wfc, dtype=np.float32).copy()).to(DEV))
    opt = FlatAdam([W, FC], lr=R.LR, weight_decay=wd)
    if state is not None or counts != (0, 0):
        st = state if state is not None else [np.zeros_like(w), np.zeros_like(w), np.zeros_like(wfc), np.zeros_like(wfc)]
        for i, p in enumerate((W, FC)):
            opt.state[p] = (torch.from_numpy(st[2 * i].copy()).to(DEV), torch.from_numpy(st[2 * i + 1].copy()).to(DEV),
                            torch.tensor([counts[i]], dtype=torch.int32, device=DEV))
    return W, FC, opt


def _collect(loss, gw, gf, W, FC, opt):
    got = {"loss": loss.detach().reshape(1), "grad.w": gw, "grad.fc": gf, "w": W.detach(), "fc": FC.detach(),
           "m.w": opt.state[W][0], "v.w": opt.state[W][1], "m.fc": opt.state[FC][0], "v.fc": opt.state[FC][1],
           "c.w": opt.state[W][2], "c.fc": opt.state[FC][2]}
    return {k: v.detach().cpu().numpy().copy() for k, v in got.items()}


def _stub_encoder(W, FC):
    return types.SimpleNamespace(feat_dim=int(W.shape[1]), embed_dim=int(W.shape[0]), weight=W, fc=types.SimpleNamespace(weight=FC))


def _default_steps(x1, t, bp, w, wfc, state=None, counts=(0, 0), wp=1.0, wn=1.0, wd=R.WD):
    """The handler's default path on the rows bp cuts: losses and what the last step left."""
    W, FC, opt = _params(w, wfc, state, counts, wd)
    xd, td = torch.from_numpy(x1).to(DEV), torch.from_numpy(t).to(DEV)
    losses = []
    for i in range(len(bp) - 1):
        opt.zero_grad()
        lo, hi = int(bp[i]), int(bp[i + 1])
        r = LinearFn.apply(LinearFn.apply(xd[lo:hi], W, True), FC, True)
        loss = GD._ReconCols.apply(r, td[lo:hi], wp, wn)
        loss.backward()
        gw, gf = W.grad.clone(), FC.grad.clone()
        opt.step()
        losses.append(loss.detach().reshape(1))
    got = _collect(loss, gw, gf, W, FC, opt)
    got["losses"] = torch.cat(losses).cpu().numpy().astype(np.float64)
    return got


def _device_steps(x1, t, bp, w, wfc, state=None, counts=(0, 0), wp=1.0, wn=1.0, wd=R.WD, launches=None):
    """`ReconDevice.steps` on a fresh stub encoder: one launch over bp, or one launch per group of `launches` consecutive steps."""
    W, FC, opt = _params(w, wfc, state, counts, wd)
    rd = ReconDevice().bind(_stub_encoder(W, FC), opt)
    xd, td = torch.from_numpy(x1).to(DEV), torch.from_numpy(t).to(DEV)
    n = len(bp) - 1
    k = n if launches is None else launches
    losses = []
    for s0 in range(0, n, k):
        lo, hi = int(bp[s0]), int(bp[min(n, s0 + k)])
        losses.append(rd.steps(xd[lo:hi], td[lo:hi], np.asarray(bp[s0:s0 + k + 1]) - lo, wp, wn).clone())
    assert W.grad is rd.grads[0] and FC.grad is rd.grads[1]
    got = _collect(losses[-1][-1], W.grad, FC.grad, W, FC, opt)
    got["losses"] = torch.cat(losses).cpu().numpy().astype(np.float64)
    return got


def _first_step_masks(want, w, wfc, wd=R.WD, floor=1e-6):
    """Which parameter elements a FIRST Adam step (zero moments) determines well.  There p -= lr g / (|g| + 1e-8) with g = grad + wd p:
    the sign of g, whatever its size, so where grad and wd p cancel the float32 rounding of the gradient decides the result -- in any
    implementation (the reason parameters are not asserted at wd = 0 at all).  d p / d g = lr 1e-8 / (|g| + 1e-8)^2 <= 10 lr at
    |g| >= 1e-6, which turns a gradient error of 1e-8 into 1e-10; below that the element is left to the gradient check and to the
    bit-for-bit Adam test.  Decided from the float64 restatement alone."""
    return {"w": np.abs(want["grad.w"] + wd * np.asarray(w, np.float64)) >= floor,
            "fc": np.abs(want["grad.fc"] + wd * np.asarray(wfc, np.float64)) >= floor}


def _judge(tag, got, yard, want, keys, capsys, finite_yard=None, masks=None):
    """Prints every figure, then holds `got` to max(4 x the yardstick's own error, 1e-6 max|want|) per key (over the elements of
    masks[key] where one is given)."""
    failures = []
    with capsys.disabled():
        for key in keys:
            assert got[key].shape == want[key].shape and np.isfinite(got[key]).all(), key
            y = yard[key] if np.isfinite(yard[key]).all() or finite_yard is None else finite_yard[key]
            keep = np.ones(want[key].shape, dtype=bool) if masks is None or key not in masks else masks[key]
            assert keep.mean() > 0.98, (key, keep.mean())
            err, e_def = float(np.abs(got[key] - want[key])[keep].max()), float(np.abs(y - want[key])[keep].max())
            bound = max(4.0 * e_def, 1e-6 * float(np.abs(want[key]).max()))
            print(f"\n[recon_mb {tag}] {key}: device {err:.3e} default {e_def:.3e} ratio {err / max(e_def, 1e-30):.2f} "
                  f"bound {bound:.3e}" + (f" ({int((~keep).sum())} of {keep.size} elements left out)" if not keep.all() else ""), end="")
            if not err <= bound:
                failures.append((key, err, e_def, bound))
        print()
    assert not failures, failures


def test_the_library_takes_what_the_tests_assume():
    lib = load()
    assert lib.ggad_abi_version() == 11
    assert _max_rows(17) >= 256 and _max_rows(32) >= 256 and _max_rows(64) >= 150
    assert lib.ggad_recon_mb_supported(1, 64, 1) and lib.ggad_recon_mb_supported(64, 64, _max_rows(64))
    assert not lib.ggad_recon_mb_supported(64, 64, _max_rows(64) + 1) and not lib.ggad_recon_mb_supported(17, 32, 48)


def _shapes():
    return [(1, 1), (2, 17), (48, 17), (150, 17), (150, 64), (None, 32)]


@pytest.mark.parametrize("weights", R.WEIGHTS)
@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: f"{s[0] or 'max'}x{s[1]}")
def test_single_step_branches(shape, weights, capsys):
    """B = 1 (one row in one block), 2, 48 (the fixture's batch: waves 12 .. 15 idle), 150 (the handler's batch: a ragged last block),
    the row limit at F = 32 (every row block of every wave) and B = 150 at F = 64 (every owner thread, the LDS limit in reach);
    F = 1, 17, 32, 64.  Loss, both raw gradients and both parameters after Adam with weight decay 0.007 (the parameters over the
    elements `_first_step_masks` keeps)."""
    b, f = shape
    b = _max_rows(f) if b is None else b
    x1, t, w, wfc = R.make_case(b, f, 1000 * b + f)
    want = R.step(x1, t, w, wfc, w_pos=weights[0], w_neg=weights[1])
    yard = _default_steps(x1, t, [0, b], w, wfc, wp=weights[0], wn=weights[1])
    got = _device_steps(x1, t, [0, b], w, wfc, wp=weights[0], wn=weights[1])
    _judge(f"step B={b} F={f} w={weights}", got, yard, want, KEYS, capsys, masks=_first_step_masks(want, w, wfc))
    assert got["c.w"][0] == 1 and got["c.fc"][0] == 1


def test_dead_hidden_channel_dead_output_column_and_a_started_optimiser(capsys):
    """A row of W negative enough that h = 0 for the whole batch; an output column with r = 0 against a zero target column (s_c = 0:
    0/0 behind the ReLU's select, which must drop it as torch does -- tests/test_recon_device_cpu.py checks torch's float64 gradient
    is finite there); a step from counter 7 with non-zero moments.  Should the default path's own figure not be finite there, the
    float32 restatement's error is the yardstick."""
    b, f = 48, 17
    x1, t, w, wfc = R.make_case(b, f, 77)
    w[5] = -np.abs(w[5]) - 0.1
    for weights in ((1.0, 1.0), (0.8, 0.2)):
        want = R.step(x1, t, w, wfc, w_pos=weights[0], w_neg=weights[1])
        assert float(np.abs(want["grad.w"][5]).max()) == 0.0 and float(np.abs(want["grad.fc"][:, 5]).max()) == 0.0
        yard = _default_steps(x1, t, [0, b], w, wfc, wp=weights[0], wn=weights[1])
        got = _device_steps(x1, t, [0, b], w, wfc, wp=weights[0], wn=weights[1])
        assert np.all(got["grad.w"][5] == 0.0) and np.all(got["grad.fc"][:, 5] == 0.0)
        _judge(f"dead channel w={weights}", got, yard, want, KEYS, capsys, masks=_first_step_masks(want, w, wfc))
    x1, t, w, wfc = R.make_case(b, f, 78)
    wfc[3] = -np.abs(wfc[3]) - 0.5
    t[:, 3] = 0.0
    for weights in ((1.0, 1.0), (0.8, 0.2)):
        want = R.step(x1, t, w, wfc, w_pos=weights[0], w_neg=weights[1])
        assert all(np.isfinite(v).all() for v in want.values()) and float(np.abs(want["grad.fc"][3]).max()) == 0.0
        yard32 = R.step(x1, t, w, wfc, w_pos=weights[0], w_neg=weights[1], dtype=torch.float32)
        yard = _default_steps(x1, t, [0, b], w, wfc, wp=weights[0], wn=weights[1])
        got = _device_steps(x1, t, [0, b], w, wfc, wp=weights[0], wn=weights[1])
        assert np.all(got["grad.fc"][3] == 0.0)
        _judge(f"dead column w={weights}", got, yard, want, KEYS, capsys, finite_yard=yard32, masks=_first_step_masks(want, w, wfc))
    x1, t, w, wfc = R.make_case(150, f, 79)
    state = R.make_state(w, wfc, 80)
    want = R.step(x1, t, w, wfc, state, (7, 7), 0.8, 0.2)
    yard = _default_steps(x1, t, [0, 150], w, wfc, state, (7, 7), 0.8, 0.2)
    got = _device_steps(x1, t, [0, 150], w, wfc, state, (7, 7), 0.8, 0.2)
    _judge("counter 7", got, yard, want, KEYS + ("m.w", "v.w", "m.fc", "v.fc"), capsys)
    assert got["c.w"][0] == 8 and got["c.fc"][0] == 8


@pytest.mark.parametrize("count", [0, 7])
def test_adam_is_the_projects_adam_bit_for_bit(count):
    """One device step that hands back the raw gradients; `ggad_adam_multi_f32` (through `FlatAdam.step`) applied with those
    gradients to copies of the initial parameters, moments and counters: equal bits."""
    b, f = 150, 17
    x1, t, w, wfc = R.make_case(b, f, 91 + count)
    state = R.make_state(w, wfc, 92) if count else None
    got = _device_steps(x1, t, [0, b], w, wfc, state, (count, count), 0.8, 0.2)
    W, FC, opt = _params(w, wfc, state, (count, count), R.WD)
    W.grad, FC.grad = torch.from_numpy(got["grad.w"]).to(DEV), torch.from_numpy(got["grad.fc"]).to(DEV)
    opt.step()
    ref = _collect(torch.zeros(1), W.grad, FC.grad, W, FC, opt)
    assert float(np.abs(got["grad.w"]).max()) > 1e-5 and not np.array_equal(got["w"], w)
    for k in ("w", "fc", "m.w", "v.w", "m.fc", "v.fc", "c.w", "c.fc"):
        assert np.array_equal(got[k].view(np.int32), ref[k].view(np.int32)), k
    assert got["c.w"][0] == count + 1


def _build(g, tag, modname, **kw):
    m = importlib.import_module(modname)
    adj = synth.csr_to_adj_lists(g["rowptr"], g["col"])
    feats = torch.nn.Embedding(int(g["n"]), int(g["f"]))
    feats.weight = torch.nn.Parameter(torch.from_numpy(g["feat"]), requires_grad=False)
    agg = m.GCNAggregator(feats, cuda=True)
    enc = m.GCNEncoder(feats, int(g["f"]), int(g["d"]), adj, agg, gcn=True, cuda=True, **kw)
    model = m.GCN(2, enc)
    with torch.no_grad():
        for k in (k for k in model.state_dict().keys() if "features" not in k):
            model.state_dict()[k].copy_(torch.from_numpy(g[f"{tag}.init.{k}"]))
    return adj, agg, enc, model


@pytest.mark.parametrize("tag,modname,weights", TAGS)
def test_recorded_trajectory_in_one_launch_and_the_scores(tag, modname, weights, capsys):
    """The fixture's five batches of 48 through ONE `steps` call on the plan of the real aggregator, against the trajectory recorded from
    the reference (the bounds of tests/test_baselines_gpu.py); five 1-step launches and a rerun give the same bits; both counters
    advance by 5; then `recon_scores` -- slices of 30 with a ragged tail -- through `ReconDevice.scores`."""
    g = load_golden("minibatch_baselines.npz")
    feat = torch.from_numpy(g["feat"])
    runs = []
    for launches in (5, 1, 5):
        adj, agg, enc, model = _build(g, tag, modname, recon_device=True)
        assert isinstance(enc.recon_device, ReconDevice) and model.recon_weights == weights
        opt = FlatAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.007)
        rd = enc.recon_device.bind(enc, opt)
        batches = [b.tolist() for b in g["batches"]]
        x1, bp = agg.aggregate(batches, adj, len(batches))
        x1 = x1.clone()
        target = feat[np.concatenate(batches)].to(DEV)
        losses = []
        for s0 in range(0, 5, launches):
            lo, hi = int(bp[s0]), int(bp[s0 + launches])
            losses.append(rd.steps(x1[lo:hi], target[lo:hi], np.asarray(bp[s0:s0 + launches + 1]) - lo, *weights).clone())
            if s0 == 0 and launches == 1:
                np.testing.assert_allclose(enc.weight.detach().cpu().numpy(), g[f"{tag}.step1.enc.weight"], atol=3e-6, rtol=0)
                np.testing.assert_allclose(enc.fc.weight.detach().cpu().numpy(), g[f"{tag}.step1.enc.fc.weight"], atol=3e-6, rtol=0)
        assert int(opt.state[enc.weight][2]) == 5 and int(opt.state[enc.fc.weight][2]) == 5
        assert model.weight.grad is None and model.weight not in opt.state
        runs.append((torch.cat(losses).cpu().numpy(), enc.weight.detach().cpu().numpy().copy(), enc.fc.weight.detach().cpu().numpy().copy(),
                     enc.weight.grad.cpu().numpy().copy(), enc.fc.weight.grad.cpu().numpy().copy()))
    np.testing.assert_allclose(runs[0][0], g[f"{tag}.losses"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(runs[0][1], g[f"{tag}.final.enc.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(runs[0][2], g[f"{tag}.final.enc.fc.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(model.weight.detach().cpu().numpy(), g[f"{tag}.init.weight"], atol=0, rtol=0)
    for other in runs[1:]:          # five 1-step launches, then a rerun of the 5-step launch
        for a, b in zip(runs[0], other):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # scores with the weights the device steps left (the last model built)
    nodes, bs = g["test_nodes"], int(g["test_bs"])
    sc = recon_scores(model, nodes, bs, feat).cpu().numpy()
    np.testing.assert_allclose(sc, g[f"{tag}.test_scores"], atol=2e-5, rtol=0)
    xs = [O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes[s:s + bs], False, dtype=np.float64).to_feats
          for s in range(0, len(nodes), bs)]
    want = {"scores": R.scores(np.concatenate(xs), g["feat"][nodes], runs[0][1], runs[0][2])}
    several = recon_scores(model, nodes, bs, feat, batches_per_launch=3).cpu().numpy()          # plans of three slices
    np.testing.assert_allclose(several, g[f"{tag}.test_scores"], atol=2e-5, rtol=0)
    rd, enc.recon_device = enc.recon_device, None
    yard = {"scores": recon_scores(model, nodes, bs, feat, batches_per_launch=3).cpu().numpy()}
    enc.recon_device = rd
    _judge(f"scores {tag}", {"scores": several}, yard, want, ("scores",), capsys)


def test_ragged_schedule(capsys):
    """Batches of 48, 1, 150 and 2 rows in one launch: the losses and the last step's gradients under the measured bound; the weights
    after the four steps within the 2e-5 the recorded five-step trajectory allows the final weights (early Adam steps follow the sign
    of the gradient, see `_first_step_masks`, so a measured bound on them would be a bound on luck)."""
    sizes = [48, 1, 150, 2]
    bp = np.concatenate([[0], np.cumsum(sizes)])
    x1, t, w, wfc = R.make_case(int(bp[-1]), 17, 555)
    losses, _, want = R.run_steps(x1, t, bp, w, wfc, 0.8, 0.2)
    want["losses"] = losses
    yard = _default_steps(x1, t, bp, w, wfc, wp=0.8, wn=0.2)
    got = _device_steps(x1, t, bp, w, wfc, wp=0.8, wn=0.2)
    _judge("ragged 48/1/150/2", got, yard, want, ("losses", "grad.w", "grad.fc"), capsys)
    np.testing.assert_allclose(got["w"], want["w"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(got["fc"], want["fc"], atol=2e-5, rtol=0)
    again = _device_steps(x1, t, bp, w, wfc, wp=0.8, wn=0.2, launches=1)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    assert got["c.w"][0] == 4 and got["c.fc"][0] == 4


def _handler_cfg(data, **kw):
    cfg = dict(data_name="dgraphfin", data_dir="./data/", train_ratio=0.4, test_ratio=0.67, save_dir="./pytorch_models/",
               model="GCN", multi_relation="GNN", emb_size=64, thres=0.4, rho=0.5, seed=72, optimizer="adam", lr=0.001,
               weight_decay=0.007, batch_size=150, num_epochs=2, valid_epochs=5, alpha=2, no_cuda=False, cuda_id="0", data=data)
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("which,pw", [("dominate", None), ("anomalydae", 0.5)])
def test_handler_with_the_switch_equals_the_oracle_loop_and_the_default_path(which, pw):
    """The setup of `test_handler_epochs_equal_the_oracle_loop` (tests/test_baselines_gpu.py) with `recon_device=True`."""
    mh = importlib.import_module(f"ggad_amd.model_handler_{which}")
    n, f = 30000, 17
    rowptr, col = synth.make_graph(n, 150000, 3, kind="powerlaw", max_degree=300)
    feat_raw = synth.make_features(n, f, 3)
    y = synth.make_labels(n, 0.02, 3).astype(np.int32)
    nb = 12
    start = random.getstate()
    torch.manual_seed(72)
    np.random.seed(72)
    h = mh.ModelHandler(_handler_cfg(((rowptr, col), feat_raw, y), num_batches=nb, recon_device=True))
    idx_train0 = list(h.dataset["idx_train"])
    state_after_split = random.getstate()
    h.train()
    state_after_train = random.getstate()
    assert isinstance(h.model.enc.recon_device, ReconDevice)
    torch.manual_seed(72)
    torch.nn.Embedding(n, f)
    w = torch.nn.init.xavier_uniform_(torch.empty(64, f)).requires_grad_(True)
    fc = torch.nn.Linear(64, f, bias=False).weight.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([w, fc], lr=0.001, weight_decay=0.007)
    feat = np.asarray(h.dataset["feat_data"], dtype=np.float32)
    random.setstate(state_after_split)
    idx = idx_train0
    for epoch in range(2):
        random.shuffle(idx)
        for b in range(nb):
            nodes = idx[b * 150:(b + 1) * 150]
            opt.zero_grad()
            loss, _ = O.baseline_loss(w, fc, rowptr, col, feat, nodes, feat[nodes], pw)
            loss.backward()
            opt.step()
            assert abs(loss.item() - h.epoch_losses[epoch][b]) < 2e-5, (epoch, b)
    got_w, got_fc = h.model.enc.weight.detach().cpu().numpy(), h.model.enc.fc.weight.detach().cpu().numpy()
    np.testing.assert_allclose(got_w, w.detach().numpy(), atol=3e-5, rtol=0)
    np.testing.assert_allclose(got_fc, fc.detach().numpy(), atol=3e-5, rtol=0)
    assert random.getstate() == state_after_train
    assert len(h.valid_history) == 1
    sc = recon_scores(h.model, h.dataset["idx_valid"][:1000], 150, torch.from_numpy(feat)).cpu().numpy()
    ref = O.baseline_scores(w.detach(), fc.detach(), rowptr, col, feat, h.dataset["idx_valid"][:1000], 150, feat)
    np.testing.assert_allclose(sc, ref, atol=3e-5, rtol=0)
    # the default path from the same seeds
    random.setstate(start)
    torch.manual_seed(72)
    np.random.seed(72)
    d = mh.ModelHandler(_handler_cfg(((rowptr, col), feat_raw, y), num_batches=nb))
    d.train()
    assert d.model.enc.recon_device is None and random.getstate() == state_after_train
    np.testing.assert_allclose(got_w, d.model.enc.weight.detach().cpu().numpy(), atol=3e-5, rtol=0)
    np.testing.assert_allclose(got_fc, d.model.enc.fc.weight.detach().cpu().numpy(), atol=3e-5, rtol=0)
    assert len(d.valid_history) == 1


def test_misuse_raises_before_any_launch():
    x1, t, w, wfc = R.make_case(48, 17, 3)
    for f, d in ((65, 64), (17, 32)):
        W, FC, opt = _params(np.zeros((d, f), np.float32), np.zeros((f, d), np.float32), None, (0, 0), R.WD)
        with pytest.raises(ValueError):
            ReconDevice().bind(_stub_encoder(W, FC), opt)
        assert opt.state == {}
    f = 64
    big = _max_rows(f) + 1
    x1, t, w, wfc = R.make_case(big, f, 4)
    W, FC, opt = _params(w, wfc, None, (0, 0), R.WD)
    rd = ReconDevice().bind(_stub_encoder(W, FC), opt)
    xd, td = torch.from_numpy(x1).to(DEV), torch.from_numpy(t).to(DEV)
    bad = [lambda: rd.steps(xd, td, [0, big]), lambda: rd.steps(xd, td, [0, 10, 10, big - 1]), lambda: rd.steps(xd, td, [0, 10]),
           lambda: rd.steps(xd.double(), td, [0, 10, big]), lambda: rd.steps(xd.cpu(), td, [0, 10, big]),
           lambda: rd.steps(xd[:, :17], td[:, :17], [0, 10, big]), lambda: rd.steps(xd.t().contiguous().t(), td, [0, 10, big]),
           lambda: rd.steps(xd[:20], td[:20], [0, 20], losses=torch.empty(2, device=DEV)), lambda: rd.scores(xd, td[:5]),
           lambda: ReconDevice().bind(_stub_encoder(W, FC)).steps(xd[:20], td[:20], [0, 20])]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
        torch.cuda.synchronize()
        assert np.array_equal(W.detach().cpu().numpy(), w) and np.array_equal(FC.detach().cpu().numpy(), wfc), i
        assert int(opt.state[W][2]) == 0 and not bool(opt.state[W][0].any())
    assert load().ggad_recon_mb_steps_f32(*[xd.data_ptr()] * 3, 1, big, big, f, 64, *[xd.data_ptr()] * 8, 1e-3, 0.007, 1.0, 1.0,
                                          *[xd.data_ptr()] * 3, None) == -1
    assert np.array_equal(W.detach().cpu().numpy(), w)
