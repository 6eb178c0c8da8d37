"""The mini-batch AEGIS step and sweep in fused HIP kernels (`ggad_amd/aegis_device.py`, `csrc/aegis_mb.hip`): every branch against
the float64 restatement (tests/aegis_mb_fp64.py), saturated heads, determinism, the trajectory of the default path's test, the
one-launch sweep, the `aegis_device` switch of `ModelHandler`, and the errors raised before any launch."""
import random
import types

import numpy as np
import pytest
import torch

import aegis_mb_fp64 as R
from ggad_amd import synth
from oracle import ggad_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd import graphsage_aegis as M
    from ggad_amd import sage_utils as SU
    from ggad_amd._lib import load
    from ggad_amd.aegis_device import AegisDevice
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import FeatureTable

DEV = "cuda:0"
MAX_ROWS = 256                                  # ggad_aegis_mb_max_rows(); asserted below
SIZES = (2, 3, 63, 64, 65, 150, MAX_ROWS)
WIDTHS = (1, 17, 64)
DB0, DW0 = "grad.enc.discriminator2.lins.0.bias", "grad.enc.discriminator2.lins.0.weight"


def _case(b, f):
    return R.make_inputs(b, f, 1000 * b + f), R.make_params(f, 7 * f + b)


def _stub_encoder(f, params):
    """What `AegisDevice` reads of a `GCNEncoder`: the widths, `weight`, `discriminator2` (the restated MLP with its batch norm)."""
    enc = types.SimpleNamespace(feat_dim=f, embed_dim=64)
    enc.weight = torch.nn.Parameter(torch.from_numpy(params[0].copy()).to(DEV))
    d2 = M.MLP(64, 64, 1, 2, 0.0, torch.sigmoid).to(DEV)
    with torch.no_grad():
        for t, p in zip((d2.lins[0].weight, d2.lins[0].bias, d2.norms[0].module.weight, d2.norms[0].module.bias, d2.lins[1].weight,
                         d2.lins[1].bias), params[1:]):
            t.copy_(torch.from_numpy(p.copy()))
    enc.discriminator2 = d2
    return enc


def _device_step(x_feat, x_noise, params, dev=None, poison=False):
    """One `AegisDevice.step` on a fresh stub encoder (running buffers 0 / 1): every quantity of R.KEYS as float64 numpy."""
    f, b = x_feat.shape[1], x_feat.shape[0]
    dev = AegisDevice() if dev is None else dev
    dev.enc = None
    enc = _stub_encoder(f, params)
    dev.bind(enc)
    if poison:
        dev.reserve(b, 1)
        for t in (dev.scratch, dev.inv_std, dev.stats, dev.p_all, dev.p_gen, dev.losses):
            t.fill_(float("nan"))
    l1, l2 = dev.step(torch.from_numpy(x_feat).to(DEV), torch.from_numpy(x_noise).to(DEV))
    bn = enc.discriminator2.norms[0].module
    assert int(bn.num_batches_tracked) == 2
    st = dev.stats[0].view(4, 64)
    got = {"p": dev.p_all[:2 * b], "p_gen": dev.p_gen[:b], "loss_dis": l1.reshape(1), "loss_g": l2.reshape(1), "mean": st[0],
           "var": st[1], "mean_gen": st[2], "var_gen": st[3], "running_mean": bn.running_mean, "running_var": bn.running_var}
    for k, p in zip(R.GRADS, dev.params()):
        got[k] = p.grad
    return {k: v.detach().cpu().numpy().copy() for k, v in got.items()}


@pytest.fixture(scope="module")
def yardsticks():
    """float64 and float32 restatements of every case, computed once, and the float32 residue of the lins.0.bias gradient -- which is
    mathematically zero, batch norm subtracts the mean -- as the largest max|d b0| / max|d W0| over all cases."""
    want, yard = {}, {}
    for b in SIZES:
        for f in WIDTHS:
            (xf, xn), params = _case(b, f)
            want[b, f] = R.evaluate(xf, xn, params, torch.float64)
            yard[b, f] = R.evaluate(xf, xn, params, torch.float32)
    residue = max(float(np.abs(y[DB0]).max()) / float(np.abs(y[DW0]).max()) for y in yard.values())
    return want, yard, residue


def test_the_library_takes_what_the_tests_assume():
    lib = load()
    assert lib.ggad_abi_version() == 11 and lib.ggad_aegis_mb_max_rows() == MAX_ROWS >= 256
    assert lib.ggad_aegis_mb_supported(1, 64, 2) and lib.ggad_aegis_mb_supported(64, 64, MAX_ROWS)
    for bad in ((0, 64, 2), (65, 64, 2), (17, 32, 2), (17, 64, 1), (17, 64, MAX_ROWS + 1)):
        assert not lib.ggad_aegis_mb_supported(*bad), bad
    # an unsupported shape is refused with nothing launched (GGAD_E_UNSUPPORTED = -4): the pointers are never read
    one = torch.zeros(64, device=DEV)
    args = [one.data_ptr()] * 3 + [1, 2, 2, 65, 64] + [one.data_ptr()] * 7 + [0] + [one.data_ptr()] * 6 + [None]
    assert lib.ggad_aegis_mb_fwd_f32(*args) == -4


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("b", SIZES)
def test_every_branch_against_float64(b, f, yardsticks, capsys):
    """B = 2, 3 (one row block, a ragged one), 63 / 64 / 65 (the last block of wave 15 empty, full, one past it), 150 (the reference's
    batch), 256 (every register row in use); F = 1, 17, 64.  Bound per quantity: max(4 x the float32 restatement's own error against
    float64, 1e-6 x the quantity's largest magnitude); for the lins.0.bias gradient, whose true value is zero, 4 x the largest
    float32 residue ratio over all cases x this case's max|d W0|."""
    want_all, yard_all, residue = yardsticks
    (xf, xn), params = _case(b, f)
    want, yard = want_all[b, f], yard_all[b, f]
    got = _device_step(xf, xn, params)
    failures = []
    with capsys.disabled():
        for key in R.KEYS:
            assert got[key].shape == want[key].shape and np.isfinite(got[key]).all(), key
            err = float(np.abs(got[key] - want[key]).max())
            err32 = float(np.abs(yard[key] - want[key]).max())
            if key == DB0:
                bound = 4.0 * residue * float(np.abs(want[DW0]).max())
            else:
                bound = max(4.0 * err32, 1e-6 * float(np.abs(want[key]).max()))
            print(f"\n[aegis_mb branches B={b} F={f}] {key}: device {err:.3e} float32 {err32:.3e} "
                  f"ratio {err / max(err32, 1e-30):.2f} bound {bound:.3e}", end="")
            if err > bound:
                failures.append((key, err, err32, bound))
        print()
    assert not failures, failures


@pytest.mark.parametrize("b", (3, 150))
def test_saturated_heads_and_a_dead_channel_stay_finite(b):
    """b1 = +-1000 saturates both heads: the clamped logs give the losses exactly, the gradient divisor max((1 - p) p, 1e-12)
    gives zeros, not NaN.  A zero row of lins.0.weight gives a channel of zero variance: everything stays finite."""
    (xf, xn), params = _case(b, 17)
    for b1, loss_g in ((1000.0, 100.0), (-1000.0, 0.0)):
        ps = [p.copy() for p in params]
        ps[6][:] = b1
        got = _device_step(xf, xn, ps)
        assert all(np.isfinite(v).all() for v in got.values())
        assert np.all(got["p"] == (1.0 if b1 > 0 else 0.0)) and np.all(got["p_gen"] == (1.0 if b1 > 0 else 0.0))
        assert got["loss_g"][0] == loss_g and got["loss_dis"][0] == 50.0
        for k in R.GRADS:
            assert np.all(got[k] == 0.0), k
    ps = [p.copy() for p in params]
    ps[1][5, :] = 0.0
    got = _device_step(xf, xn, ps)
    assert all(np.isfinite(v).all() for v in got.values())
    assert got["var"][5] < 1e-12 and got["var_gen"][5] < 1e-12                 # zero up to the rounding of the mean
    want = R.evaluate(xf, xn, ps, torch.float64)
    np.testing.assert_allclose(got["p"], want["p"], atol=3e-6, rtol=0)


def test_equal_inputs_give_equal_bits():
    """The same batch twice, from a fresh `AegisDevice`, with every buffer pre-filled with NaN, and as batch 1 of a three-batch
    launch against a launch of its own."""
    b, f = 150, 17
    (xf, xn), params = _case(b, f)
    dev = AegisDevice()
    first = _device_step(xf, xn, params, dev)
    (of, on), _ = _case(65, f)
    _device_step(of, on, params, dev)
    second = _device_step(xf, xn, params, dev)
    fresh = _device_step(xf, xn, params)
    poisoned = _device_step(xf, xn, params, AegisDevice(), poison=True)
    for key in R.KEYS:
        for name, other in (("second", second), ("fresh", fresh), ("poisoned", poisoned)):
            assert np.array_equal(first[key], other[key]), (key, name)
    # many-batch launch: batches of 65, 150 and 2 rows
    (tf, tn), _ = _case(2, f)
    enc = _stub_encoder(f, params)
    dev = AegisDevice(enc)
    cat_f, cat_n = (torch.from_numpy(np.concatenate(a)).to(DEV) for a in ((of, xf, tf), (on, xn, tn)))
    many = dev.forward_many(cat_f, cat_n, [0, 65, 215, 217])
    bn = enc.discriminator2.norms[0].module
    assert int(bn.num_batches_tracked) == 6
    alone = AegisDevice(_stub_encoder(f, params)).forward_many(torch.from_numpy(xf).to(DEV), torch.from_numpy(xn).to(DEV), [0, b])
    assert torch.equal(many["p_all"][130:430], alone["p_all"]) and torch.equal(many["p_gen"][65:215], alone["p_gen"])
    assert torch.equal(many["losses"][1], alone["losses"][0]) and torch.equal(many["stats"][1], alone["stats"][0])
    assert np.array_equal(alone["p_all"].cpu().numpy(), first["p"].astype(np.float32))
    assert np.array_equal(alone["losses"][0].cpu().numpy(), np.array([first["loss_dis"][0], first["loss_g"][0]], dtype=np.float32))
    scores = AegisDevice(_stub_encoder(f, params)).score_many(cat_f, cat_n, [0, 65, 215, 217])
    assert torch.equal(scores[65:215], alone["p_all"][:b]) and torch.equal(scores[:65], many["p_all"][:65])
    assert torch.equal(scores[215:], many["p_all"][430:432])


# ------------------------------------------------------------------------------------------------ the model
N_NODES, F_DIM = 6000, 17


@pytest.fixture(scope="module")
def graph6k():
    rowptr, col = synth.make_graph(N_NODES, 60000, 5, kind="powerlaw", max_degree=300)
    feat = O.normalize_rows(synth.make_features(N_NODES, F_DIM, 5)).astype(np.float32)
    return rowptr, col, feat


def _model(graph6k, device_path):
    rowptr, col, feat = graph6k
    torch.manual_seed(11)
    features = FeatureTable(torch.from_numpy(feat))
    agg = M.GCNAggregator(features, feat, cuda=True)
    enc = M.GCNEncoder(features, F_DIM, 64, DeviceGraph(rowptr, col, DEV), agg, gcn=True, cuda=True,
                       aegis_device=True if device_path else None)
    model = M.GCN(2, enc).to(DEV)
    features.to(DEV)
    return model, agg


def _buffers(model):
    bn = model.enc.discriminator2.norms[0].module
    return bn.running_mean.cpu().numpy().astype(np.float64), bn.running_var.cpu().numpy().astype(np.float64), int(bn.num_batches_tracked)


def _compare_buffers(dev_model, def_model):
    """Relative 1e-6 of the buffer's largest magnitude (a running mean has entries near zero); the count exactly."""
    (m1, v1, n1), (m0, v0, n0) = _buffers(dev_model), _buffers(def_model)
    assert n1 == n0 and n0 > 0
    assert float(np.abs(m1 - m0).max()) <= 1e-6 * float(np.abs(m0).max())
    assert float(np.abs(v1 - v0).max()) <= 1e-6 * float(np.abs(v0).max())


def test_trajectory_of_the_default_paths_test_on_the_device_path(graph6k, capsys):
    """The setup of `test_aegis_minibatch_model_against_the_oracle_restatement`: n = 6,000, four batches of 150, lr 0.005, weight
    decay 0.007 (> 0: with 0, lins.0.bias follows rounding noise in both paths).  Both paths run side by side against the oracle;
    a bound is the larger of that test's bound and 4 x the default path's own error, and which limb held is printed."""
    rowptr, col, feat = graph6k
    rng = np.random.default_rng(3)
    batches = [rng.choice(N_NODES, size=150, replace=False) for _ in range(4)]
    runs = {}
    for path in ("default", "device"):
        model, agg = _model(graph6k, path == "device")
        assert (model.enc.aegis_device is not None) == (path == "device")
        names = [k for k, p in model.named_parameters() if p.requires_grad]
        used = [k for k in names if k == "enc.weight" or k.startswith("enc.discriminator2")]
        P = {k: p.detach().cpu().clone().requires_grad_() for k, p in model.named_parameters() if p.requires_grad}
        noise = agg.noise.numpy()
        out = {}
        la, lg, lab = model(batches[0])
        assert la.shape == (300, 1) and lg.shape == (150, 1) and lab.shape == (300,)
        ra, rg, rlab = O.aegis_forward(P, rowptr, col, feat, noise, batches[0])
        assert np.array_equal(lab.cpu().numpy(), rlab.numpy())
        out["logits_all"] = (la[:, 0].detach().cpu().numpy(), ra.detach().numpy(), 3e-6, 0.0)
        out["logits_gen"] = (lg[:, 0].detach().cpu().numpy(), rg.detach().numpy(), 3e-6, 0.0)
        tp = model.to_prob(batches[0])
        assert tp.shape == (150, 1)
        out["to_prob"] = (tp[:, 0].detach().cpu().numpy(), ra.detach().numpy()[:150], 3e-6, 0.0)
        opt = FlatAdam([p for p in model.parameters() if p.requires_grad], lr=0.005, weight_decay=0.007)
        ref_opt = O.make_adam([P[k] for k in used], 0.005, 0.007)
        for b in range(4):
            opt.zero_grad()
            l1, l2 = model.loss(batches[b])
            if path == "default":
                (l1 + l2).backward()
            ref_opt.zero_grad()
            r1, r2 = O.aegis_loss(P, rowptr, col, feat, noise, batches[b])
            (r1 + r2).backward()
            out[f"losses.{b}"] = (np.array([l1.item(), l2.item()]), np.array([r1.item(), r2.item()]), 5e-6, 0.0)
            if b == 0:
                got = dict(model.named_parameters())
                for k in used:
                    out["grad." + k] = (got[k].grad.cpu().numpy().copy(), P[k].grad.numpy().copy(), 5e-6, 2e-4)
                for k in names:
                    if k not in used:
                        assert got[k].grad is None, k                          # generator / discriminator / fc / weight: unused
            opt.step()
            ref_opt.step()
        got = dict(model.named_parameters())
        for k in used:
            out["final." + k] = (got[k].detach().cpu().numpy().copy(), P[k].detach().numpy().copy(), 2e-5, 0.0)
        runs[path] = (out, model)
    failures = []
    with capsys.disabled():
        for key, (got, want, atol, rtol) in runs["device"][0].items():
            dgot, dwant, _, _ = runs["default"][0][key]
            base = atol + rtol * np.abs(want)
            own = 4.0 * float(np.abs(dgot - dwant).max())
            err = np.abs(got - want)
            limb = "the default test's bound" if own <= float(base.min()) else "4 x the default path's error"
            print(f"\n[aegis_mb trajectory] {key}: device {float(err.max()):.3e} default {own / 4.0:.3e} limb: {limb}", end="")
            if not np.all(err <= np.maximum(base, own)):
                failures.append((key, float(err.max()), own / 4.0))
        print()
    assert not failures, failures
    _compare_buffers(runs["device"][1], runs["default"][1])
    assert _buffers(runs["device"][1])[2] == 2 * 6                              # two forwards and four steps, two calls each


def test_sweep_in_one_launch_equals_the_default_path(graph6k, capsys):
    """362 ids in slices of 90: four full slices and a last one of 2 rows, one forward launch and one fold.  Bound: the logits' of
    the trajectory test, max(3e-6, 4 x the default path's own error against the oracle).  A last slice of 1 row raises, as
    `BatchNorm1d` does in the default path, and nothing is launched: the running buffers stay where they were."""
    rowptr, col, feat = graph6k
    ids = np.random.default_rng(8).choice(N_NODES, size=362, replace=False)
    dmodel, agg = _model(graph6k, True)
    model, _ = _model(graph6k, False)
    got = SU.aegis_scores(dmodel, ids, 90).cpu().numpy()
    ref = SU.aegis_scores(model, ids, 90).cpu().numpy()
    assert got.shape == ref.shape == (362,)
    P = {k: p.detach().cpu() for k, p in model.named_parameters()}
    noise = agg.noise.numpy()
    with capsys.disabled():
        for s in range(5):
            sl = slice(90 * s, min(90 * (s + 1), 362))
            want = O.aegis_forward(P, rowptr, col, feat, noise, ids[sl])[0].detach().numpy()[:sl.stop - sl.start]
            own = float(np.abs(ref[sl] - want).max())
            err = float(np.abs(got[sl] - ref[sl]).max())
            print(f"\n[aegis_mb sweep] slice {s} ({sl.stop - sl.start} rows): device - default {err:.3e}, default - oracle {own:.3e}", end="")
            assert err <= max(3e-6, 4.0 * own), s
        print()
    _compare_buffers(dmodel, model)
    assert _buffers(dmodel)[2] == 10
    before = _buffers(dmodel)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        SU.aegis_scores(dmodel, ids[:361], 90)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        SU.aegis_scores(model, ids[:361], 90)
    after = _buffers(dmodel)
    assert after[2] == before[2] and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])


def _run_handler(graph6k, tmp_path, perturb=False, **kw):
    from ggad_amd.model_handler_aegis import ModelHandler

    class Handler(ModelHandler):
        def build_model(self, dev):
            out = super().build_model(dev)
            if perturb:                                                         # every weight one part in 1e7 away: an ulp each
                with torch.no_grad():
                    for p in out[2].parameters():
                        p.copy_((p.double() * (1.0 + 1e-7)).float())
            return out
    rowptr, col, _ = graph6k
    lab = synth.make_labels(N_NODES, 0.05, 5)
    cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), synth.make_features(N_NODES, F_DIM, 5), lab), seed=72, model="GCN",
               multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=90, num_epochs=3, valid_epochs=2,
               num_batches=5, save_dir=str(tmp_path) + "/", test_ratio=0.67, device=0)
    cfg.update(kw)
    random.seed(72)
    np.random.seed(72)
    torch.manual_seed(72)
    h = Handler(cfg)
    assert h.train() is None
    return h, random.getstate()


def test_handler_switch_against_the_default_path(graph6k, tmp_path, capsys):
    """`aegis_device: true` on the configuration of the default path's handler test (3 epochs of 5 batches of 90, validation at
    epochs 0 and 2).  Yardstick: how far the default path's own losses move when every initial weight moves by one part in 1e7,
    measured here per epoch and per loss as the largest movement over the epoch's batches (the two trajectories part further with
    every step, so an epoch is judged against the movement of that epoch); the device path stays within 4 x that.  Epochs 1 and 2
    are one captured graph: they equal the `capture: false` run bit for bit.  `random` ends where the default path leaves it."""
    base, state0 = _run_handler(graph6k, tmp_path)
    moved, _ = _run_handler(graph6k, tmp_path, perturb=True)
    dev, state1 = _run_handler(graph6k, tmp_path, aegis_device=True)
    eager, state2 = _run_handler(graph6k, tmp_path, aegis_device=True, capture=False)
    assert dev.model.enc.aegis_device is not None and base.model.enc.aegis_device is None
    assert state1 == state0 and state2 == state0
    failures = []
    with capsys.disabled():
        for e in range(3):
            assert dev.epoch_losses[e].shape == (5, 2) and np.isfinite(dev.epoch_losses[e]).all()
            for c, name in enumerate(("loss_dis", "loss_g")):
                move = float(np.abs(moved.epoch_losses[e][:, c] - base.epoch_losses[e][:, c]).max())
                err = float(np.abs(dev.epoch_losses[e][:, c] - base.epoch_losses[e][:, c]).max())
                print(f"\n[aegis_mb handler] epoch {e} {name}: device - default {err:.3e}, default's own movement {move:.3e} "
                      f"ratio {err / max(move, 1e-30):.2f}", end="")
                if err > 4.0 * move:
                    failures.append((e, name, err, move))
        print()
    assert not failures, failures
    assert len(dev.valid_history) == len(base.valid_history) == 2 and all(0.0 <= v[1] <= 1.0 for v in dev.valid_history)
    for e in range(3):
        assert np.array_equal(dev.epoch_losses[e], eager.epoch_losses[e]), e
    for (k, p), (_, q) in zip(dev.model.state_dict().items(), eager.model.state_dict().items()):
        assert torch.equal(p, q), k
    assert _buffers(dev.model)[2] == _buffers(base.model)[2]


def test_errors_raise_before_any_launch(graph6k):
    rowptr, col, feat = graph6k
    wide = synth.make_features(300, 65, 1)
    features = FeatureTable(torch.from_numpy(wide))
    g300 = DeviceGraph(*synth.make_graph(300, 2000, 1, kind="powerlaw", max_degree=40), DEV)
    with pytest.raises(ValueError, match="feat_dim <= 64"):
        M.GCNEncoder(features, 65, 64, g300, M.GCNAggregator(features, wide, cuda=True), gcn=True, cuda=True, aegis_device=True)
    f17 = FeatureTable(torch.from_numpy(feat))
    with pytest.raises(ValueError, match="emb_size must be 64"):
        M.GCNEncoder(f17, F_DIM, 32, DeviceGraph(rowptr, col, DEV), M.GCNAggregator(f17, feat, cuda=True), gcn=True, cuda=True,
                     aegis_device=True)
    with pytest.raises(ValueError, match="emb_size 64"):
        AegisDevice(types.SimpleNamespace(feat_dim=17, embed_dim=32))
    with pytest.raises(ValueError, match="True or an AegisDevice"):
        M.GCNEncoder(f17, F_DIM, 64, DeviceGraph(rowptr, col, DEV), M.GCNAggregator(f17, feat, cuda=True), gcn=True, cuda=True,
                     aegis_device="yes")
    params = R.make_params(17, 1)
    enc = _stub_encoder(17, params)
    dev = AegisDevice(enc)
    bn = enc.discriminator2.norms[0].module

    def x(b, f=17, where=DEV):
        return torch.ones(b, f, device=where)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        dev.step(x(1), x(1))
    with pytest.raises(ValueError, match=f"at most {MAX_ROWS}"):
        dev.step(x(MAX_ROWS + 1), x(MAX_ROWS + 1))
    with pytest.raises(ValueError, match=f"at most {MAX_ROWS}"):
        dev.score_many(x(MAX_ROWS + 3), x(MAX_ROWS + 3), [0, 2, MAX_ROWS + 3])
    with pytest.raises(ValueError, match="on cuda"):
        dev.step(x(4, where="cpu"), x(4))
    with pytest.raises(ValueError, match="17 columns"):
        dev.discriminate(x(4, 16), x(4, 16))
    with pytest.raises(ValueError, match="contiguous"):
        dev.step(x(8)[::2], x(4))
    with pytest.raises(ValueError, match="same number of rows"):
        dev.step(x(4), x(5))
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == 0 and all(p.grad is None for p in dev.params())
