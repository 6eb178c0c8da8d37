"""Keeping the best epoch on the device: `ggad_select_decide_f64` / `ggad_select_copy_f32` (csrc/select.hip), `BestKeeper`
(ggad_amd/select.py), `Model.score` and `run.py --select / --save / --score`.

Kernel level (against the numpy restatement tests/select_ref.py, everything compared bit for bit):
  1. the decision sequence of the CPU test, one epoch at a time, for both metrics; without a curve; with a curve shorter than the run;
  2. the copy at 1, 3, 63, 64, 65, 257 and 300*300+1 elements, source and destination independently 0, 4, 8 and 12 bytes into their
     allocations, the destination carved out of the NaN blocks of tests/dirty.py: taken -> equal bits and intact guards, not taken ->
     the previous bits;
  3. 16 tensors in one call, 17 in two calls after one decide;
  4. n = 0, n = 17 and which = 2 return GGAD_E_INVALID and change no byte;
  5. metric + decide + copy captured as one hipGraph and replayed over a changing score buffer for 6 epochs = the eager sequence.

End to end, on a planted-anomaly graph of 1,200 nodes written as a `.mat` file (so that a child process loads the same graph),
embedding_dim 64, 6 epochs, noise N(0.02, 0.01):
  6. `Model.score` = the evaluation forward's scores, and it leaves the CPU generator where it was;
  7. `--select` does not perturb the training: losses, last weights and the generator state equal a run without it;
  8. captured = `--no_graph`;
  9. the curve and the kept weights against plain runs of 1..6 epochs and sklearn (1e-12: the bound of
     tests/test_eval_cache_gpu.py::test_rank_report_against_exact_counts_and_sklearn), for `--select auroc` and `--select ap`;
 10. `--save`, then `--score --top_k 50 --top_k_out` in a fresh child process; a checkpoint with another n_in is refused."""
import contextlib
import ctypes
import importlib.util
import io
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dirty
import select_ref as R
import topk_ref as TK
from conftest import ROOT
from ggad_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _lib():
    from ggad_amd import _lib as L
    return L


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _decide(out8, which, state4, curve, cap):
    L = _lib()
    L.call("ggad_select_decide_f64", L.ptr(out8), which, L.ptr(state4), L.ptr(curve), cap)


def _out8(triple):
    a, p, st = triple
    return torch.tensor([a, p, 5.0, 6.0, 7.0, 8.0, 12.0, st], dtype=torch.float64, device=DEV)


def _state():
    return torch.tensor(R.initial_state(), dtype=torch.float64, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. decide
@pytest.mark.parametrize("which", [0, 1])
def test_decision_sequence_equals_the_restatement(which):
    n = len(R.SEQUENCE)
    state4, curve = _state(), torch.full((n, 3), NAN, dtype=torch.float64, device=DEV)
    ref_state, ref_curve = R.initial_state(), np.full((n, 3), NAN)
    for e, triple in enumerate(R.SEQUENCE):
        _decide(_out8(triple), which, state4, curve, n)
        taken = R.decide(ref_state, triple, which, ref_curve)
        assert taken == R.TAKEN[which][e]
        assert R.same(state4.cpu().numpy(), ref_state), (which, e, state4.cpu().tolist(), ref_state.tolist())
    assert R.same(curve.cpu().numpy(), ref_curve)
    full = R.run(R.SEQUENCE, which)
    assert R.same(state4.cpu().numpy(), full["state4"]) and R.same(curve.cpu().numpy(), full["curve"])


def test_decision_without_a_curve_and_with_a_short_one():
    n = len(R.SEQUENCE)
    state4 = _state()
    for triple in R.SEQUENCE:
        _decide(_out8(triple), 0, state4, None, 0)
    assert R.same(state4.cpu().numpy(), R.run(R.SEQUENCE, 0)["state4"])
    # a curve of 4 epochs inside a NaN block: epochs 4.. are decided but not recorded, and nothing behind the curve is written
    block = torch.full((dirty.GUARD + 12 + dirty.GUARD,), NAN, dtype=torch.float64, device=DEV)
    before = block.clone()
    curve = block[dirty.GUARD:dirty.GUARD + 12].view(4, 3)
    state4 = _state()
    for triple in R.SEQUENCE:
        _decide(_out8(triple), 1, state4, curve, 4)
    ref = R.run(R.SEQUENCE, 1, curve_cap=4)
    assert R.same(state4.cpu().numpy(), ref["state4"]) and R.same(curve.cpu().numpy(), ref["curve"])
    assert n > 4 and torch.equal(block[:dirty.GUARD].view(torch.int64), before[:dirty.GUARD].view(torch.int64))
    assert torch.equal(block[dirty.GUARD + 12:].view(torch.int64), before[dirty.GUARD + 12:].view(torch.int64))


# ------------------------------------------------------------------------------------------------ 2. copy: sizes and alignment
SIZES = [1, 3, 63, 64, 65, 257, 300 * 300 + 1]
OFFSETS = [(so, do) for so in range(4) for do in range(4)]          # floats into the allocation: 0, 4, 8, 12 bytes, both sides


def _carve(n, off):
    """A float32 view of n elements starting `off` floats behind the front guard of a NaN block: (block, view)."""
    block = torch.full((dirty.GUARD + off + n + dirty.GUARD,), NAN, dtype=torch.float32, device=DEV)
    assert block.data_ptr() % 16 == 0
    return block, block[dirty.GUARD + off:dirty.GUARD + off + n]


def _outside_intact(block, n, off):
    bits = _bits(block)
    bits[dirty.GUARD + off:dirty.GUARD + off + n] = dirty.NAN_BITS
    bad = np.flatnonzero(bits != dirty.NAN_BITS)
    assert bad.size == 0, f"{bad.size} words outside the tensor were written, first at float {int(bad[0]) - dirty.GUARD - off}"


def _random_bits(n, rng):
    """n float32 of arbitrary bit patterns (NaNs, infinities and denormals among them)."""
    return torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)).to(DEV).view(torch.float32)


def _copy(src, dst, state4):
    from ggad_amd.select import copy_if_taken
    copy_if_taken(src, dst, state4)


@pytest.mark.parametrize("n", SIZES)
def test_copy_at_every_alignment(n):
    rng = np.random.default_rng(n)
    assert len(OFFSETS) == _lib().load().ggad_select_max_tensors()       # the 16 (source, destination) offsets go in ONE call
    srcs, dsts = [], []
    for so, do in OFFSETS:
        sb, s = _carve(n, so)
        s.copy_(_random_bits(n, rng))
        db, d = _carve(n, do)
        assert s.data_ptr() % 16 == 4 * so and d.data_ptr() % 16 == 4 * do
        srcs.append((sb, s))
        dsts.append((db, d, do))
    S, D = [s for _, s in srcs], [d for _, d, _ in dsts]
    state4 = _state()
    # epoch 0 is not taken (one class only): every destination keeps its NaN bits
    _decide(_out8((NAN, 0.0, 1.0)), 0, state4, None, 0)
    _copy(S, D, state4)
    assert state4.cpu().tolist()[3] == 0.0
    for db, d, do in dsts:
        assert (_bits(db) == dirty.NAN_BITS).all()
    # epoch 1 is taken: equal bits, and nothing outside the tensor is touched
    _decide(_out8((0.75, 0.5, 0.0)), 0, state4, None, 0)
    _copy(S, D, state4)
    assert state4.cpu().tolist() == [0.75, 1.0, 2.0, 1.0]
    first = [_bits(s) for s in S]
    for (db, d, do), want in zip(dsts, first):
        assert np.array_equal(_bits(d), want), (n, do)
        _outside_intact(db, n, do)
    # epoch 2 is not taken (a lower value), the sources have moved on: the destinations keep epoch 1's bits exactly
    for s in S:
        s.copy_(_random_bits(n, rng))
    _decide(_out8((0.5, 0.5, 0.0)), 0, state4, None, 0)
    _copy(S, D, state4)
    assert state4.cpu().tolist() == [0.75, 1.0, 3.0, 0.0]
    for (db, d, do), want, s in zip(dsts, first, S):
        assert np.array_equal(_bits(d), want) and (n < 3 or not np.array_equal(_bits(s), want))
        _outside_intact(db, n, do)
    for sb, s in srcs:                                                     # (the sources are only read)
        _outside_intact(sb, n, (s.data_ptr() - sb.data_ptr()) // 4 - dirty.GUARD)


# ------------------------------------------------------------------------------------------------ 3. tensor counts
@pytest.mark.parametrize("count", [16, 17])
def test_tensor_count_boundaries(count):
    L = _lib()
    cap = int(L.load().ggad_select_max_tensors())
    assert cap == 16
    rng = np.random.default_rng(count)
    sizes = [int(v) for v in rng.integers(1, 700, count)]
    sizes[3] = 0                                                           # an empty tensor among them
    src = [_random_bits(n, rng) for n in sizes]
    pairs = [_carve(n, i % 4) for i, n in enumerate(sizes)]
    dst = [d for _, d in pairs]
    calls = []
    real = L.call

    def counting(name, *a):
        calls.append((name, a[0]))
        return real(name, *a)
    state4 = _state()
    _decide(_out8((0.5, 0.5, 0.0)), 1, state4, None, 0)                   # ONE decide: taken
    L.call = counting
    try:
        _copy(src, dst, state4)
    finally:
        L.call = real
    assert calls == ([("ggad_select_copy_f32", 16)] if count == 16 else [("ggad_select_copy_f32", 16), ("ggad_select_copy_f32", 1)])
    want = [_bits(s) for s in src]
    for i, ((b, d), w) in enumerate(zip(pairs, want)):
        assert np.array_equal(_bits(d), w), i
        _outside_intact(b, sizes[i], i % 4)
    for s in src:
        s.copy_(_random_bits(s.numel(), rng))
    _decide(_out8((0.5, 0.5, 0.0)), 1, state4, None, 0)                   # ONE decide: a tie, not taken -- both groups leave dst alone
    _copy(src, dst, state4)
    assert state4.cpu().tolist() == [0.5, 0.0, 2.0, 0.0]
    for i, ((b, d), w) in enumerate(zip(pairs, want)):
        assert np.array_equal(_bits(d), w), i


# ------------------------------------------------------------------------------------------------ 4. argument checks
def test_invalid_arguments_change_no_byte():
    L = _lib()
    lib = L.load()
    st = L.current_stream()
    src = [_random_bits(40, np.random.default_rng(i)) for i in range(17)]
    pairs = [_carve(40, 0) for _ in range(17)]
    state4 = torch.tensor([0.5, 0.0, 1.0, 1.0], dtype=torch.float64, device=DEV)       # (taken: a launch WOULD copy)
    curve = torch.full((4, 3), NAN, dtype=torch.float64, device=DEV)
    arr = ctypes.c_void_p * 17
    s_arr, d_arr = arr(*[t.data_ptr() for t in src]), arr(*[d.data_ptr() for _, d in pairs])
    num = (ctypes.c_int64 * 17)(*([40] * 17))
    for n in (0, 17):
        assert lib.ggad_select_copy_f32(n, s_arr, d_arr, num, L.ptr(state4), st) == L.GGAD_E_INVALID
    out8 = _out8((0.9, 0.9, 0.0))
    for which in (2, -1):
        assert lib.ggad_select_decide_f64(L.ptr(out8), which, L.ptr(state4), L.ptr(curve), 4, st) == L.GGAD_E_INVALID
    torch.cuda.synchronize()
    for b, _ in pairs:
        assert (_bits(b) == dirty.NAN_BITS).all()
    assert state4.cpu().tolist() == [0.5, 0.0, 1.0, 1.0] and bool(torch.isnan(curve).all())


# ------------------------------------------------------------------------------------------------ 5. capture
def test_captured_metric_decide_copy_equals_eager():
    from ggad_amd.select import BestKeeper
    rng = np.random.default_rng(11)
    n_all, n_val, epochs = 900, 300, 6
    rows = rng.choice(n_all, n_val, replace=False)
    y = (rng.random(n_val) < 0.2).astype(np.uint8)
    y_all = np.zeros(n_all, dtype=np.float32)
    y_all[rows] = y
    base = rng.normal(0.0, 1.0, n_all).astype(np.float32)
    # the separation of the classes by epoch: up, down, up, the SAME scores again (a tie: not taken), down
    sep = [0.0, 0.6, 0.2, 1.2, 1.2, 0.1]
    scores = [torch.from_numpy(base + np.float32(a) * y_all).to(DEV) for a in sep]
    shapes = [(5,), (64, 3), (1,), (33, 7)] + [(i + 2,) for i in range(13)]                  # 17 tensors: two copy groups
    weights = [[_random_bits(int(np.prod(s)), rng).view(*s) for s in shapes] for _ in range(epochs)]

    def keeper_on(params):
        return BestKeeper(params, epochs, "auroc", labels_u8=y, rows=rows)

    # eager: the parameters are rebound every epoch
    eager_params = [w.clone() for w in weights[0]]
    eager = keeper_on(eager_params)
    for e in range(epochs):
        for p, w in zip(eager_params, weights[e]):
            p.copy_(w)
        eager.step(scores[e])
    taken_curve = eager.curve()
    assert eager.best_epoch == 3 and taken_curve[3, 0] == taken_curve[4, 0] and np.all(taken_curve[:, 2] == 0.0)
    assert taken_curve[1, 0] > taken_curve[0, 0] and taken_curve[2, 0] < taken_curve[1, 0] and taken_curve[3, 0] > taken_curve[1, 0]
    for s, w in zip(eager.snapshot, weights[3]):
        assert np.array_equal(_bits(s), _bits(w))
    # captured: one graph of gather + metric + decide + two copies over static buffers, refilled before every replay
    params = [w.clone() for w in weights[0]]
    static_scores = scores[0].clone()
    cap = keeper_on(params)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.step(static_scores)
    torch.cuda.synchronize()
    assert R.same(cap.state4.cpu().numpy(), R.initial_state())              # (the capture itself executed nothing)
    for e in range(epochs):
        static_scores.copy_(scores[e])
        for p, w in zip(params, weights[e]):
            p.copy_(w)
        graph.replay()
    torch.cuda.synchronize()
    assert R.same(cap.state4.cpu().numpy(), eager.state4.cpu().numpy())
    assert R.same(cap.curve(), taken_curve) and cap.best_epoch == eager.best_epoch and cap.best_value == eager.best_value
    for a, b in zip(cap.snapshot, eager.snapshot):
        assert np.array_equal(_bits(a), _bits(b))
    # and the restatement on the curve the kernels measured
    ref = R.run([tuple(r) for r in taken_curve], 0)
    assert R.same(ref["state4"], cap.state4.cpu().numpy()) and ref["taken"] == [True, True, False, True, False, False]


def test_best_keeper_refuses_more_positives_than_the_metric_kernel_sorts():
    from ggad_amd.select import BestKeeper
    cap = int(_lib().load().ggad_rank_metrics_max_pos())
    n = cap + 1
    with pytest.raises(ValueError, match=f"{n} positives.*ggad_rank_metrics_max_pos\\(\\) = {cap}"):
        BestKeeper([torch.zeros(4, device=DEV)], 2, "auroc", labels_u8=np.ones(n, dtype=np.uint8), rows=np.arange(n))
    k = BestKeeper([torch.zeros(4, device=DEV)], 2, "ap", labels_u8=np.ones(8, dtype=np.uint8), rows=np.arange(8))
    with pytest.raises(RuntimeError, match="no epoch was taken"):
        k.load_into()


# ------------------------------------------------------------------------------------------------ end to end
N, F, H, EPOCHS = 1200, 24, 64, 6
SEED = 0                     # seed 0 gives the validation list 3+ positives and 3+ negatives (asserted in `world`)
DATASET = "planted"          # not one of run.py's names: 1e-3 / 100 epochs by default, raw features, noise from the arguments below


def _run_py():
    spec = importlib.util.spec_from_file_location("ggad_run_script_select_gpu", os.path.join(ROOT, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


class World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The graph as ./dataset/planted.mat under a temporary directory, loaded the way `run.py` loads it, and every training run the
    checks below share -- each made once."""
    import scipy.io as sio
    import scipy.sparse as sp
    w = World()
    w.tmp = tmp_path_factory.mktemp("select")
    os.makedirs(w.tmp / "dataset")
    rowptr, col = synth.make_graph(N, 12 * N, SEED, kind="powerlaw", max_degree=N // 8)
    feat = synth.make_features(N, F, SEED)
    y = synth.make_labels(N, 0.08, SEED)
    rowptr, col, feat = synth.plant_anomalies(rowptr, col, feat, y, SEED, scale=0.25, rewire=0.5)
    sio.savemat(str(w.tmp / "dataset" / (DATASET + ".mat")),
                {"Network": synth.csr_to_scipy(rowptr, col, N), "Attributes": sp.csr_matrix(feat), "Label": y.reshape(1, -1)})
    w.run = run = _run_py()
    w.ckpt = str(w.tmp / "best.pt")
    w.cwd = os.getcwd()
    old_env = os.environ.get("GGAD_CAPTURE_BELOW_S")
    os.environ["GGAD_CAPTURE_BELOW_S"] = "10"            # (a busy host must not decide whether the epoch is captured)
    os.chdir(w.tmp)
    try:
        w.argv = ["--dataset", DATASET, "--seed", str(SEED), "--embedding_dim", str(H), "--num_epoch", str(EPOCHS), "--quiet"]
        args = run.parse(w.argv)
        random.seed(SEED), np.random.seed(SEED), torch.manual_seed(SEED)          # what init_process seeds before the loader runs
        w.dev = torch.device(DEV)
        torch.cuda.set_device(w.dev)
        with contextlib.redirect_stdout(io.StringIO()):
            w.g = g = run.load_graph(args)
        w.y = np.asarray(g.ano_label).reshape(-1)
        assert w.y.shape == (N,) and np.array_equal(w.y, y)
        yv = w.y[np.asarray(g.idx_val)]
        assert int((yv == 1).sum()) >= 3 and int((yv == 0).sum()) >= 3, (int((yv == 1).sum()), len(yv))
        w.full, w.feats, w.ft = run.prepare(args, g.adj, g.feat, w.dev)
        assert w.ft == F

        def train(select=None, num_epoch=EPOCHS, no_graph=False, save=None):
            from ggad_amd.model import Model
            a = run.parse(w.argv + (["--select", select] if select else []) + (["--no_graph"] if no_graph else [])
                          + (["--save", save] if save else []))
            a.num_epoch, a.mean, a.var = num_epoch, 0.02, 0.01
            torch.manual_seed(SEED)
            model = Model(F, H, "prelu", a.negsamp_ratio, a.readout).to(w.dev)
            hist, out = {}, io.StringIO()
            with contextlib.redirect_stdout(out):
                run.fit(a, w.dev, w.full, w.feats, model, g.normal_idx, g.abn_idx, g.idx_test, g.ano_label, history=hist, idx_val=g.idx_val)
            torch.cuda.synchronize()
            return dict(hist=hist, out=out.getvalue(), model=model, rng=torch.get_rng_state().clone(),
                        params=[p.detach().cpu().clone() for p in model.parameters()])
        w.train = train
        w.plain = train()
        w.auroc = train("auroc", save=w.ckpt)
        w.ap = train("ap")
        w.eager = train("auroc", no_graph=True)
        w.prefix = [train(num_epoch=e + 1) for e in range(EPOCHS - 1)] + [w.plain]
    finally:
        os.chdir(w.cwd)
        if old_env is None:
            os.environ.pop("GGAD_CAPTURE_BELOW_S", None)
        else:
            os.environ["GGAD_CAPTURE_BELOW_S"] = old_env
    return w


def _same_tensors(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_model_score_equals_the_evaluation_forward_and_draws_nothing(world):
    w = world
    model = w.plain["model"]
    args = w.run.parse(w.argv)
    args.mean, args.var = 0.02, 0.01
    model.eval()
    before = torch.get_rng_state().clone()
    s = model.score(w.feats, w.full)
    assert torch.equal(torch.get_rng_state(), before)
    with torch.no_grad():
        f_3 = model(w.feats, w.full, w.g.abn_idx, w.g.normal_idx, False, args)[2]
    assert not torch.equal(torch.get_rng_state(), before)                   # (the existing forward draws, quirk 5)
    assert s.shape == (N,) and s.dtype == torch.float32 and not s.requires_grad
    assert torch.equal(s, f_3[0, :, 0])
    model.train()
    assert torch.equal(model.score(w.feats, w.full), s)
    assert np.array_equal(_bits(s), w.plain["hist"]["final_logits"].view(np.int32))


def test_select_does_not_perturb_the_training(world):
    w = world
    for sel in (w.auroc, w.ap, w.eager):
        assert sel["hist"]["losses"] == w.plain["hist"]["losses"] and len(sel["hist"]["losses"]) == EPOCHS
        assert _same_tensors(sel["hist"]["last_params"], w.plain["params"])
        assert torch.equal(sel["rng"], w.plain["rng"])
        assert sel["hist"]["eval"] == w.plain["hist"]["eval"]
        assert np.array_equal(sel["hist"]["final_logits"].view(np.int32), w.plain["hist"]["final_logits"].view(np.int32))
    assert "[select]" not in w.plain["out"] and "val_curve" not in w.plain["hist"]
    # (the run without the flag prints what the run with it prints, less the [select] lines and the closing timing lines)
    strip = lambda out: [ln for ln in out.splitlines() if not ln.startswith(("[select]", "nodes/s", "median epoch", "weights of epoch"))]
    assert strip(w.auroc["out"]) == strip(w.plain["out"])


def test_captured_equals_eager(world):
    a, e = world.auroc["hist"], world.eager["hist"]
    assert a["captured"] and not e["captured"]
    assert R.same(a["val_curve"], e["val_curve"]) and a["val_curve"].shape == (EPOCHS, 3)
    assert a["best_epoch"] == e["best_epoch"] and a["best_value"] == e["best_value"]
    assert _same_tensors(world.auroc["params"], world.eager["params"])       # (the model ends with the best weights loaded)
    assert np.array_equal(a["best_scores"].view(np.int32), e["best_scores"].view(np.int32))


@pytest.mark.parametrize("which", ["auroc", "ap"])
def test_curve_and_kept_weights_against_plain_runs_and_sklearn(world, which):
    from sklearn.metrics import average_precision_score, roc_auc_score
    w = world
    sel = getattr(w, which)
    curve = sel["hist"]["val_curve"]
    rows = np.asarray(w.g.idx_val)
    yv = w.y[rows]
    assert curve.shape == (EPOCHS, 3) and np.all(curve[:, 2] == 0.0)
    assert R.same(curve, w.auroc["hist"]["val_curve"])                       # (what is measured does not depend on what is selected)
    for e in range(EPOCHS):
        pre = w.prefix[e]
        assert pre["hist"]["losses"] == w.plain["hist"]["losses"][:e + 1]     # the same trajectory prefix
        sv = pre["hist"]["final_logits"][rows].astype(np.float64)
        auc, ap = roc_auc_score(yv, sv), average_precision_score(yv, sv)
        print(f"[{which}] epoch {e}: val auroc {curve[e, 0]!r} - sklearn {curve[e, 0] - auc:.3g}, ap {curve[e, 1]!r} - sklearn {curve[e, 1] - ap:.3g}")
        assert abs(curve[e, 0] - auc) <= 1e-12 and abs(curve[e, 1] - ap) <= 1e-12
    col = {"auroc": 0, "ap": 1}[which]
    ref = R.run([tuple(r) for r in curve], col)
    best = int(ref["state4"][1])
    assert sel["hist"]["best_epoch"] == best and sel["hist"]["best_value"] == curve[best, col] == ref["state4"][0]
    assert best == int(np.flatnonzero(curve[:, col] == np.nanmax(curve[:, col]))[0])      # the EARLIEST epoch of the maximum
    assert _same_tensors(sel["params"], w.prefix[best]["params"])            # the kept snapshot = the weights after `best + 1` plain epochs
    assert np.array_equal(sel["hist"]["best_scores"].view(np.int32), w.prefix[best]["hist"]["final_logits"].view(np.int32))
    assert f"[select] best epoch {best:04d} by validation {which}" in sel["out"]
    assert f"[select] best epoch: Testing {DATASET} AUC:{sel['hist']['best_auc']:.4f}" in sel["out"]
    assert f"[select] best epoch: Testing AP: {sel['hist']['best_ap']}" in sel["out"]


CHILD = "import sys, numpy as np; root, out = sys.argv[1:3]; sys.path.insert(0, root); import run; np.save(out, run.main(sys.argv[3:]))"


def test_save_then_score_and_rank_in_a_fresh_process(world):
    w = world
    hist = w.auroc["hist"]
    ck = torch.load(w.ckpt, map_location="cpu", weights_only=True)
    assert ck["meta"] == {"dataset": DATASET, "n_in": F, "embedding_dim": H, "nodes": N, "seed": SEED, "epoch": hist["best_epoch"],
                          "select": "auroc", "value": hist["best_value"]}
    assert f"weights of epoch {hist['best_epoch']:04d} written to {w.ckpt}" in w.auroc["out"]
    names = [k for k, _ in w.auroc["model"].named_parameters()]
    assert list(ck["state_dict"].keys()) == list(w.auroc["model"].state_dict().keys()) and len(names) == 17
    assert _same_tensors([ck["state_dict"][k] for k in names], w.auroc["params"])
    out_npy, out_npz = str(w.tmp / "scores.npy"), str(w.tmp / "ranked.npz")
    argv = ["--dataset", DATASET, "--seed", str(SEED), "--embedding_dim", str(H), "--score", w.ckpt, "--top_k", "50", "--top_k_out", out_npz]
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out_npy] + argv, cwd=str(w.tmp), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    scores = np.load(out_npy)
    assert scores.dtype == np.float32 and np.array_equal(scores.view(np.int32), hist["best_scores"].view(np.int32))
    # the reference's two lines, unprefixed, with the training process's numbers; no training happened
    assert f"\nTesting {DATASET} AUC:{hist['best_auc']:.4f}\n" in r.stdout and f"\nTesting AP: {hist['best_ap']}\n" in r.stdout
    assert "Epoch:" not in r.stdout and "Total time" not in r.stdout and "[select]" not in r.stdout
    idx_test = np.asarray(w.g.idx_test, dtype=np.int64)
    y_test = w.y[idx_test].astype(np.uint8)
    ref = TK.reference(scores[idx_test], y_test, 50)
    z = np.load(out_npz)
    assert ref["m"] == 50 and np.array_equal(z["node"], idx_test[ref["pos"]])
    assert np.array_equal(z["score"].view(np.int32), ref["score"].view(np.int32)) and np.array_equal(z["label"], y_test[ref["pos"]])
    assert np.array_equal(z["cum_positives"], ref["cum_pos"]) and int(z["n_pos"]) == ref["n_pos"] and int(z["tied_left_out"]) == ref["tied_left_out"]
    hits = int(ref["cum_pos"][-1])
    m = re.search(r"precision@50 ([0-9.]+) recall@50 ([0-9.]+)", r.stdout)
    assert m and m.group(1) == f"{hits / 50:.4f}" and m.group(2) == f"{hits / ref['n_pos']:.4f}"


def test_a_checkpoint_of_another_feature_width_is_refused(world):
    w = world
    ck = torch.load(w.ckpt, map_location="cpu", weights_only=True)
    ck["meta"]["n_in"] = F + 3
    bad = str(w.tmp / "bad.pt")
    torch.save(ck, bad)
    argv = ["--dataset", DATASET, "--seed", str(SEED), "--embedding_dim", str(H), "--score", bad]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run.py")] + argv, cwd=str(w.tmp), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert f"n_in = {F + 3}, embedding_dim = {H}" in r.stderr and f"n_in = {F}, embedding_dim = {H}" in r.stderr
    assert "Testing" not in r.stdout
