"""GPU tests of the device-resident generator (csrc/rng.hip through `ggad_amd.rng.DeviceMT`): the kernel against torch's CPU stream
(state exactly, values against the float64 formula within twice torch's own deviation from it), a captured launch that draws fresh
values on every replay, the refusals, and training with the noise drawn on the device: `run.fit` on both long fixtures, the planted
GAAN and AEGIS runs, and the scripts' captured epoch against their eager one."""
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mt_randn_ref as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 5
STARTS = {"fresh": 0, "mid_block": 100}          # a prior torch.randn(100) leaves the position at 116 of 624
SIZES = (16, 17, 31, 32, 300, 623, 624, 625, 71400, 71401, 10984 * 16, 46564 * 16, 844 * 300, 89 * 300)


@pytest.fixture(autouse=True)
def _keep_host_stream():
    st = torch.get_rng_state()
    yield
    torch.set_rng_state(st)


def _host_state(prior, seed=SEED):
    torch.manual_seed(seed)
    if prior:
        torch.randn(prior)
    return torch.get_rng_state()


def _rel(values, v64, r64):
    """max |values - v64| / r over the draws with r > 0 (r = 0 gives the value 0 exactly in every evaluation)."""
    d = np.abs(np.asarray(values, dtype=np.float64) - v64)
    return float(np.max(np.divide(d, r64, out=np.zeros_like(d), where=r64 > 0)))


_TORCH_DEV = {}


def _torch_deviation(start):
    """torch's own deviation from the float64 formula on the same uniforms, divided by r: the largest over every size of this file
    drawn from this start (1.6 M values).  It is a property of torch's vectorised log / sin / cos and of the float32 rounding of
    t = 2 pi u2, so it is taken over all of those draws and not over the 16 values of the smallest case."""
    if start not in _TORCH_DEV:
        from ggad_amd import rng
        worst = 0.0
        for n in SIZES:
            st = _host_state(STARTS[start])
            words, pos = rng.parse_rng_state(st)
            want = torch.randn(n).numpy()
            u, _, _ = R.draw_uniforms(words, pos, n)
            v64, r64 = R.box_muller(u, n, np.float64)
            worst = max(worst, _rel(want, v64, r64))
        _TORCH_DEV[start] = worst
    return _TORCH_DEV[start]


# ------------------------------------------------------------------------------------------------ the kernel against the stream
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("start", list(STARTS))
def test_kernel_against_the_stream(start, n, capsys):
    """State and position after the call: exactly the restatement's.  Values: against the float64 formula on the same u, at most twice
    torch's own deviation from it, both divided by r (the device's logf / sinf / cosf round differently from the host's vector routines:
    the factor 2 is that margin).  scale / shift 0.01 / 0.02: bit-equal to fl(fl(x * 0.01) + 0.02) of the kernel's own plain values x
    (product and sum rounded separately; a fused multiply-add fails this), and equal to `restated * 0.01 + 0.02` in float32 within the
    same bound times 0.01 -- plus one float32 step of the result, which that comparison cannot do without: two normals that differ
    by less than the bound round to neighbouring float32 values of 0.02 + 0.01 x whenever the exact sums straddle a rounding point
    (step 1.9e-9 at 0.02; the bound times 0.01 is 5.7e-9 r and falls below it for r < 0.33).  The number of values beyond the bound
    WITHOUT that step is printed.  Two launches from the same uploaded state are bit-identical."""
    from ggad_amd import rng
    st = _host_state(STARTS[start])
    words, pos = rng.parse_rng_state(st)
    u, words2, pos2 = R.draw_uniforms(words, pos, n)
    v64, r64 = R.box_muller(u, n, np.float64)
    v32, _ = R.box_muller(u, n, np.float32)
    torch_dev = _torch_deviation(start)
    bound = 2.0 * torch_dev

    mt = rng.DeviceMT(DEV, words, pos, st)
    buf = torch.full((n,), float("nan"), device=DEV)
    mt.randn_(buf)
    got_words, got_pos = mt.state_host()
    assert got_pos == pos2 and np.array_equal(got_words, words2)
    got = buf.cpu().numpy()
    assert np.isfinite(got).all()
    kern_dev = _rel(got, v64, r64)
    with capsys.disabled():
        print(f"\n[device randn] {start} n={n}: kernel deviation / r {kern_dev:.3e}, torch's {torch_dev:.3e}, bound {bound:.3e}; "
              f"max |kernel - restated| {np.abs(got.astype(np.float64) - v32).max():.3e}")
    assert kern_dev <= bound, (start, n, kern_dev, torch_dev)

    mt2 = rng.DeviceMT(DEV, words, pos, st)
    buf2 = torch.full((n,), float("nan"), device=DEV)
    mt2.randn_(buf2)
    assert torch.equal(buf, buf2) and np.array_equal(mt2.state_host()[0], words2)

    mt3 = rng.DeviceMT(DEV, words, pos, st)
    buf3 = torch.full((n,), float("nan"), device=DEV)
    mt3.randn_(buf3, 0.01, 0.02)
    assert mt3.state_host()[1] == pos2 and np.array_equal(mt3.state_host()[0], words2)
    s, b = np.float32(0.01), np.float32(0.02)
    got3 = buf3.cpu().numpy()
    assert np.array_equal(got3, (got * s).astype(np.float32) + b)
    want3 = (v32 * s).astype(np.float32) + b
    d3 = np.abs(got3.astype(np.float64) - want3.astype(np.float64))
    beyond = int((d3 > bound * 0.01 * r64).sum())
    with capsys.disabled():
        print(f"[device randn] {start} n={n}: scaled, max |kernel - restated| {d3.max():.3e}; {beyond} of {n} beyond bound x 0.01 x r "
              "before the result's own float32 step is allowed")
    assert np.all(d3 <= bound * 0.01 * r64 + np.spacing(np.abs(want3)).astype(np.float64))


# ------------------------------------------------------------------------------------------------ capture
def test_replay_draws_fresh_values_and_the_host_continues():
    """One captured launch, replayed three times: three consecutive draws of the stream (each within the kernel test's bound of the
    float64 formula on ITS uniforms), the state after them exact, and the host generator continues bit for bit after `to_host`."""
    from ggad_amd import rng
    n = 89 * 300
    st = _host_state(0)
    words, pos = rng.parse_rng_state(st)
    want = []
    for _ in range(3):
        u, words, pos = R.draw_uniforms(words, pos, n)
        want.append(R.box_muller(u, n, np.float64))
    for _ in range(3):
        torch.randn(n)
    tail = torch.randn(40)
    torch.set_rng_state(st)

    mt = rng.DeviceMT.from_host(DEV)
    buf = torch.zeros(n, device=DEV)
    mt.reserve(n)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mt.randn_(buf)
    got = []
    for _ in range(3):
        graph.replay()
        got.append(buf.cpu().numpy().copy())
    torch.cuda.synchronize()
    bound = 2.0 * _torch_deviation("fresh")
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    for g, (v64, r64) in zip(got, want):
        assert _rel(g, v64, r64) <= bound
    assert mt.state_host()[1] == pos and np.array_equal(mt.state_host()[0], words)
    mt.to_host()
    assert torch.equal(torch.randn(40), tail)


def test_a_draw_that_would_allocate_inside_a_capture_is_refused(monkeypatch):
    """`randn_` under capture allocates nothing: without scratch it raises instead (no capture is started here)."""
    from ggad_amd import rng
    mt = rng.DeviceMT.from_host(DEV)
    buf = torch.zeros(64, device=DEV)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="reserve"):
        mt.randn_(buf)
    monkeypatch.undo()
    mt.randn_(buf)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    mt.reserve(32)                                                     # (enough scratch: no complaint)


def test_to_host_without_a_draw_leaves_the_host_state_as_it_was():
    from ggad_amd import rng
    for prior in (0, 100):
        st = _host_state(prior)
        rng.DeviceMT.from_host(DEV).to_host()
        assert torch.equal(torch.get_rng_state(), st)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from ggad_amd import _lib, rng
    mt = rng.DeviceMT.from_host(DEV)
    with pytest.raises(ValueError):
        mt.randn_(torch.zeros(15, device=DEV))
    with pytest.raises(ValueError):
        mt.randn_(torch.zeros(32, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        mt.randn_(torch.zeros(8, 8, device=DEV)[:, :4])
    with pytest.raises(ValueError):
        mt.randn_(torch.zeros(32))                                     # a host tensor
    lib = _lib.load()
    buf, scratch = torch.zeros(32, device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV)
    assert lib.ggad_mt_randn_f32(mt.state.data_ptr(), buf.data_ptr(), 15, 1.0, 0.0, scratch.data_ptr(), None) == _lib.GGAD_E_INVALID
    assert lib.ggad_mt_randn_f32(None, buf.data_ptr(), 32, 1.0, 0.0, scratch.data_ptr(), None) == _lib.GGAD_E_INVALID
    assert lib.ggad_mt_randn_f32(mt.state.data_ptr(), None, 32, 1.0, 0.0, scratch.data_ptr(), None) == _lib.GGAD_E_INVALID
    assert lib.ggad_mt_randn_f32(mt.state.data_ptr(), buf.data_ptr(), 32, 1.0, 0.0, None, None) == _lib.GGAD_E_INVALID
    assert lib.ggad_mt_randn_scratch_elems(300) == 316 and lib.ggad_mt_randn_scratch_elems(15) == 0
    assert lib.ggad_mt_state_words() >= 625


# ------------------------------------------------------------------------------------------------ run.fit, end of training
def _spy_on_fit(monkeypatch, seen):
    """parity_long.full_graph_long loads run.py afresh and keeps its `history` to itself: wrap the loaded module's `fit` so that the
    dict it is handed is kept."""
    real = importlib.util.module_from_spec

    def module_from_spec(spec):
        mod = real(spec)
        real_exec = spec.loader.exec_module

        def exec_module(m):
            real_exec(m)
            fit = m.fit

            def fit_spy(*a, **k):
                seen.append(k.get("history"))
                return fit(*a, **k)
            m.fit = fit_spy
        spec.loader = types.SimpleNamespace(exec_module=exec_module)
        return mod
    monkeypatch.setattr(importlib.util, "module_from_spec", module_from_spec)


def _long_run(monkeypatch, seen, fixture, device):
    import parity_long
    monkeypatch.setenv("GGAD_CAPTURE_BELOW_S", "10")      # (a busy host must not decide the path)
    if device:
        monkeypatch.setenv("GGAD_DEVICE_NOISE", "1")
    else:
        monkeypatch.delenv("GGAD_DEVICE_NOISE", raising=False)
    r = parity_long.full_graph_long(fixture=fixture)
    return r, seen[-1], torch.get_rng_state()


@pytest.mark.parametrize("fixture,epochs", [("fullgraph_long_planted.npz", 50), ("fullgraph_long_photo_schedule.npz", 100)])
def test_end_of_training_parity_with_device_noise(fixture, epochs, capsys, monkeypatch):
    """The assertions of the two host-path tests (tests/test_fullgraph_gpu.py: loss curve to 2e-4, every AUROC / AP to 1e-4 against
    the imported reference's dense run) with the noise of all epochs and evaluations drawn on the device.  Both fixtures draw 89 x 300
    values: 26,700 is not a multiple of 16, so every draw takes the tail rule.  The host generator ends byte-equal to where the host
    path leaves it."""
    seen = []
    _spy_on_fit(monkeypatch, seen)
    r_host, h_host, st_host = _long_run(monkeypatch, seen, fixture, False)
    r, h, st_dev = _long_run(monkeypatch, seen, fixture, True)
    assert len(seen) == 2
    with capsys.disabled():
        print(f"\n[end-of-training parity, device noise, {fixture}]", r)
        print(f"[the host path on the same machine] loss_delta_max {r_host['loss_delta_max']:.3e}, "
              f"auc {r_host['eval_auc_delta_max']:.3e}, ap {r_host['eval_ap_delta_max']:.3e}")
    assert "noise" not in h_host and h["noise"] == "device"
    assert r["epochs"] == epochs and r["captured"] and h["captured"]
    if fixture == "fullgraph_long_planted.npz":
        assert r["final_auc"][1] >= 0.8 and r["final_ap"][1] >= 0.5
    assert r["loss_delta_max"] < 2e-4
    assert r["eval_auc_delta_max"] <= 1e-4 and r["eval_ap_delta_max"] <= 1e-4
    assert r["final_auc_delta"] <= 1e-4 and r["final_ap_delta"] <= 1e-4
    assert r["weight_norm_rel_delta_max"] < 1e-4
    assert torch.equal(st_dev, st_host)


def test_fit_hands_the_stream_back_on_an_exception(monkeypatch):
    """`run.fit` with the flag: an exception inside the loop still returns the generator to the host (here: unchanged, nothing was
    drawn) and clears the model's attributes."""
    import run
    from ggad_amd import rng
    st = _host_state(0)
    calls = []
    real = rng.DeviceMT.to_host
    monkeypatch.setattr(rng.DeviceMT, "to_host", lambda self: (calls.append(1), real(self))[1])

    def boom(*a, **k):
        raise KeyError("stop")
    monkeypatch.setattr(run, "_fit", boom)
    model = types.SimpleNamespace(device_noise=None, noise_override=None)
    hist = {}
    with pytest.raises(KeyError):
        run.fit(types.SimpleNamespace(device_noise=True), torch.device(DEV), None, None, model, [], [], [], None, history=hist)
    assert calls == [1] and model.device_noise is None and hist["noise"] == "device"
    assert torch.equal(torch.get_rng_state(), st)


# ------------------------------------------------------------------------------------------------ GAAN and AEGIS, planted
def _setup(c, which):
    from ggad_amd import synth
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.utils import normalize_adj
    Model = importlib.import_module("ggad_amd.model_" + which).Model
    n = int(c["n"])
    adj = synth.csr_to_scipy(c["rowptr"], c["col"], n)
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(n), adj + sp.eye(n), DEV)
    torch.manual_seed(int(c["seed"]))
    model = Model(int(c["f"]), int(c["n_h"]), "prelu", 1, "avg").to(DEV)
    x = torch.from_numpy(c["features"]).float().to(DEV)[None]
    return full, model, x


def _host_state_after(st, n, draws):
    torch.set_rng_state(st)
    for _ in range(draws):
        torch.randn(n, 16)
    return torch.get_rng_state()


def test_gaan_planted_auroc_ap_with_device_noise():
    """tests/test_gaan_gpu.py::test_planted_auroc_ap_at_every_print_epoch with `model.device_noise` set: same fixture, same bound."""
    from ggad_amd import rng
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.metrics import average_precision, roc_auc
    c = load_golden("fullgraph_gaan_planted.npz")
    full, model, x = _setup(c, "gaan")
    st = torch.get_rng_state()
    model.device_noise = mt = rng.DeviceMT.from_host(DEV)
    lr = float(c["lr"])
    all_idx, idx_test = list(c["all_idx"]), c["idx_test"]
    opt = FlatAdam(model.parameters(), lr=lr)
    opt_gen = FlatAdam(model.generator.parameters(), lr=lr)
    yt = torch.as_tensor(c["ano"][idx_test].astype(np.int64), device=DEV)
    aucs, aps = [], []
    for epoch in range(int(c["num_epoch"])):
        model.train()
        opt.zero_grad()
        opt_gen.zero_grad()
        loss, loss_g, score = model(x, full, all_idx, idx_test)
        torch.autograd.backward([loss, loss_g])
        opt.step()
        opt_gen.step()
        if epoch % 5 == 0:
            aucs.append(roc_auc(score.view(-1), yt))
            aps.append(average_precision(score.view(-1), yt))
            model.eval()
    mt.to_host()
    assert torch.equal(torch.get_rng_state(), _host_state_after(st, int(c["n"]), int(c["num_epoch"])))
    tol_auc = max(1e-4, 3 * float(np.max(c["self_sens_auc"])))
    tol_ap = max(1e-4, 3 * float(np.max(c["self_sens_ap"])))
    assert np.all(np.abs(np.array(aucs) - c["auc"]) <= tol_auc), (aucs, c["auc"])
    assert np.all(np.abs(np.array(aps) - c["ap"]) <= tol_ap), (aps, c["ap"])


def test_aegis_planted_auroc_ap_with_device_noise():
    """tests/test_aegis_gpu.py::test_planted_auroc_ap_at_every_print_epoch with `model.device_noise` set (the reconstruction epochs
    draw too): same fixture, same bound."""
    from ggad_amd import rng
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.metrics import average_precision, roc_auc
    c = load_golden("fullgraph_aegis_planted.npz")
    full, model, x = _setup(c, "aegis")
    st = torch.get_rng_state()
    model.device_noise = mt = rng.DeviceMT.from_host(DEV)
    lr = float(c["lr"])
    all_idx, normal_idx, idx_test = list(c["all_idx"]), list(c["normal_idx"]), c["idx_test"]
    opt_ae = FlatAdam(model.parameters(), lr=1e-3)
    opt = FlatAdam(model.parameters(), lr=lr)
    opt_gen = FlatAdam(model.generator.parameters(), lr=lr)
    for _ in range(int(c["recon_epochs"])):
        loss_ae, _, _, _, _, _ = model.train_forward(x, full, normal_idx, idx_test)
        loss_ae.backward()
        opt_ae.step()
    yt = torch.as_tensor(c["ano"][idx_test].astype(np.int64), device=DEV)
    aucs, aps = [], []
    for epoch in range(int(c["num_epoch"])):
        model.train()
        opt.zero_grad()
        opt_gen.zero_grad()
        loss_ae, loss_g, score, _, _, _ = model.train_forward(x, full, all_idx, idx_test)
        torch.autograd.backward([loss_g, loss_ae])
        opt.step()
        opt_gen.step()
        if epoch % 5 == 0:
            aucs.append(roc_auc(score.view(-1), yt))
            aps.append(average_precision(score.view(-1), yt))
            model.eval()
    mt.to_host()
    assert torch.equal(torch.get_rng_state(), _host_state_after(st, int(c["n"]), int(c["recon_epochs"]) + int(c["num_epoch"])))
    tol_auc = max(2e-4, 5 * float(np.max(c["self_sens_auc"])))
    tol_ap = max(2e-4, 5 * float(np.max(c["self_sens_ap"])))
    assert np.all(np.abs(np.array(aucs) - c["auc"]) <= tol_auc), (aucs, c["auc"])
    assert np.all(np.abs(np.array(aps) - c["ap"]) <= tol_ap), (aps, c["ap"])


# ------------------------------------------------------------------------------------------------ the scripts
def _script_lines(script, args):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("GGAD_DEVICE_NOISE", None)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, script)] + args
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith(("Epoch:", "Testing"))], r.stdout


def test_gaan_script_captured_equals_eager_with_device_noise():
    args = ["--dataset", "Amazon", "--synthetic", "--num_epoch", "22", "--quiet", "--device_noise"]
    graph, raw_g = _script_lines("gaan.py", args)
    eager, raw_e = _script_lines("gaan.py", args + ["--no_graph"])
    assert "training epoch captured as a hipGraph" in raw_g and "training epoch captured" not in raw_e
    assert graph == eager
    assert sum(ln.startswith("Epoch:") and "train_loss=" in ln for ln in graph) == 5
    assert sum(ln.startswith("Testing Amazon AUC:") for ln in graph) == 5


def test_aegis_script_captured_equals_eager_with_device_noise():
    args = ["--dataset", "reddit", "--synthetic", "--num_epoch", "22", "--quiet", "--device_noise"]
    graph, raw_g = _script_lines("aegis.py", args)
    eager, raw_e = _script_lines("aegis.py", args + ["--no_graph"])
    assert "training epoch captured as a hipGraph" in raw_g and "training epoch captured" not in raw_e
    assert graph == eager
    assert sum(ln.startswith("Epoch:") and "ae_loss=" in ln for ln in graph) == 10
    assert sum(ln.startswith("Testing reddit AUC:") for ln in graph) == 5


def test_run_script_captured_equals_eager_with_device_noise():
    args = ["--dataset", "reddit", "--synthetic", "--num_epoch", "13", "--device_noise"]
    graph, raw_g = _script_lines("run.py", args)
    eager, raw_e = _script_lines("run.py", args + ["--no_graph"])
    assert "training epoch captured as a hipGraph" in raw_g and "training epoch captured" not in raw_e
    assert len(graph) >= 7 * 4 + 4
    assert graph == eager
