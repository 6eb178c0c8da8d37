"""What the device path of the mini-batch DOMINANT / AnomalyDAE handlers can be held to without a GPU: the float64 restatement the
GPU tests measure against (`tests/recon_mb_fp64.py`) reproduces the trajectory recorded from the reference; the new entry points
refuse bad arguments before any launch; `ReconDevice.bind` refuses tensors the kernels cannot read; the switch is off by default."""
import types

import numpy as np
import pytest
import torch

import recon_mb_fp64 as R
from conftest import load_golden
from ggad_amd import _lib, synth
from ggad_amd.recon_device import ReconDevice

TAGS = [("dominant", (1.0, 1.0)), ("anomalydae", (0.5, 0.5))]


@pytest.mark.parametrize("tag,weights", TAGS)
def test_float64_restatement_reproduces_the_reference_trajectory(tag, weights):
    """Five steps of 48 rows, F = 17, D = 64; the bounds `tests/test_baselines_gpu.py` holds the default path to on the same arrays."""
    g = load_golden("minibatch_baselines.npz")
    x1, t, bp = R.golden_tables(g)
    assert x1.shape == (5 * 48, 17) and list(np.diff(bp)) == [48] * 5
    np.testing.assert_allclose(x1[:48], g[f"{tag}.agg_to_feats"], atol=2e-6, rtol=0)
    losses, first, last = R.run_steps(x1, t, bp, g[f"{tag}.init.enc.weight"], g[f"{tag}.init.enc.fc.weight"], *weights)
    np.testing.assert_allclose(losses, g[f"{tag}.losses"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(first["grad.w"], g[f"{tag}.grad.enc.weight"], atol=3e-6, rtol=1e-4)
    np.testing.assert_allclose(first["grad.fc"], g[f"{tag}.grad.enc.fc.weight"], atol=3e-6, rtol=1e-4)
    np.testing.assert_allclose(first["w"], g[f"{tag}.step1.enc.weight"], atol=3e-6, rtol=0)
    np.testing.assert_allclose(first["fc"], g[f"{tag}.step1.enc.fc.weight"], atol=3e-6, rtol=0)
    np.testing.assert_allclose(last["w"], g[f"{tag}.final.enc.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(last["fc"], g[f"{tag}.final.enc.fc.weight"], atol=2e-5, rtol=0)
    assert float(np.abs(first["grad.w"]).max()) > 1e-4          # a live gradient, not zeros against zeros


@pytest.mark.parametrize("tag,weights", TAGS)
def test_float64_score_reproduces_the_reference_scores(tag, weights):
    from oracle import ggad_oracle as O
    g = load_golden("minibatch_baselines.npz")
    nodes, bs = g["test_nodes"], int(g["test_bs"])
    xs = [O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes[s:s + bs], False, dtype=np.float64).to_feats
          for s in range(0, len(nodes), bs)]
    got = R.scores(np.concatenate(xs), g["feat"][nodes], g[f"{tag}.final.enc.weight"], g[f"{tag}.final.enc.fc.weight"])
    np.testing.assert_allclose(got, g[f"{tag}.test_scores"], atol=2e-5, rtol=0)


def test_dead_column_has_a_finite_float64_gradient():
    """A column with r = 0 and t = 0 over the whole batch: s_c = 0 and 0/0 behind the ReLU's select; torch drops it."""
    x1, t, w, wfc = R.make_case(48, 17, 5)
    wfc[3] = -np.abs(wfc[3]) - 0.5          # h >= 0, so r[:, 3] = 0
    t[:, 3] = 0.0
    got = R.step(x1, t, w, wfc, w_pos=0.8, w_neg=0.2)
    assert all(np.isfinite(v).all() for v in got.values())
    assert float(np.abs(got["grad.fc"][3]).max()) == 0.0 and float(np.abs(got["grad.w"]).max()) > 1e-4


def test_entry_points_refuse_bad_arguments_without_a_launch():
    lib = _lib.load()
    assert lib.ggad_abi_version() == 11
    assert lib.ggad_recon_mb_max_rows(17) >= 256 and lib.ggad_recon_mb_max_rows(32) >= 256 and lib.ggad_recon_mb_max_rows(64) >= 150
    assert lib.ggad_recon_mb_max_rows(0) == 0 and lib.ggad_recon_mb_max_rows(65) == 0
    assert lib.ggad_recon_mb_supported(1, 64, 1) and lib.ggad_recon_mb_supported(64, 64, lib.ggad_recon_mb_max_rows(64))
    for bad in ((0, 64, 1), (65, 64, 1), (17, 32, 1), (17, 64, 0), (17, 64, lib.ggad_recon_mb_max_rows(17) + 1),
                (64, 64, lib.ggad_recon_mb_max_rows(64) + 1)):
        assert not lib.ggad_recon_mb_supported(*bad), bad
    p = 4096          # stands for a non-null pointer: every case below is refused before anything is read

    def steps(ptrs=None, n_steps=1, total=48, max_rows=48, f=17, d=64):
        ptrs = [p] * 3 + [p] * 8 + [p] * 3 if ptrs is None else ptrs
        return lib.ggad_recon_mb_steps_f32(*ptrs[:3], n_steps, total, max_rows, f, d, *ptrs[3:11], 1e-3, 0.007, 1.0, 1.0, *ptrs[11:14], None)

    for i in range(12):          # x1, target, batch_ptr, the two weights, four moments, two counters, losses (the gradients may be null)
        ptrs = [p] * 14
        ptrs[i] = None
        assert steps(ptrs) == _lib.GGAD_E_INVALID, i
    assert steps(f=0) == -1 and steps(f=65) == -1 and steps(d=32) == -1 and steps(d=65) == -1
    assert steps(max_rows=lib.ggad_recon_mb_max_rows(17) + 1, total=1000) == -1
    assert steps(f=64, max_rows=lib.ggad_recon_mb_max_rows(64) + 1, total=1000) == -1
    assert steps(n_steps=0) == -1 and steps(n_steps=-3) == -1 and steps(max_rows=0) == -1

    def scores(ptrs=None, rows=10, f=17, d=64):
        ptrs = [p] * 5 if ptrs is None else ptrs
        return lib.ggad_recon_mb_scores_f32(ptrs[0], ptrs[1], rows, f, d, ptrs[2], ptrs[3], ptrs[4], None)

    for i in range(5):
        ptrs = [p] * 5
        ptrs[i] = None
        assert scores(ptrs) == -1, i
    assert scores(f=0) == -1 and scores(f=65) == -1 and scores(d=32) == -1 and scores(rows=-1) == -1


class _Enc:
    def __init__(self, w, fc, f=17, d=64):
        self.feat_dim, self.embed_dim = f, d
        self.weight = w
        self.fc = types.SimpleNamespace(weight=fc)


def test_bind_refuses_tensors_the_kernels_cannot_read():
    good_w, good_fc = torch.zeros(64, 17), torch.zeros(17, 64)
    cases = {"float64": (good_w.double(), good_fc), "float64 fc": (good_w, good_fc.double()),
             "non-contiguous": (torch.zeros(17, 64).t(), good_fc), "cpu": (good_w, good_fc), "shape": (torch.zeros(64, 18), good_fc)}
    for name, (w, fc) in cases.items():
        rd = ReconDevice()
        with pytest.raises(ValueError):
            rd.bind(_Enc(w, fc))
        assert rd.enc is None, name
    for f, d in ((65, 64), (0, 64), (17, 32)):
        with pytest.raises(ValueError):
            ReconDevice().bind(_Enc(good_w, good_fc, f, d))


def _cfg(data, **kw):
    cfg = dict(data_name="dgraphfin", data_dir="./data/", train_ratio=0.4, test_ratio=0.67, save_dir="./pytorch_models/",
               model="GCN", multi_relation="GNN", emb_size=64, thres=0.4, rho=0.5, seed=72, optimizer="adam", lr=0.001,
               weight_decay=0.007, batch_size=150, num_epochs=2, valid_epochs=5, alpha=2, no_cuda=False, cuda_id="0", data=data)
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("which", ["dominate", "anomalydae"])
def test_a_config_without_the_key_builds_no_recon_device(which, capsys, monkeypatch):
    """`build_model` as the handler runs it, with the feature table left on the CPU (the one thing patched): nothing is launched
    while a model is built."""
    import importlib
    from ggad_amd import graphsage
    monkeypatch.setattr(graphsage, "_device", lambda: torch.device("cpu"))
    mh = importlib.import_module(f"ggad_amd.model_handler_{which}")
    n, f = 600, 17
    rowptr, col = synth.make_graph(n, 3000, 3, kind="powerlaw", max_degree=40)
    data = ((rowptr, col), synth.make_features(n, f, 3), synth.make_labels(n, 0.05, 3).astype(np.int32))
    for kw in ({}, {"recon_device": False}):
        h = mh.ModelHandler(_cfg(data, **kw))
        _, _, model = h.build_model(torch.device("cpu"))
        assert model.enc.recon_device is None
    with pytest.raises(ValueError):          # the switch builds one, and one cannot be bound to CPU tensors: no quiet fallback
        mh.ModelHandler(_cfg(data, recon_device=True)).build_model(torch.device("cpu"))
    capsys.readouterr()
