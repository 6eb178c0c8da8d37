"""Embedding widths above 64 on the mini-batch path, the parts that need no GPU: the CPU oracle against what the imported
reference returned at d = 128 and d = 200 (tests/golden/make_golden_wide.py; the assertions and tolerances of
tests/test_oracle_golden.py for `minibatch_small` / `minibatch_dense`), and the C-ABI limits of the wide step chain."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from ggad_amd import _lib, synth
from oracle import ggad_oracle as O

TOL = 2e-6
WIDE = ["minibatch_wide128.npz", "minibatch_wide200.npz"]


def _mini_params(g, prefix):
    return O.MiniParams(torch.tensor(g[prefix + ".weight"], requires_grad=True),
                        torch.tensor(g[prefix + ".enc.weight"], requires_grad=True),
                        torch.tensor(g[prefix + ".enc.fc.weight"], requires_grad=True))


@pytest.mark.parametrize("name", WIDE)
def test_inputs_regenerate(name):
    g = load_golden(name)
    assert int(g["d"]) in (128, 200)
    assert synth.crc_of(g["rowptr"], g["col"], g["feat_raw"]) == int(g["inputs_crc"])
    np.testing.assert_allclose(O.normalize_rows(g["feat_raw"]).astype(np.float32), g["feat"], rtol=0, atol=1e-7)


@pytest.mark.parametrize("name", WIDE)
def test_aggregator_closed_form(name):
    g = load_golden(name)
    nodes = g["batches"][0]
    agg = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True)
    np.testing.assert_allclose(agg.to_feats, g["agg_to_feats"], atol=TOL, rtol=0)
    ref_u = g["agg_unique"]
    assert sorted(ref_u.tolist()) == agg.unique.tolist()
    perm = np.searchsorted(agg.unique, ref_u)
    np.testing.assert_allclose(agg.to_feats_neigh[perm], g["agg_to_feats_neigh"], atol=TOL, rtol=0)
    np.testing.assert_allclose(agg.mask_row_dense()[:, perm], g["agg_mask_row"], atol=1e-7, rtol=0)


@pytest.mark.parametrize("name", WIDE)
def test_encoder_loss_grads_and_adam_trajectory(name):
    g = load_golden(name)
    p = _mini_params(g, "init")
    assert tuple(p.enc_fc_weight.shape) == (int(g["d"]), int(g["d"]))
    opt = O.make_adam(p.tensors(), 1e-3, 0.007)
    for step, (nodes, lab) in enumerate(zip(g["batches"], g["labels"])):
        agg = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True)
        if step == 0:
            with torch.no_grad():
                ca, nbar, af, afn = O.encoder_forward(p, agg, lab, True)
            np.testing.assert_allclose(ca.numpy(), g["enc_combined_all"], atol=TOL, rtol=0)
            np.testing.assert_allclose(nbar.numpy(), g["enc_to_feats_neigh"], atol=TOL, rtol=0)
            np.testing.assert_allclose(af.numpy(), g["enc_anomaly_feat"], atol=TOL, rtol=0)
            np.testing.assert_allclose(afn.numpy(), g["enc_anomaly_feat_new"], atol=TOL, rtol=0)
        opt.zero_grad()
        total, cls, margin, rec = O.batch_loss(p, agg, lab)
        total.backward()
        got = np.array([total.item(), cls.item(), margin.item(), rec.item()])
        np.testing.assert_allclose(got, g["losses"][step], atol=5e-6, rtol=0)
        if step == 0:
            np.testing.assert_allclose(p.weight.grad.numpy(), g["grad.weight"], atol=TOL, rtol=1e-5)
            np.testing.assert_allclose(p.enc_weight.grad.numpy(), g["grad.enc.weight"], atol=TOL, rtol=1e-5)
            np.testing.assert_allclose(p.enc_fc_weight.grad.numpy(), g["grad.enc.fc.weight"], atol=TOL, rtol=1e-5)
        opt.step()
        if step == 0:
            np.testing.assert_allclose(p.enc_weight.detach().numpy(), g["step1.enc.weight"], atol=TOL, rtol=0)
    np.testing.assert_allclose(p.weight.detach().numpy(), g["final.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(p.enc_weight.detach().numpy(), g["final.enc.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(p.enc_fc_weight.detach().numpy(), g["final.enc.fc.weight"], atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", WIDE)
def test_to_prob_reference_batches(name):
    g = load_golden(name)
    p = _mini_params(g, "final")
    bs = int(g["test_bs"])
    nodes = g["test_nodes"]
    got = []
    for s in range(0, len(nodes), bs):
        got.extend(O.to_prob(p, g["rowptr"], g["col"], g["feat"], nodes[s:s + bs]).tolist())
    np.testing.assert_allclose(np.array(got, dtype=np.float32), g["test_probs"], atol=TOL, rtol=0)


def test_wide_limits_of_the_c_abi():
    lib = _lib.load()
    assert lib.ggad_mb_wide_max_embed_dim() == 256
    assert lib.ggad_max_embed_dim() == 64                       # the one-lane-per-channel kernels keep their limit
    for d, f in ((65, 1), (256, 128), (128, 17)):
        assert lib.ggad_mb_wide_supported(d, f) == 1, (d, f)
    assert lib.ggad_mb_wide_supported(257, 17) == 0
    assert lib.ggad_mb_wide_supported(128, 0) == 0 and lib.ggad_mb_wide_supported(0, 17) == 0
    for f in (1, 17, 128):                                      # every F from 1 to at least 128 at every wide D
        assert all(lib.ggad_mb_wide_supported(d, f) == 1 for d in range(65, 257)), f
    for f in (1, 17, 128):
        want = 256 + 256 * f + 256 * 256
        assert lib.ggad_mb_param_count(256, f) == want
        assert lib.ggad_mb_param_block_elems(256, f) == want + f * 256 + 256 * 256
        assert lib.ggad_mb_dw_part_elems(200, 256, f) == lib.ggad_mb_bwd_parts() * f * 256
        assert lib.ggad_mb_dw_part_elems(410, 256, f) == 410 * f * 256
    # d w partials: one block of 64 ceil(D / 64) floats per loss workgroup (4 rows), sized for D = 256
    for rows in (1, 2, 50, 410):
        nwg = (rows + 3) // 4
        assert lib.ggad_mb_loss_workspace_elems(rows) >= rows * 8 + nwg * 8 + nwg * 256
    # argument checks happen before any launch, so they can be exercised without a device
    assert lib.ggad_mb_params_sync(None, 128, 17, None) == -1
    assert lib.ggad_mb_project(None, 128, 17, None, None, 0, 0, None, None) == -1
    assert lib.ggad_mb_project(None, 257, 17, None, None, 0, 0, None, None) == -1
