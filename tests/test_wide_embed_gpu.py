"""The wide step chain (csrc/step_wide.hip): mini-batch GGAD at embedding widths 64 < D <= 256, and -- as `chain=3` -- the same
kernels at D <= 64 where the one-lane-per-channel kernels are already pinned.

  1. reference vectors at D = 128 / 200 (tests/golden/make_golden_wide.py), engine and drop-in classes;
  2. chain 3 against the existing D = 64 / D = 32 reference vectors and against chain 2 on random batches;
  3. every branch against the float64 oracle with the bounds of tests/step_reference.py (|HIP - float64|: losses 1e-5,
     gradients 3e-6 + 2e-5 |g|, the masked one-step Adam rule and its moment bounds), D in {65, 128, 129, 192, 255, 256} at F = 17
     and (D, F) in {(96, 1), (200, 9), (256, 70), (130, 128)}, on batches that hold a hub row of more than 1,024 entries (second
     pass of the forward-rows block loop), a row of closed size 2, a duplicated node, label-1 rows in the middle, exactly one
     label-1 row, two rows (1 + 1) and 333 + 77 rows (more than 256 positions / one bwd_flat part per row);
  4. determinism, Adam fused into the last launch, padding never read;
  5. DGraphTrainer / ModelHandler at emb_size 128;
  6. what stays refused.
"""
import functools
import glob
import os
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
from ggad_amd import synth
from oracle import ggad_oracle as O
import step_reference as R
import width_reference as WR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.minibatch import BatchChunk, MiniBatchEngine

DEV = "cuda:0"
WIDE = ["minibatch_wide128.npz", "minibatch_wide200.npz"]


def _setup(g, train=True, max_batches=8):
    graph = DeviceGraph(g["rowptr"], g["col"], DEV)
    feat = torch.from_numpy(np.ascontiguousarray(g["feat"])).to(DEV)
    ch = BatchChunk(graph, feat, int(g["d"]), max_batches=max_batches, rows_cap=64, ent_cap=64, train=train, hop2="ldsw")
    return graph, feat, ch


# ------------------------------------------------------------------ 1 + 2a: reference vectors
def _trajectory_vs_golden(g, chain):
    """The assertions of tests/test_minibatch_gpu.py::test_loss_grads_adam_trajectory_vs_golden."""
    graph, feat, ch = _setup(g)
    eng = MiniBatchEngine(int(g["f"]), int(g["d"]), DEV, lr=1e-3, weight_decay=0.007, chain=chain)
    assert eng.wide and not eng.resident
    eng.load_params(g["init.weight"], g["init.enc.weight"], g["init.enc.fc.weight"])
    batches = [b for b in g["batches"]]
    labels = [l for l in g["labels"]]
    ch.build(batches, labels)
    k = len(batches)
    for b in range(k):
        eng.loss_and_grads(ch, b, b)
        if b == 0:
            D, F = eng.D, eng.F
            gr = eng.grads.cpu().numpy()
            np.testing.assert_allclose(gr[:D].reshape(1, D), g["grad.weight"], atol=2e-6, rtol=1e-5)
            np.testing.assert_allclose(gr[D:D + D * F].reshape(D, F), g["grad.enc.weight"], atol=2e-6, rtol=1e-5)
            np.testing.assert_allclose(gr[D + D * F:].reshape(D, D), g["grad.enc.fc.weight"], atol=2e-6, rtol=1e-5)
            r0, r1 = ch.batch_rows(0)
            h1 = ch.h1[:ch.n_rows * D].view(-1, D)[r0:r1].cpu().numpy()
            nbar = ch.nbar[:ch.n_rows * D].view(-1, D)[r0:r1].cpu().numpy()
            gen = ch.gen[:ch.n_rows * D].view(-1, D)[r0:r1].cpu().numpy()
            lab = labels[0]
            np.testing.assert_allclose(nbar, g["enc_to_feats_neigh"], atol=2e-6, rtol=0)
            np.testing.assert_allclose(h1[lab == 1].T, g["enc_anomaly_feat"], atol=2e-6, rtol=0)
            np.testing.assert_allclose(gen[lab == 1].T, g["enc_anomaly_feat_new"], atol=2e-6, rtol=0)
            comb = np.concatenate([h1[lab == 0], gen[lab == 1]]).T
            np.testing.assert_allclose(comb, g["enc_combined_all"], atol=2e-6, rtol=0)
        eng.adam_step()
        if b == 0:
            np.testing.assert_allclose(eng.enc_weight.cpu().numpy(), g["step1.enc.weight"], atol=2e-6, rtol=0)
            np.testing.assert_allclose(eng.enc_fc_weight.cpu().numpy(), g["step1.enc.fc.weight"], atol=2e-6, rtol=0)
            np.testing.assert_allclose(eng.weight.cpu().numpy(), g["step1.weight"], atol=2e-6, rtol=0)
    np.testing.assert_allclose(eng.losses(k), g["losses"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(eng.weight.cpu().numpy(), g["final.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(eng.enc_weight.cpu().numpy(), g["final.enc.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(eng.enc_fc_weight.cpu().numpy(), g["final.enc.fc.weight"], atol=2e-5, rtol=0)
    D, F = eng.D, eng.F
    nt = eng.n_train
    wt = eng.params[nt:nt + F * D].view(F, D).cpu().numpy()
    np.testing.assert_array_equal(wt, eng.enc_weight.cpu().numpy().T)
    fct = eng.params[nt + F * D:].view(D, D).cpu().numpy()
    np.testing.assert_array_equal(fct, eng.enc_fc_weight.cpu().numpy().T)
    # the whole chunk in one host call (Adam fused into the last launch) walks the same trajectory
    eng2 = MiniBatchEngine(int(g["f"]), int(g["d"]), DEV, lr=1e-3, weight_decay=0.007, chain=chain)
    eng2.load_params(g["init.weight"], g["init.enc.weight"], g["init.enc.fc.weight"])
    eng2.train_chunk(ch)
    np.testing.assert_array_equal(eng2.params.cpu().numpy(), eng.params.cpu().numpy())
    np.testing.assert_array_equal(eng2.losses(k), eng.losses(k))


def _to_prob_vs_golden(g, chain):
    """The assertions of tests/test_minibatch_gpu.py::test_to_prob_vs_golden."""
    graph, feat, ch = _setup(g, train=False, max_batches=4)
    eng = MiniBatchEngine(int(g["f"]), int(g["d"]), DEV, chain=chain)
    eng.load_params(g["final.weight"], g["final.enc.weight"], g["final.enc.fc.weight"])
    nodes = g["test_nodes"]
    bs = int(g["test_bs"])
    batches = [nodes[s:s + bs] for s in range(0, len(nodes), bs)]   # reference batch boundaries, last one ragged
    ch.build(batches)
    out = torch.empty(len(nodes), dtype=torch.float32, device=DEV)
    eng.score_chunk(ch, out)
    np.testing.assert_allclose(out.cpu().numpy(), g["test_probs"], atol=2e-6, rtol=0)
    torch.cuda.synchronize()
    assert int(ch.cnt1.abs().sum()) == 0


@pytest.mark.parametrize("name", WIDE)
def test_loss_grads_adam_trajectory_vs_golden_wide(name):
    _trajectory_vs_golden(load_golden(name), chain=0)


@pytest.mark.parametrize("name", WIDE)
def test_to_prob_vs_golden_wide(name):
    _to_prob_vs_golden(load_golden(name), chain=0)


@pytest.mark.parametrize("name", WIDE)
def test_encoder_forward_and_autograd_wide(name):
    """`GCNEncoder.forward(..., train_flag=True)` and autograd through `_EncoderRows` / `GCN.loss` (`_FusedBatchLoss`) against
    `enc_*` and `grad.*`, as tests/test_dropin_gpu.py does at D = 64 / 32."""
    from ggad_amd.graphsage import GCN, GCNAggregator, GCNEncoder
    g = load_golden(name)
    adj = synth.csr_to_adj_lists(g["rowptr"], g["col"])
    feats = torch.nn.Embedding(int(g["n"]), int(g["f"]))
    feats.weight = torch.nn.Parameter(torch.from_numpy(g["feat"]), requires_grad=False)
    agg = GCNAggregator(feats, cuda=True)
    enc = GCNEncoder(feats, int(g["f"]), int(g["d"]), adj, agg, gcn=True, cuda=True)
    model = GCN(2, enc)
    with torch.no_grad():
        model.weight.copy_(torch.from_numpy(g["init.weight"]))
        enc.weight.copy_(torch.from_numpy(g["init.enc.weight"]))
        enc.fc.weight.copy_(torch.from_numpy(g["init.enc.fc.weight"]))
    nodes, lab = g["batches"][0].tolist(), g["labels"][0]
    combined_all, nbar, a_feat, a_new = enc.forward(nodes, torch.LongTensor(lab), True)
    np.testing.assert_allclose(combined_all.detach().cpu().numpy(), g["enc_combined_all"], atol=2e-6, rtol=0)
    np.testing.assert_allclose(nbar.detach().cpu().numpy(), g["enc_to_feats_neigh"], atol=2e-6, rtol=0)
    np.testing.assert_allclose(a_feat.detach().cpu().numpy(), g["enc_anomaly_feat"], atol=2e-6, rtol=0)
    np.testing.assert_allclose(a_new.detach().cpu().numpy(), g["enc_anomaly_feat_new"], atol=2e-6, rtol=0)
    # the reference's GCN.loss written with torch ops on the layered outputs (graphsage.py:244-258); gradients flow through the
    # HIP vector-Jacobian product of the encoder (row_coefs -> bwd_flat -> grad_reduce)
    scores, tfn, embeds, af, afn = model.forward(nodes, torch.LongTensor(lab), True)
    labt = torch.as_tensor(lab, device=DEV)
    cls = torch.mean(torch.nn.functional.binary_cross_entropy_with_logits(scores.squeeze(), labt.float(), reduction="none"))
    aff = torch.cosine_similarity(embeds, tfn.t(), dim=0)
    margin = (1 - (aff[labt == 0].mean() - aff[labt == 1].mean())).clamp_min(0)
    rec = torch.mean(torch.sqrt(torch.sum(torch.pow(af - afn, 2), 0)))
    total = cls + margin + 0.1 * rec
    np.testing.assert_allclose([total.item(), cls.item(), margin.item(), rec.item()], g["losses"][0], atol=1e-5)
    total.backward()
    np.testing.assert_allclose(model.weight.grad.cpu().numpy(), g["grad.weight"], atol=3e-6, rtol=1e-4)
    np.testing.assert_allclose(enc.weight.grad.cpu().numpy(), g["grad.enc.weight"], atol=3e-6, rtol=1e-4)
    np.testing.assert_allclose(enc.fc.weight.grad.cpu().numpy(), g["grad.enc.fc.weight"], atol=3e-6, rtol=1e-4)
    emb, n1, n2, n3 = enc.forward(nodes, None, False)
    assert n1 is None and n2 is None and n3 is None and emb.shape == (int(g["d"]), len(nodes))
    np.testing.assert_allclose(emb.cpu().numpy()[:, lab == 1], g["enc_anomaly_feat"], atol=2e-6, rtol=0)
    # GCN.loss: the fused chain; its gradients against the same vectors with the engine test's tolerances
    for p in (model.weight, enc.weight, enc.fc.weight):
        p.grad = None
    total2, cls2, margin2, rec2 = model.loss(nodes, torch.LongTensor(lab))
    total2.backward()
    np.testing.assert_allclose([total2.item(), cls2.item(), margin2.item(), rec2.item()], g["losses"][0], atol=1e-5)
    np.testing.assert_allclose(model.weight.grad.cpu().numpy(), g["grad.weight"], atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(enc.weight.grad.cpu().numpy(), g["grad.enc.weight"], atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(enc.fc.weight.grad.cpu().numpy(), g["grad.enc.fc.weight"], atol=2e-6, rtol=1e-5)
    prob = model.to_prob(nodes[:30], None)
    assert tuple(prob.shape) == (30, 1)


@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_chain3_vs_golden_at_narrow_widths(name):
    """The wide kernels with one full channel slot (D = 64) and one partial slot (D = 32) on the reference vectors the D <= 64
    kernels are pinned to."""
    g = load_golden(name)
    _trajectory_vs_golden(g, chain=3)
    _to_prob_vs_golden(g, chain=3)


def _random_case(n, n_entries, f, d, seed, nb, bsz, n_ano):
    """tests/test_minibatch_gpu.py::_random_case"""
    rowptr, col = synth.make_graph(n, n_entries, seed, kind="powerlaw", max_degree=300, self_loop_frac=0.02)
    feat = O.normalize_rows(synth.make_features(n, f, seed)).astype(np.float32)
    rng = np.random.default_rng(seed + 3)
    batches, labels = [], []
    hub = int(np.argmax(np.diff(rowptr)))
    for b in range(nb):
        nodes = rng.choice(n, size=bsz, replace=False)
        if b == 0:
            nodes[3] = hub
            nodes[7] = nodes[5]
        lab = np.zeros(bsz, dtype=np.int64)
        lab[bsz - n_ano:] = 1
        lab[rng.choice(bsz - n_ano, size=3, replace=False)] = 1
        batches.append(nodes)
        labels.append(lab)
    return dict(rowptr=rowptr, col=col, feat=feat, f=f, d=d), batches, labels


@pytest.mark.parametrize("d,bsz,n_ano", [(64, 200, 50), (32, 333, 77), (48, 23, 5)])
def test_chain3_equals_chain2(d, bsz, n_ano):
    """Chain 3 (wide kernels) against chain 2 (the layered D <= 64 kernels) with the bounds
    test_fused_forward_chain_equals_six_launch_chain uses between chains: 1e-6 absolute, 1e-5 relative on gradients."""
    g, batches, labels = _random_case(n=12000, n_entries=150000, f=17, d=d, seed=31 + d, nb=3, bsz=bsz, n_ano=n_ano)
    torch.manual_seed(d)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, d))
    W = torch.nn.init.xavier_uniform_(torch.empty(d, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(d, d))
    res = {}
    for chain in (3, 2):
        graph, feat, ch = _setup(g, max_batches=3)
        eng = MiniBatchEngine(17, d, DEV, chain=chain)
        eng.load_params(w, W, fc)
        ch.build(batches, labels)
        grads = []
        for b in range(3):
            eng.loss_and_grads(ch, b, b)
            grads.append(eng.grads.cpu().numpy().copy())
            eng.adam_step()
        res[chain] = (np.stack(grads), eng.losses(3).copy(), eng.params.cpu().numpy().copy())
        eng2 = MiniBatchEngine(17, d, DEV, chain=chain, resident=False)      # Adam fused into the last launch
        eng2.load_params(w, W, fc)
        eng2.train_chunk(ch)
        np.testing.assert_array_equal(eng2.params.cpu().numpy(), res[chain][2])
    np.testing.assert_allclose(res[3][0], res[2][0], atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(res[3][1], res[2][1], atol=1e-6, rtol=0)
    np.testing.assert_allclose(res[3][2], res[2][2], atol=1e-6, rtol=0)


# ------------------------------------------------------------------ 3: every branch against float64
N_NODES = 20000


@functools.lru_cache(maxsize=None)
def _branch_graph():
    """Power-law graph on 20,000 nodes (ring: no isolated node) with hubs of more than 1,024 neighbours; the last node is made
    a pendant of node 0 (one neighbour: closed size 2)."""
    import scipy.sparse as sp
    n = N_NODES
    rowptr, col = synth.make_graph(n - 1, 400000, 9, kind="powerlaw", max_degree=1500)
    rows = np.concatenate([np.repeat(np.arange(n - 1), np.diff(rowptr)), [n - 1, 0]])
    cols = np.concatenate([col, [0, n - 1]])
    a = sp.csr_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n, n))
    a.sort_indices()
    rowptr, col = a.indptr.astype(np.int32), a.indices.astype(np.int32)
    deg = np.diff(rowptr)
    assert deg.min() >= 1 and deg[n - 1] == 1 and deg.max() + 1 > 1024
    return rowptr, col


@functools.lru_cache(maxsize=None)
def _branch_feat(f):
    return O.normalize_rows(synth.make_features(N_NODES, f, 9 + f)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _branch_batches():
    rowptr, col = _branch_graph()
    n = N_NODES
    deg = np.diff(rowptr)
    rng = np.random.default_rng(99)
    out = []
    # "mixed": 40 + 10 rows with the hub, the pendant, a duplicated node (both labels) and label-1 rows in the middle
    nodes = rng.choice(n - 1, 50, replace=False).astype(np.int64)
    lab = np.zeros(50, dtype=np.int64)
    lab[[5, 17, 18, 30]] = 1
    lab[44:] = 1
    nodes[2] = int(np.argmax(deg))                 # label 0, > 1,024 closed entries
    nodes[18] = int(np.argsort(deg)[-2])           # label 1: the second hub feeds the outlier generation
    nodes[9] = n - 1                               # closed size 2
    nodes[21] = nodes[20]                          # same node twice, same label
    nodes[30] = nodes[12]                          # ... and once with each label
    assert deg[nodes[2]] + 1 > 1024
    out.append(("mixed", nodes, lab))
    # "one1": exactly one label-1 row
    nodes = rng.choice(n - 1, 23, replace=False).astype(np.int64)
    lab = np.zeros(23, dtype=np.int64)
    lab[11] = 1
    out.append(("one1", nodes, lab))
    # "two": 1 + 1 rows
    out.append(("two", rng.choice(n - 1, 2, replace=False).astype(np.int64), np.array([0, 1], dtype=np.int64)))
    # "big": 333 + 77 rows
    nodes = rng.choice(n - 1, 410, replace=False).astype(np.int64)
    lab = np.zeros(410, dtype=np.int64)
    lab[rng.choice(410, 77, replace=False)] = 1
    out.append(("big", nodes, lab))
    return out


@functools.lru_cache(maxsize=None)
def _branch_aggs(f):
    """float64 and float32 aggregates of every batch at feature width f (computed once, shared by the widths)."""
    rowptr, col = _branch_graph()
    feat = _branch_feat(f)
    return [(O.aggregate_batch(rowptr, col, feat, nodes, True, dtype=np.float64), O.aggregate_batch(rowptr, col, feat, nodes, True))
            for _, nodes, _ in _branch_batches()]


@functools.lru_cache(maxsize=None)
def _branch_device(f):
    rowptr, col = _branch_graph()
    return DeviceGraph(rowptr, col, DEV), torch.from_numpy(_branch_feat(f)).to(DEV)


BRANCH_CASES = [(d, 17) for d in (65, 128, 129, 192, 255, 256)] + [(96, 1), (200, 9), (256, 70), (130, 128)]


@pytest.mark.parametrize("d,f", BRANCH_CASES, ids=[f"d{d}-f{f}" for d, f in BRANCH_CASES])
def test_wide_step_against_float64(d, f):
    """Teacher-forced steps (`loss_and_grads`, then `adam_step`) of every batch shape, from fresh state and from preloaded moments
    at step counter 10,000: losses, gradient, moments, parameters, transposed copies and step counter against the float64 step.
    Prints |device - float64|, |float32 oracle - float64| and their ratio per quantity."""
    graph, feat = _branch_device(f)
    cases = _branch_batches()
    aggs = _branch_aggs(f)
    ch = BatchChunk(graph, feat, d, max_batches=len(cases), rows_cap=512, ent_cap=16384, train=True, hop2="ldsw")
    ch.build([c[1] for c in cases], [c[2] for c in cases])
    assert int(ch.batch_max_row[0]) > 1024 and int(np.diff(ch.ent_ptr_host).min()) == 2
    torch.manual_seed(500 + d + f)
    params = (torch.nn.init.xavier_uniform_(torch.empty(1, d)), torch.nn.init.xavier_uniform_(torch.empty(d, f)),
              torch.nn.init.xavier_uniform_(torch.empty(d, d)))
    p0 = R.flat(*params)
    eng = MiniBatchEngine(f, d, DEV, lr=R.LR, weight_decay=R.WD)
    assert eng.wide and not eng.resident
    failures = []
    for b, (shape, nodes, lab) in enumerate(cases):
        agg64, agg32 = aggs[b]
        ref_loss, g = R.loss_and_grad64(agg64, lab, params)
        p32 = O.MiniParams.leaves(*[np.asarray(t) for t in params])
        t32 = O.batch_loss(p32, agg32, lab)
        t32[0].backward()
        l32 = np.array([t.item() for t in t32])
        g32 = np.concatenate([t.grad.numpy().reshape(-1) for t in p32.tensors()]).astype(np.float64)
        for t0 in (0, 10000):
            what = f"D={d} F={f} {shape} t0={t0}"
            m0, v0 = R.preload_state(g, p0, t0, 7 + t0)
            R.load_state(eng, params, m0, v0, t0)
            eng.loss_and_grads(ch, b, 0)
            got_l = eng.losses(1)[0].astype(np.float64)
            got_g = eng.grads.cpu().numpy().astype(np.float64)
            if t0 == 0:
                el, el32 = np.abs(got_l - ref_loss).max(), np.abs(l32 - ref_loss).max()
                rg, rg32 = (np.abs(got_g - g) / R.grad_bound(g)).max(), (np.abs(g32 - g) / R.grad_bound(g)).max()
                print(f"{what}: loss err device {el:.2e} f32-oracle {el32:.2e} ratio {el / max(el32, 1e-30):.1f} | "
                      f"grad err/bound device {rg:.3f} f32-oracle {rg32:.3f} ratio {rg / max(rg32, 1e-30):.1f} "
                      f"(|g|max {np.abs(g).max():.2e})")
            try:
                R.check_losses(got_l, ref_loss, what)
                R.check_grads(got_g, g, what)
                eng.adam_step()
                WR.check_step(eng, (p0, m0, v0, t0), g, what)
            except AssertionError as exc:
                failures.append(str(exc))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ 4: determinism, fusion, padding
def _poison(t, n_used=0):
    big = torch.full((int(t.numel() * 1.25) + 64,), float("nan"), dtype=t.dtype, device=t.device)
    big[:n_used] = t[:n_used]
    return big


@pytest.mark.parametrize("d", [128, 256])
def test_wide_chunk_is_deterministic_fused_and_reads_no_padding(d):
    f = 17
    graph, feat = _branch_device(f)
    cases = _branch_batches()
    batches, labels = [c[1] for c in cases], [c[2] for c in cases]
    torch.manual_seed(d)
    params = (torch.nn.init.xavier_uniform_(torch.empty(1, d)), torch.nn.init.xavier_uniform_(torch.empty(d, f)),
              torch.nn.init.xavier_uniform_(torch.empty(d, d)))
    k = len(batches)

    def snapshot(eng):
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy().view(np.int32) for x in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.loss_log[:8 * k])]

    def run(mode):
        ch = BatchChunk(graph, feat, d, max_batches=k, rows_cap=512, ent_cap=16384, train=True, hop2="ldsw")
        ch.build(batches, labels)
        eng = MiniBatchEngine(f, d, DEV, lr=R.LR, weight_decay=R.WD)
        eng.load_params(*params)
        eng.ensure_capacity(ch, k)
        if mode == "poisoned":
            # every scratch buffer 25 % larger and NaN all over (each is written before it is read); the parameter block, the
            # optimiser state and the plan's tables keep their content and get a NaN tail
            torch.cuda.synchronize()
            for name in ("h2", "dw_part", "loss_ws"):
                setattr(eng, name, _poison(getattr(eng, name)))
            for name in ("h1", "nbar", "gen", "dz", "coef_a", "coef_g"):
                setattr(ch, name, _poison(getattr(ch, name)))
            for name in ("exp_avg", "exp_avg_sq", "grads"):
                t = getattr(eng, name)
                setattr(eng, name, _poison(t, t.numel()))
            ch.x1 = _poison(ch.x1, ch.n_rows * f)
        if mode == "stepwise":
            for b in range(k):
                eng.loss_and_grads(ch, b, b)
                eng.adam_step()
        else:
            eng.train_chunk(ch)
        n = eng.n_train
        snap = snapshot(eng)
        return [snap[0], snap[1][:n], snap[2][:n], snap[3]]

    first = run("chunk")
    assert np.isfinite(first[0].view(np.float32)).all() and np.isfinite(first[3].view(np.float32)).all()
    for mode in ("chunk", "stepwise", "poisoned"):
        again = run(mode)
        for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "loss log"), first, again):
            assert np.array_equal(a, b), f"D={d}: {name} of the '{mode}' run differ from the first train_chunk run"


# ------------------------------------------------------------------ 5: public classes
def _small_synthetic():
    n = 3000
    rowptr, col = synth.make_graph(n, 30000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    return n, rowptr, col, feat, lab


def test_dgraph_trainer_at_emb_128():
    from ggad_amd.sampler import PyCompatRandom
    from ggad_amd.trainer import BatchSchedule, DGraphTrainer
    n, rowptr, col, feat_raw, lab = _small_synthetic()
    feat_np = O.normalize_rows(feat_raw).astype(np.float32)
    pool = np.flatnonzero(lab == 1)
    train = np.flatnonzero(lab == 0)[:1500]
    d = 128
    torch.manual_seed(6)
    params = (torch.nn.init.xavier_uniform_(torch.empty(1, d)), torch.nn.init.xavier_uniform_(torch.empty(d, 17)),
              torch.nn.init.xavier_uniform_(torch.empty(d, d)))
    runs = []
    for overlap in (False, True, False):
        graph = DeviceGraph(rowptr, col, DEV)
        feat = torch.from_numpy(feat_np).to(DEV)
        sched = BatchSchedule(train.copy(), pool.copy(), lab, 60, PyCompatRandom(72), n_pseudo=20, batches_per_epoch=6)
        tr = DGraphTrainer(graph, feat, d, sched, chunk_batches=6, overlap=overlap, prefetch=False)
        assert tr.engine.wide and tr.engine.resident is False
        tr.engine.load_params(*params)
        tr.run_steps(18)
        torch.cuda.synchronize()
        tr.check_exchange()
        assert tr.resident_fallbacks == 0 and tr.engine.xcd_ws is None
        runs.append((tr.engine.params.cpu().numpy().copy(), tr.engine.losses(6).copy()))
    assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][1]).all()
    for other in runs[1:]:
        np.testing.assert_array_equal(runs[0][0].view(np.int32), other[0].view(np.int32))
        np.testing.assert_array_equal(runs[0][1].view(np.int32), other[1].view(np.int32))


def test_model_handler_at_emb_128(tmp_path, capsys):
    """`ModelHandler(cfg).train()` with `emb_size: 128` on the small synthetic configuration of
    test_model_handler_sage_runs_end_to_end: launch chain, finite 5-tuple, checkpoint written and restored with the wide shapes,
    bit-reproducible from the seeds, validation scores equal to the oracle's `to_prob`."""
    from ggad_amd.model_handler import ModelHandler
    n, rowptr, col, feat, lab = _small_synthetic()
    losses, states = [], []
    for run in range(2):
        save = tmp_path / f"run{run}"
        cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab), seed=72, model="GCN",
                   multi_relation="GNN", emb_size=128, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=3,
                   valid_epochs=2, num_batches=6, n_pseudo=20, save_dir=str(save) + "/", test_ratio=0.67, device=0)
        random.seed(72)
        np.random.seed(72)
        torch.manual_seed(72)
        h = ModelHandler(cfg)
        res = h.train()
        eng = h.trainer.engine
        assert eng.D == 128 and eng.wide and eng.resident is False and h.trainer.resident_fallbacks == 0
        assert len(res) == 5 and all(np.isfinite(r) for r in res)
        assert h.last_epoch_losses.shape == (6, 4) and np.isfinite(h.last_epoch_losses).all()
        out = capsys.readouterr().out
        assert "Saving model" in out and "Restore model from epoch" in out
        files = glob.glob(os.path.join(str(save), "*", "synthetic_GCN.pkl"))
        assert len(files) == 1
        sd = torch.load(files[0])
        assert tuple(sd["weight"].shape) == (1, 128) and tuple(sd["enc.weight"].shape) == (128, 17)
        assert tuple(sd["enc.fc.weight"].shape) == (128, 128)
        now = h.model.state_dict()
        for key in ("weight", "enc.weight", "enc.fc.weight"):                  # the restored model is the checkpoint
            np.testing.assert_array_equal(now[key].cpu().numpy(), sd[key].cpu().numpy())
        losses.append(h.last_epoch_losses.copy())
        states.append({k: now[k].cpu().numpy().copy() for k in ("weight", "enc.weight", "enc.fc.weight")})
    np.testing.assert_array_equal(losses[0].view(np.int64), losses[1].view(np.int64))
    for key in states[0]:
        np.testing.assert_array_equal(states[0][key].view(np.int32), states[1][key].view(np.int32))
    # the validation sweep's scores: slices of 30 over 95 nodes, against the oracle on the restored weights
    from ggad_amd.sage_utils import score_nodes
    nodes = np.random.default_rng(1).choice(n, 95, replace=False).astype(np.int64)
    got = score_nodes(h.model, nodes, 30)
    p = O.MiniParams(*[torch.from_numpy(states[1][k]) for k in ("weight", "enc.weight", "enc.fc.weight")])
    feat_n = np.asarray(h.dataset["feat_data"], dtype=np.float32)
    want = np.concatenate([O.to_prob(p, rowptr, col, feat_n, nodes[s:s + 30]) for s in range(0, 95, 30)])
    np.testing.assert_allclose(got, want.reshape(-1), atol=2e-6, rtol=0)


# ------------------------------------------------------------------ 6: rejections
def test_what_stays_refused():
    from ggad_amd.exchange import OneShotExchange
    from ggad_amd.sampler import PyCompatRandom
    from ggad_amd.trainer import BatchSchedule, DGraphTrainer
    with pytest.raises(ValueError, match="256"):
        MiniBatchEngine(17, 257, DEV)
    with pytest.raises(ValueError, match="256"):
        MiniBatchEngine(17, 257, DEV, chain=3)
    with pytest.raises(ValueError, match="XCD-resident"):
        MiniBatchEngine(17, 128, DEV, resident=True)
    with pytest.raises(ValueError):
        MiniBatchEngine(17, 128, DEV, chain=1)
    with pytest.raises(ValueError):
        MiniBatchEngine(17, 64, DEV, chain=3, resident=True)
    n, rowptr, col, feat_raw, lab = _small_synthetic()
    graph = DeviceGraph(rowptr, col, DEV)
    feat = torch.from_numpy(O.normalize_rows(feat_raw).astype(np.float32)).to(DEV)
    sched = BatchSchedule(np.flatnonzero(lab == 0)[:600], np.flatnonzero(lab == 1), lab, 60, PyCompatRandom(72), n_pseudo=20,
                          batches_per_epoch=2)
    xchg = OneShotExchange(0, 1, 128 + 128 * 17 + 128 * 128, DEV)
    with pytest.raises(ValueError, match="one-shot"):
        DGraphTrainer(graph, feat, 128, sched, chunk_batches=2, exchange=xchg, overlap=False, prefetch=False)
