"""GPU parity tests of the DGraph mini-batch hot path (HIP kernels through the C-ABI) against
(a) the golden vectors captured from the imported reference and (b) the CPU oracle on seeded inputs.

Tolerances: fp32 path, summation order differs from the reference's dense mm -> 2e-6 absolute on
O(1) tensors, 1e-5 on losses, 2e-5 on weights after k Adam steps (tolerance stated per assert).
"""
import numpy as np
import pytest
import torch

import plan_counts_ref
from conftest import load_golden
from ggad_amd import synth

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd import _lib
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.minibatch import BatchChunk, MiniBatchEngine
from oracle import ggad_oracle as O

DEV = "cuda:0"


def _setup(g, train=True, max_batches=8, hop2="ldsw"):
    graph = DeviceGraph(g["rowptr"], g["col"], DEV)
    feat = torch.from_numpy(np.ascontiguousarray(g["feat"])).to(DEV)
    d = int(g["d"])
    ch = BatchChunk(graph, feat, d, max_batches=max_batches, rows_cap=64, ent_cap=64, train=train, hop2=hop2)
    return graph, feat, ch


@pytest.mark.parametrize("n", [1, 5, 2047, 2048, 2049, 100000, 1 << 20])
def test_exclusive_scan(n):
    lib = _lib.load()
    rng = np.random.default_rng(n)
    a = rng.integers(0, 50, size=n).astype(np.int32)
    x = torch.from_numpy(a).to(DEV)
    out = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.ggad_scan_workspace_elems(n)), dtype=torch.int32, device=DEV)
    _lib.call("ggad_exclusive_scan_i32", x.data_ptr(), out.data_ptr(), n, ws.data_ptr())
    ref = np.concatenate([[0], np.cumsum(a.astype(np.int64))])
    assert np.array_equal(out.cpu().numpy().astype(np.int64), ref)


def _check_plan_against_oracle(g, ch, batches, feat_np, atol=2e-6, range_option=0):
    rp, ci = g["rowptr"], g["col"]
    if ch.last_hop2 == "ldsw":      # the integers behind x2, exact (range_option: what ggad_mb_set_gather_options had at the build)
        plan_counts_ref.assert_plan_integers_exact(ch, rp, ci, batches, plan_counts_ref.effective_range_deg(range_option))
    ent_ptr = ch.ent_ptr[:ch.n_rows + 1].cpu().numpy()
    etot = int(ent_ptr[-1])
    assert np.array_equal(ent_ptr, ch.ent_ptr_host)          # host-side exact entry offsets == device scan
    ent_col = ch.ent_col[:etot].cpu().numpy()
    ent_own = ch.ent_own[:etot].cpu().numpy()
    ent_c1 = ch.ent_c1[:etot].cpu().numpy()
    ent_row = ch.ent_row[:etot].cpu().numpy()
    assert np.array_equal(ent_row, np.repeat(np.arange(ch.n_rows), np.diff(ent_ptr)))
    F = feat_np.shape[1]
    x1 = ch.x1[:ch.n_rows * F].view(-1, F).cpu().numpy()
    x2 = ch.x2[:etot * F].view(-1, F).cpu().numpy() if ch.train else None
    for b, nodes in enumerate(batches):
        r0, r1 = ch.batch_rows(b)
        agg = O.aggregate_batch(rp, ci, feat_np, nodes, ch.train)
        # entries: closed neighbourhoods, ascending
        assert np.array_equal(ent_ptr[r0:r1 + 1] - ent_ptr[r0], agg.ent_ptr)
        e0, e1 = ent_ptr[r0], ent_ptr[r1]
        assert np.array_equal(ent_col[e0:e1], agg.unique[agg.ent_pos])
        cnt = np.bincount(agg.ent_pos, minlength=len(agg.unique))
        assert np.array_equal(ent_c1[e0:e1], cnt[agg.ent_pos])
        np.testing.assert_allclose(x1[r0:r1], agg.to_feats, atol=atol, rtol=0, err_msg=f"x1 batch {b}")
        # owners: one per distinct column, inside this batch's entry range, same column
        own = ent_own[e0:e1]
        assert (own >= e0).all() and (own < e1).all()
        assert np.array_equal(ent_col[own], ent_col[e0:e1])
        owners = np.unique(own)
        assert len(owners) == len(agg.unique)
        assert (ent_own[owners] == owners).all()
        if ch.train:
            pos = np.searchsorted(agg.unique, ent_col[owners])
            np.testing.assert_allclose(x2[owners], agg.to_feats_neigh[pos], atol=atol, rtol=0, equal_nan=True,
                                       err_msg=f"x2 batch {b}")


@pytest.mark.parametrize("hop2", ["ldsw", "global"])
@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_plan_matches_golden_and_oracle(name, hop2):
    g = load_golden(name)
    graph, feat, ch = _setup(g, hop2=hop2)
    batches = [b for b in g["batches"]]
    ch.build(batches, [l for l in g["labels"]])
    torch.cuda.synchronize()
    _check_plan_against_oracle(g, ch, batches, g["feat"])
    # golden (reference) values for batch 0
    F = int(g["f"])
    r0, r1 = ch.batch_rows(0)
    x1 = ch.x1[:ch.n_rows * F].view(-1, F)[r0:r1].cpu().numpy()
    np.testing.assert_allclose(x1, g["agg_to_feats"], atol=2e-6, rtol=0)
    ent_ptr = ch.ent_ptr[:ch.n_rows + 1].cpu().numpy()
    etot = int(ent_ptr[-1])
    ent_col = ch.ent_col[:etot].cpu().numpy()
    ent_own = ch.ent_own[:etot].cpu().numpy()
    x2 = ch.x2[:etot * F].view(-1, F).cpu().numpy()
    e0, e1 = ent_ptr[r0], ent_ptr[r1]
    owner_of = {int(ent_col[e]): int(ent_own[e]) for e in range(e0, e1)}
    got = np.stack([x2[owner_of[int(u)]] for u in g["agg_unique"]])
    np.testing.assert_allclose(got, g["agg_to_feats_neigh"], atol=2e-6, rtol=0)
    # the plan leaves its counter slots clean
    torch.cuda.synchronize()
    assert ch.last_hop2 == hop2
    assert int(ch.cnt1.abs().sum()) == 0 and (ch.cnt2 is None or int(ch.cnt2.abs().sum()) == 0)


@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_loss_grads_adam_trajectory_vs_golden(name):
    g = load_golden(name)
    graph, feat, ch = _setup(g)
    eng = MiniBatchEngine(int(g["f"]), int(g["d"]), DEV, lr=1e-3, weight_decay=0.007)
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
            # forward tensors of batch 0 against the reference encoder outputs
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
    # transposed copies stay in sync with the trained block
    D, F = eng.D, eng.F
    nt = eng.n_train
    wt = eng.params[nt:nt + F * D].view(F, D).cpu().numpy()
    np.testing.assert_array_equal(wt, eng.enc_weight.cpu().numpy().T)
    fct = eng.params[nt + F * D:].view(D, D).cpu().numpy()
    np.testing.assert_array_equal(fct, eng.enc_fc_weight.cpu().numpy().T)


@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_resident_chunk_kernel_trajectory_vs_golden(name):
    """The DEFAULT hot path -- all optimiser steps of the chunk in the ONE launch resident on one XCD (`ggad_mb_train_chunk_xcd`,
    reference loop `src/model_handler.py:330-364`) -- directly against the reference's golden trajectory: per-step losses and the
    weights after the last Adam step (`final.*`), with the launch's own status word clean.  The resident kernel is built for the 17
    DGraph-Fin features: for any other width it is refused up front, and the default hot path is the launch chain of the chunk,
    held to the same trajectory."""
    g = load_golden(name)
    resident = int(g["f"]) == 17
    if not resident:
        with pytest.raises(ValueError):
            MiniBatchEngine(int(g["f"]), int(g["d"]), DEV, resident=True)
    graph, feat, ch = _setup(g)
    eng = MiniBatchEngine(int(g["f"]), int(g["d"]), DEV, lr=1e-3, weight_decay=0.007, resident=True if resident else None)
    eng.load_params(g["init.weight"], g["init.enc.weight"], g["init.enc.fc.weight"])
    batches = [b for b in g["batches"]]
    labels = [l for l in g["labels"]]
    ch.build(batches, labels)
    assert eng.resident == resident
    eng.train_chunk(ch)
    torch.cuda.synchronize()
    if resident:
        st = eng.xcd_status()
        assert st["error"] == 0 and st["workgroups"] == 32, st
    k = len(batches)
    assert int(eng.step_counter.item()) == k
    np.testing.assert_allclose(eng.losses(k), g["losses"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(eng.weight.cpu().numpy(), g["final.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(eng.enc_weight.cpu().numpy(), g["final.enc.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(eng.enc_fc_weight.cpu().numpy(), g["final.enc.fc.weight"], atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_to_prob_vs_golden(name):
    g = load_golden(name)
    graph, feat, ch = _setup(g, train=False, max_batches=4)
    eng = MiniBatchEngine(int(g["f"]), int(g["d"]), DEV)
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


def _random_case(n, n_entries, f, d, seed, nb, bsz, n_ano):
    rowptr, col = synth.make_graph(n, n_entries, seed, kind="powerlaw", max_degree=300, self_loop_frac=0.02)
    feat = O.normalize_rows(synth.make_features(n, f, seed)).astype(np.float32)
    rng = np.random.default_rng(seed + 3)
    batches, labels = [], []
    hub = int(np.argmax(np.diff(rowptr)))
    for b in range(nb):
        nodes = rng.choice(n, size=bsz, replace=False)
        if b == 0:
            nodes[3] = hub              # > 64 neighbours: exercises the 64-entry block loops
            nodes[7] = nodes[5]         # duplicate node in a batch (rows are per position)
        lab = np.zeros(bsz, dtype=np.int64)
        lab[bsz - n_ano:] = 1
        lab[rng.choice(bsz - n_ano, size=3, replace=False)] = 1
        batches.append(nodes)
        labels.append(lab)
    return dict(rowptr=rowptr, col=col, feat=feat, f=f, d=d), batches, labels


@pytest.mark.parametrize("hop2", ["ldsw", "global"])
@pytest.mark.parametrize("f,d", [(17, 64), (9, 32), (40, 64), (70, 48)])
def test_random_graph_vs_oracle(f, d, hop2):
    g, batches, labels = _random_case(n=20000, n_entries=160000, f=f, d=d, seed=21 + f, nb=3, bsz=200, n_ano=50)
    graph, feat, ch = _setup(g, max_batches=4, hop2=hop2)
    ch.build(batches, labels)
    torch.cuda.synchronize()
    _check_plan_against_oracle(g, ch, batches, g["feat"], atol=3e-6)
    # training steps vs the oracle's autograd + torch Adam
    torch.manual_seed(f)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, d))
    W = torch.nn.init.xavier_uniform_(torch.empty(d, f))
    fc = torch.nn.init.xavier_uniform_(torch.empty(d, d))
    eng = MiniBatchEngine(f, d, DEV, lr=1e-3, weight_decay=0.007)
    eng.load_params(w, W, fc)
    p = O.MiniParams(w.clone().requires_grad_(), W.clone().requires_grad_(), fc.clone().requires_grad_())
    opt = O.make_adam(p.tensors(), 1e-3, 0.007)
    ref_losses = []
    for b in range(len(batches)):
        eng.loss_and_grads(ch, b, b)
        agg = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], batches[b], True)
        opt.zero_grad()
        tot, cls, mar, rec = O.batch_loss(p, agg, labels[b])
        tot.backward()
        ref_losses.append([tot.item(), cls.item(), mar.item(), rec.item()])
        gr = eng.grads.cpu().numpy()
        ref = np.concatenate([t.grad.numpy().reshape(-1) for t in p.tensors()])
        np.testing.assert_allclose(gr, ref, atol=3e-6, rtol=2e-5, err_msg=f"grads batch {b}")
        eng.adam_step()
        opt.step()
    np.testing.assert_allclose(eng.losses(len(batches)), np.array(ref_losses), atol=1e-5, rtol=0)
    np.testing.assert_allclose(eng.enc_weight.cpu().numpy(), p.enc_weight.detach().numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(eng.enc_fc_weight.cpu().numpy(), p.enc_fc_weight.detach().numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(eng.weight.cpu().numpy(), p.weight.detach().numpy(), atol=1e-5, rtol=0)


@pytest.mark.parametrize("d,bsz,n_ano", [(64, 200, 50), (32, 333, 77), (48, 23, 5)])
def test_fused_forward_chain_equals_six_launch_chain(d, bsz, n_ano):
    """Chain 0 (projection fused into the forward-rows kernel) and the generic 6-launch chain 2 compute the same losses,
    gradients and Adam trajectory up to summation order; oracle check."""
    g, batches, labels = _random_case(n=12000, n_entries=150000, f=17, d=d, seed=31 + d, nb=3, bsz=bsz, n_ano=n_ano)
    torch.manual_seed(d)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, d))
    W = torch.nn.init.xavier_uniform_(torch.empty(d, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(d, d))
    res = {}
    for chain in (0, 2):
        graph, feat, ch = _setup(g, max_batches=3, hop2="ldsw")
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
    # fused forward vs project + fwd_rows: same fma order per entry, 8 instead of 16 partial sums per row
    np.testing.assert_allclose(res[0][0], res[2][0], atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(res[0][1], res[2][1], atol=1e-6, rtol=0)
    np.testing.assert_allclose(res[0][2], res[2][2], atol=1e-6, rtol=0)
    p = O.MiniParams(w.clone().requires_grad_(), W.clone().requires_grad_(), fc.clone().requires_grad_())
    agg = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], batches[0], True)
    tot, cls, mar, rec = O.batch_loss(p, agg, labels[0])
    tot.backward()
    ref = np.concatenate([t.grad.numpy().reshape(-1) for t in p.tensors()])
    np.testing.assert_allclose(res[2][0][0], ref, atol=3e-6, rtol=2e-5)
    np.testing.assert_allclose(res[2][1][0], [tot.item(), cls.item(), mar.item(), rec.item()], atol=1e-5, rtol=0)
    with pytest.raises(ValueError):
        MiniBatchEngine(17, d, DEV, chain=1)


@pytest.mark.parametrize("d,bsz,n_ano,hub", [(64, 200, 50, True), (64, 150, 50, False), (32, 333, 77, True), (48, 23, 5, False)])
def test_xcd_resident_chunk_equals_launch_chain(d, bsz, n_ano, hub):
    """The dense steps of a chunk as ONE launch resident on one XCD (`ggad_mb_train_chunk_xcd`) against the 5-launch chain:
    same per-entry fma order, same piece order per row, same loss reduction tree -> the FIRST step's losses are bit-equal when the
    chain takes its chunk-parallel forward (batch 0 holds the graph's hub row); gradients are grouped by piece instead of by flat stripes -> weights and
    later losses agree to fp32 round-off.  The launch is deterministic and reports its placement."""
    g, batches, labels = _random_case(n=12000, n_entries=150000, f=17, d=d, seed=131 + d + bsz, nb=6, bsz=bsz, n_ano=n_ano)
    torch.manual_seed(d)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, d))
    W = torch.nn.init.xavier_uniform_(torch.empty(d, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(d, d))
    res = {}
    for key, resident in (("chain", False), ("xcd", True), ("xcd2", True)):
        graph, feat, ch = _setup(g, max_batches=len(batches), hop2="ldsw")
        eng = MiniBatchEngine(17, d, DEV, resident=resident)
        assert eng.resident == resident
        eng.load_params(w, W, fc)
        ch.build(batches, labels)
        eng.train_chunk(ch)
        torch.cuda.synchronize()
        res[key] = (eng.params.cpu().numpy().copy(), eng.losses(len(batches)).copy(), eng.exp_avg.cpu().numpy().copy(),
                    int(eng.step_counter.item()), int(ch.batch_max_row[0]))
        if resident:
            st = eng.xcd_status()
            assert st["error"] == 0 and st["workgroups"] == 32, st
    assert res["xcd"][3] == res["chain"][3] == len(batches)
    np.testing.assert_array_equal(res["xcd"][0], res["xcd2"][0])                 # deterministic
    np.testing.assert_array_equal(res["xcd"][1], res["xcd2"][1])
    if hub and res["chain"][4] > 256:
        np.testing.assert_array_equal(res["xcd"][1][0], res["chain"][1][0])      # same forward / loss arithmetic
    np.testing.assert_allclose(res["xcd"][1], res["chain"][1], atol=2e-6, rtol=0)
    np.testing.assert_allclose(res["xcd"][0], res["chain"][0], atol=2e-6, rtol=0)
    np.testing.assert_allclose(res["xcd"][2], res["chain"][2], atol=2e-6, rtol=1e-4)
    # and the oracle on the first step
    p = O.MiniParams(w.clone().requires_grad_(), W.clone().requires_grad_(), fc.clone().requires_grad_())
    agg = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], batches[0], True)
    tot, cls, mar, rec = O.batch_loss(p, agg, labels[0])
    np.testing.assert_allclose(res["xcd"][1][0], [tot.item(), cls.item(), mar.item(), rec.item()], atol=1e-5, rtol=0)


def test_xcd_records_prepared_on_another_stream_equal_in_launch_records():
    """`MiniBatchEngine.xcd_prepare` (ggad_mb_xcd_prepare: the chunk kernel's records and x2 per entry, on the PLAN's stream, in a
    block owned by the chunk) against the records the launch builds itself: bit-identical weights, losses and optimiser state
    over two chunks, the second one re-using the record block; a prepare made for an earlier build is not used."""
    g, batches, labels = _random_case(n=12000, n_entries=150000, f=17, d=64, seed=77, nb=6, bsz=150, n_ano=40)
    torch.manual_seed(3)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, 64))
    W = torch.nn.init.xavier_uniform_(torch.empty(64, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(64, 64))
    side = torch.cuda.Stream()
    res = {}
    for key in ("in_launch", "prepared"):
        graph, feat, ch = _setup(g, max_batches=len(batches), hop2="ldsw")
        eng = MiniBatchEngine(17, 64, DEV, resident=True)
        eng.load_params(w, W, fc)
        for rep, (bs, ls) in enumerate(((batches, labels), (batches[::-1], labels[::-1]))):
            if key == "prepared":
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    ch.build(bs, ls)
                    eng.xcd_prepare(ch)             # (the very first call finds no workspace yet: that chunk's records are built in the launch)
                torch.cuda.current_stream().wait_stream(side)
                assert rep == 0 or ch.xcd_prepared[0] == ch.build_count
            else:
                ch.build(bs, ls)
            eng.train_chunk(ch, log_base=rep * len(bs))
            torch.cuda.synchronize()
            assert eng.xcd_status()["error"] == 0
        if key == "prepared":                        # a stale prepare (older build) must be ignored
            stale = ch.xcd_prepared
            ch.build(batches, labels)
            assert ch.xcd_prepared == stale and stale[0] != ch.build_count
            eng.train_chunk(ch, log_base=2 * len(batches))
        else:
            ch.build(batches, labels)
            eng.train_chunk(ch, log_base=2 * len(batches))
        torch.cuda.synchronize()
        res[key] = (eng.params.cpu().numpy().copy(), eng.losses(3 * len(batches)).copy(), eng.exp_avg_sq.cpu().numpy().copy())
    for a, b in zip(res["in_launch"], res["prepared"]):
        np.testing.assert_array_equal(a, b)


def test_rebuild_reuses_clean_slots():
    g, batches, labels = _random_case(n=5000, n_entries=30000, f=17, d=64, seed=4, nb=2, bsz=60, n_ano=10)
    graph, feat, ch = _setup(g, max_batches=2)
    for rep in range(3):
        ch.build(batches, labels)           # build() resets the previous plan first
        torch.cuda.synchronize()
        _check_plan_against_oracle(g, ch, batches, g["feat"], atol=3e-6)


def test_fused_adam_chunk_equals_stepwise():
    g, batches, labels = _random_case(n=8000, n_entries=60000, f=17, d=64, seed=9, nb=4, bsz=120, n_ano=30)
    torch.manual_seed(1)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, 64))
    W = torch.nn.init.xavier_uniform_(torch.empty(64, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(64, 64))
    outs = []
    for fused in (True, False):
        graph, feat, ch = _setup(g, max_batches=4)
        eng = MiniBatchEngine(17, 64, DEV, resident=False)
        eng.load_params(w, W, fc)
        ch.build(batches, labels)
        if fused:
            eng.train_chunk(ch)                        # Adam fused into the last launch of every step
        else:
            for b in range(4):
                eng.loss_and_grads(ch, b, b)
                eng.adam_step()
        outs.append((eng.params.cpu().numpy().copy(), eng.losses(4).copy()))
    for o in outs[1:]:        # side-stream planning (CU-masked or plain streams) and the sampler thread change nothing
        np.testing.assert_array_equal(outs[0][0], o[0])
        np.testing.assert_array_equal(outs[0][1], o[1])


def test_hop2_many_tiles_and_isolated_owner():
    """> 1 tile of 32,768 ids (n = 150k -> 5 tiles), hub rows spanning all tiles, and a node whose only neighbour is a
    self loop removed: deg-0 owners must come out NaN like the dense 0/0 row of the reference (quirk 3)."""
    n = 150000
    rowptr, col = synth.make_graph(n, 1500000, 5, kind="powerlaw", max_degree=1500)
    feat = O.normalize_rows(synth.make_features(n, 17, 5)).astype(np.float32)
    g = dict(rowptr=rowptr, col=col, feat=feat, f=17, d=64)
    rng = np.random.default_rng(1)
    hub = int(np.argmax(np.diff(rowptr)))
    batches, labels = [], []
    for b in range(3):
        nodes = rng.choice(n, size=200, replace=False)
        nodes[0] = hub
        lab = np.zeros(200, dtype=np.int64); lab[150:] = 1
        batches.append(nodes); labels.append(lab)
    for hop2 in ("ldsw", "global"):
        graph, ft, ch = _setup(g, max_batches=3, hop2=hop2)
        ch.build(batches, labels)
        torch.cuda.synchronize()
        assert ch.last_hop2 == hop2
        _check_plan_against_oracle(g, ch, batches, feat, atol=3e-6)


def test_ldsw_hop2_owner_slabs_and_padded_rows():
    """"ldsw" with a batch of > 6,144 entries (the LDS tables are walked in slabs), several 32,768-id tiles, and the
    128-byte padded feature rows the trainer hands it: x2 must equal the global-counter path bit for bit per owner
    up to summation order, and the oracle within 2e-5 (hub rows)."""
    n = 120000
    rowptr, col = synth.make_graph(n, 1200000, 9, kind="powerlaw", max_degree=3000)
    feat = O.normalize_rows(synth.make_features(n, 17, 9)).astype(np.float32)
    g = dict(rowptr=rowptr, col=col, feat=feat, f=17, d=64)
    rng = np.random.default_rng(3)
    order = np.argsort(-np.diff(rowptr))
    batches, labels = [], []
    for b in range(2):
        nodes = rng.choice(n, size=400, replace=False)
        nodes[:6] = order[b * 6:(b + 1) * 6]              # a few hubs: > 6,144 distinct owners in the batch
        lab = np.zeros(400, dtype=np.int64); lab[300:] = 1
        batches.append(nodes); labels.append(lab)
    graph = DeviceGraph(rowptr, col, DEV)
    table = torch.zeros(n, 32, dtype=torch.float32, device=DEV)
    table[:, :17] = torch.from_numpy(feat).to(DEV)
    ch = BatchChunk(graph, table, 64, max_batches=2, rows_cap=64, ent_cap=64, train=True, feat_dim=17, hop2="ldsw")
    ch.build(batches, labels)
    torch.cuda.synchronize()
    assert ch.last_hop2 == "ldsw"
    own = ch.owner_entries()
    per_batch = [int(((own >= ch.batch_ents(b)[0]) & (own < ch.batch_ents(b)[1])).sum()) for b in range(2)]
    assert max(per_batch) > _lib.load().ggad_mb_ldsw_max_owners() and sum(per_batch) == own.numel()
    _check_plan_against_oracle(g, ch, batches, feat, atol=2e-5)       # 3,000-neighbour hub rows: values up to ~2.5
    ref = BatchChunk(graph, torch.from_numpy(feat).to(DEV), 64, max_batches=2, rows_cap=64, ent_cap=64, train=True, hop2="global")
    ref.build(batches, labels)
    torch.cuda.synchronize()
    a = ch.x2.view(-1, 17)[own]
    b_ = ref.x2.view(-1, 17)[ref.ent_own[own].long()]      # owner election is a race: same column, maybe another entry
    assert torch.allclose(a, b_, rtol=1e-5, atol=1e-6, equal_nan=True)    # same sums, weights rounded once more or less
    ch.build(batches[:1], labels[:1])                       # rebuild: counters clean, same rows again
    torch.cuda.synchronize()
    _check_plan_against_oracle(g, ch, batches[:1], feat, atol=2e-5)


def test_ldsw_falls_back_to_global_counters():
    """A chunk the LDS-counting path cannot take (here: the host bound on the pair count is forced past 2^31) silently uses
    the device-atomic 2-hop kernels; same results, counters reset, and the next chunk goes back to "ldsw"."""
    g, batches, labels = _random_case(n=9000, n_entries=70000, f=17, d=64, seed=77, nb=3, bsz=120, n_ano=30)
    graph, feat, ch = _setup(g, max_batches=3, hop2="ldsw")
    bound = graph.node_pack_host                  # the table the native plan builder reads ((degree << 40) | pair bound): overwritten in place
    real = bound.copy()
    bound[:] = (real >> 40 << 40) | (1 << 27)
    ch.build(batches, labels)
    torch.cuda.synchronize()
    assert ch.last_hop2 == "global"
    _check_plan_against_oracle(g, ch, batches, g["feat"], atol=3e-6)
    assert int(ch.cnt1.abs().sum()) == 0 and int(ch.cnt2.abs().sum()) == 0       # the fallback cleans both counter families
    bound[:] = real
    ch.build(batches, labels)
    torch.cuda.synchronize()
    assert ch.last_hop2 == "ldsw"
    _check_plan_against_oracle(g, ch, batches, g["feat"], atol=3e-6)
    assert int(ch.cnt1.abs().sum()) == 0 and int(ch.cnt2.abs().sum()) == 0


@pytest.mark.parametrize("stride,mfma,ranges", [(17, False, False), (32, False, False), (32, True, False), (32, True, True), (17, False, True)])
def test_ldsw_node_major_gather_against_per_owner_kernel(stride, mfma, ranges):
    """A hub (900 neighbours) that is an owner in 11 of 12 batches (two groups: 8 + 3 occurrences), nodes shared by 2 / 4 batches
    and single occurrences: the node-major gather (work items = group x slice for owners up to 256 neighbours, group x id range
    above; partial sums combined in slice / range order) against the per-owner kernel (slices of 256 in order), node_head left
    clean, both against the oracle.  stride 32 + mfma = rows padded to one line, the matrix-core slice; otherwise the VALU slice;
    ranges = the id-range partition of the big owners (off by default).  All of them add the same products in different fixed
    orders: equal to 2e-6 relative; the default configuration (VALU slice, slices of 256) bit for bit."""
    n = 60000
    rowptr, col = synth.make_graph(n, 600000, 13, kind="powerlaw", max_degree=900)
    feat = O.normalize_rows(synth.make_features(n, 17, 13)).astype(np.float32)
    g = dict(rowptr=rowptr, col=col, feat=feat, f=17, d=64)
    rng = np.random.default_rng(5)
    order = np.argsort(-np.diff(rowptr))
    shared = rng.choice(n, size=40, replace=False)
    batches, labels = [], []
    for b in range(12):
        nodes = rng.choice(n, size=120, replace=False)
        if b != 4:
            nodes[0] = order[0]
        if b % 3 == 0:
            nodes[1:21] = shared[:20]                    # 4 batches
        if b in (1, 2):
            nodes[1:21] = shared[20:]                    # 2 batches
        lab = np.zeros(120, dtype=np.int64); lab[90:] = 1
        batches.append(nodes); labels.append(lab)
    graph = DeviceGraph(rowptr, col, DEV)
    ft = torch.zeros(n, stride, dtype=torch.float32, device=DEV)
    ft[:, :17] = torch.from_numpy(feat).to(DEV)
    outs = []
    from ggad_amd import _lib
    lib = _lib.load()
    for nm in (True, False):
        ch = BatchChunk(graph, ft, 64, max_batches=12, rows_cap=64, ent_cap=64, train=True, hop2="ldsw", node_major=nm, feat_dim=17)
        lib.ggad_mb_set_gather_options(0 if mfma else 2 ** 31 - 1, 256 if ranges else 0)
        try:
            ch.build(batches, labels)
            torch.cuda.synchronize()
        finally:
            lib.ggad_mb_set_gather_options(0, 0)
        assert ch.last_hop2 == "ldsw"
        own = ch.owner_entries()
        outs.append((ch.ent_col[own].clone(), torch.div(own, 1, rounding_mode="floor"), ch.x2.view(-1, 17)[own].clone()))
        if nm:
            assert int(ch.node_head.abs().sum()) == 0
            _check_plan_against_oracle(g, ch, batches, feat, atol=5e-6, range_option=256 if ranges else 0)
    # owner election is a race between duplicate entries, so compare per (batch, node): sort owners by (entry range, column)
    def keyed(cols, ents, x, chunk):
        b = torch.bucketize(ents, torch.as_tensor(chunk.ent_ptr_host[chunk.batch_ptr_host][1:], device=DEV), right=True)
        k = b * n + cols.long()
        o = torch.argsort(k)
        return k[o], x[o]
    ka, xa = keyed(*outs[0], ch)
    kb, xb = keyed(*outs[1], ch)
    assert torch.equal(ka, kb)
    torch.testing.assert_close(xa, xb, rtol=2e-6, atol=2e-7)
    if not mfma and not ranges:
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))


def test_tile_major_copy_of_col_and_the_pair_counts_read_from_it(monkeypatch):
    """Round 5 (`ggad_mb_tile_major`; reference op: the duplicate counts c' of src/graphsage.py:335-348): col_t = col reordered
    tile-major (a stable sort of the edges by the tile of the neighbour id: node order inside a tile, id order inside a segment),
    tile_start[u][t] = where segment (u, t) begins in it -- checked against numpy on the whole graph (10 tiles, hubs, empty
    segments) --, and the pair counting that reads col_t (a tile's workgroups in one residue class of blockIdx, with and without an
    XCD left out) gives x2 BIT-identical to the one that reads the rows of col."""
    from ggad_amd import _lib
    lib = _lib.load()
    n = 300000
    rowptr, col = synth.make_graph(n, 3000000, 21, kind="powerlaw", max_degree=1200)
    feat = O.normalize_rows(synth.make_features(n, 17, 21)).astype(np.float32)
    graph = DeviceGraph(rowptr, col, DEV)
    shift = int(lib.ggad_mb_ldsw_tile_shift())
    nt = (n + (1 << shift) - 1) >> shift
    assert nt >= 9
    off = graph.tile_offsets(shift).cpu().numpy().reshape(n, nt + 1)
    start, col_t = graph.tile_major(shift)
    start, col_t = start.cpu().numpy().reshape(n, nt + 1), col_t.cpu().numpy()
    tile_of = col.astype(np.int64) >> shift
    np.testing.assert_array_equal(col_t, col[np.argsort(tile_of, kind="stable")])
    lens = np.diff(off, axis=1).astype(np.int64)                          # [node][tile]
    base = np.concatenate(([0], np.cumsum(lens.sum(axis=0))))[:-1]
    want = base[None, :] + np.cumsum(lens, axis=0) - lens
    np.testing.assert_array_equal(start[:, :nt], want)
    assert (start[:, nt] == 0).all()

    rng = np.random.default_rng(8)
    order = np.argsort(-np.diff(rowptr))
    batches, labels = [], []
    for b in range(9):
        nodes = rng.choice(n, size=150, replace=False)
        nodes[:3] = order[b % 2:b % 2 + 3]                                # hubs in every batch
        lab = np.zeros(150, dtype=np.int64); lab[120:] = 1
        batches.append(nodes); labels.append(lab)
    ft = torch.zeros(n, 32, dtype=torch.float32, device=DEV)
    ft[:, :17] = torch.from_numpy(feat).to(DEV)

    def run(tile_major, skip):
        monkeypatch.setenv("GGAD_TILE_MAJOR", "1" if tile_major else "0")
        ch = BatchChunk(graph, ft, 64, max_batches=9, rows_cap=64, ent_cap=64, train=True, hop2="ldsw", feat_dim=17)
        ch.xcd_skip = skip
        ch.build(batches, labels)
        torch.cuda.synchronize()
        assert ch.last_hop2 == "ldsw" and (ch.plan.col_t is not None) == tile_major
        own = ch.owner_entries()
        b = torch.bucketize(own, torch.as_tensor(ch.ent_ptr_host[ch.batch_ptr_host][1:], device=DEV), right=True)
        k = b * n + ch.ent_col[own].long()
        o = torch.argsort(k)
        return k[o], ch.x2.view(-1, 17)[own][o].clone()
    k0, x0 = run(False, -1)
    assert torch.isfinite(x0).all() and float(x0.abs().sum()) > 0
    for skip in (-1, 0, 5):
        k1, x1 = run(True, skip)
        assert torch.equal(k0, k1)
        assert torch.equal(x0.view(torch.int32), x1.view(torch.int32))


def test_overlapped_chunks_equal_serial_execution():
    """Plan of chunk c+1 on a side stream while chunk c trains: same weights and losses as the one-stream order."""
    from ggad_amd.sampler import PyCompatRandom
    from ggad_amd.trainer import BatchSchedule, DGraphTrainer
    n = 30000
    rowptr, col = synth.make_graph(n, 300000, 2, kind="powerlaw", max_degree=400)
    feat_np = O.normalize_rows(synth.make_features(n, 17, 2)).astype(np.float32)
    labels = np.zeros(n, dtype=np.int64)
    pool = np.arange(1000, 1600)
    labels[pool] = 1
    train = np.arange(2000, 20000)
    torch.manual_seed(4)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, 64))
    W = torch.nn.init.xavier_uniform_(torch.empty(64, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(64, 64))
    outs = []
    # (None: the XCD-resident chunk kernel, plan kernels skipping its XCD when overlapped; 32: the launch chain on a cross-XCD
    #  stream pair -- the two families agree to round-off, each is bit-identical across its scheduling variants)
    for overlap, prefetch, dense_cus in ((False, False, None), (True, False, None), (True, False, 0), (False, True, None),
                                         (True, False, 24)):
        graph = DeviceGraph(rowptr, col, DEV)
        feat = torch.from_numpy(feat_np).to(DEV)
        sched = BatchSchedule(train.copy(), pool.copy(), labels, 60, PyCompatRandom(72), n_pseudo=20, batches_per_epoch=5)
        tr = DGraphTrainer(graph, feat, 64, sched, chunk_batches=3, overlap=overlap, prefetch=prefetch, dense_cus=dense_cus)
        assert tr.overlap == overlap
        tr.engine.load_params(w, W, fc)
        tr.run_steps(11)                                   # chunks of 3,3,3,2 -> both buffers reused
        torch.cuda.synchronize()
        outs.append((tr.engine.params.cpu().numpy().copy(), tr.engine.losses(11).copy()))
    for o in outs[1:4]:       # side-stream planning (CU-masked or plain streams) and the sampler thread change nothing
        np.testing.assert_array_equal(outs[0][0], o[0])
        np.testing.assert_array_equal(outs[0][1], o[1])
    np.testing.assert_allclose(outs[4][0], outs[0][0], atol=2e-6, rtol=0)      # 24 instead of 28 workgroups: another summation order
    chain = []
    for overlap, dense_cus in ((False, 32), (True, 32)):
        graph = DeviceGraph(rowptr, col, DEV)
        feat = torch.from_numpy(feat_np).to(DEV)
        sched = BatchSchedule(train.copy(), pool.copy(), labels, 60, PyCompatRandom(72), n_pseudo=20, batches_per_epoch=5)
        tr = DGraphTrainer(graph, feat, 64, sched, chunk_batches=3, overlap=overlap, prefetch=False, dense_cus=dense_cus)
        assert not tr.engine.resident
        tr.engine.load_params(w, W, fc)
        tr.run_steps(11)
        torch.cuda.synchronize()
        chain.append((tr.engine.params.cpu().numpy().copy(), tr.engine.losses(11).copy()))
    np.testing.assert_array_equal(chain[0][0], chain[1][0])
    np.testing.assert_array_equal(chain[0][1], chain[1][1])
    np.testing.assert_allclose(chain[0][0], outs[0][0], atol=2e-6, rtol=0)
    np.testing.assert_allclose(chain[0][1], outs[0][1], atol=2e-6, rtol=0)


@pytest.mark.parametrize("overlap", [False, True])
def test_resident_kernel_error_is_sticky_and_recovered_on_the_launch_chain(overlap):
    """A time-out of the XCD-resident chunk kernel (VERDICT r3 / ADVICE: its error word was reset by the next launch and aborted
    training): the error is STICKY across launches, and at the next check point the trainer restores the optimiser state of the
    previous check point, replays the recorded batches on the launch chain -- bit-identical to a trainer that never used the
    resident kernel -- and goes on without it."""
    import warnings
    from ggad_amd.sampler import PyCompatRandom
    from ggad_amd.trainer import BatchSchedule, DGraphTrainer
    n = 30000
    rowptr, col = synth.make_graph(n, 300000, 2, kind="powerlaw", max_degree=400)
    feat_np = O.normalize_rows(synth.make_features(n, 17, 2)).astype(np.float32)
    labels = np.zeros(n, dtype=np.int64)
    pool = np.arange(1000, 1600)
    labels[pool] = 1
    train = np.arange(2000, 20000)
    torch.manual_seed(4)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, 64))
    W = torch.nn.init.xavier_uniform_(torch.empty(64, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(64, 64))

    def make(resident):
        graph = DeviceGraph(rowptr, col, DEV)
        feat = torch.from_numpy(feat_np).to(DEV)
        sched = BatchSchedule(train.copy(), pool.copy(), labels, 60, PyCompatRandom(72), n_pseudo=20, batches_per_epoch=5)
        tr = DGraphTrainer(graph, feat, 64, sched, chunk_batches=3, overlap=overlap, prefetch=False,
                           dense_cus=None if resident else 32)
        assert bool(tr.engine.resident) == resident
        tr.engine.load_params(w, W, fc)
        return tr

    def state(tr):
        e = tr.engine
        return [t.cpu().numpy().copy() for t in (e.params, e.exp_avg, e.exp_avg_sq, e.step_counter)]

    chain = make(False)
    chain.run_steps(4)
    torch.cuda.synchronize()
    chain.check_exchange()
    mid = state(chain)
    chain.run_steps(7)
    chain.run_steps(5)
    torch.cuda.synchronize()
    want, want_losses = state(chain), chain.engine.losses(5).copy()

    tr = make(True)
    tr.run_steps(4)
    torch.cuda.synchronize()
    tr.check_exchange()                                      # a clean check point: the window starts again behind it
    assert tr.resident_fallbacks == 0 and tr.engine.xcd_status()["error"] == 0
    for a, b in zip(state(tr), mid):
        np.testing.assert_allclose(a, b, atol=2e-6, rtol=1e-4)
    tr.run_steps(7)
    torch.cuda.synchronize()
    tr.engine.set_resident_error(2)                          # as a chunk of this run whose registration wait timed out
    tr.engine.params.mul_(1.5)                               # ... and left the weights in some half-updated state
    tr.run_steps(5)                                          # the next launches clear their control block: the error must survive
    torch.cuda.synchronize()
    assert tr.engine.xcd_status()["error"] == 2
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr.check_exchange()
    assert any("replaying 12 optimiser steps" in str(c.message) for c in caught)
    assert tr.resident_fallbacks == 1 and not tr.engine.resident and tr.steps_done == 16
    assert tr.engine.xcd_status()["error"] == 0
    # the 4 resident steps before the check point stay (round-off away from the chain's); the 12 replayed ones ran on the chain
    for a, b in zip(state(tr), want):
        np.testing.assert_allclose(a, b, atol=4e-6, rtol=1e-4)
    np.testing.assert_allclose(tr.engine.losses(5), want_losses, atol=4e-6, rtol=0)
    # bit-exactness of the replay itself: a chain trainer started from the resident trainer's check-point state
    ref = make(False)
    ref.run_steps(4)                                         # (advances the sampler stream exactly as `tr` did)
    torch.cuda.synchronize()
    snap = tr._snap
    for dst, src in zip((ref.engine.params, ref.engine.exp_avg, ref.engine.exp_avg_sq, ref.engine.step_counter), snap):
        dst.copy_(src)
    ref.run_steps(7)
    ref.run_steps(5)
    torch.cuda.synchronize()
    for a, b in zip(state(tr), state(ref)):
        np.testing.assert_array_equal(a, b)
    tr.run_steps(3)                                          # and training goes on (launch chain)
    torch.cuda.synchronize()
    tr.check_exchange()
    assert int(tr.engine.step_counter.item()) == 19


def test_resident_error_of_the_last_launch_is_cleared_by_the_recovery_and_survives_workspace_growth():
    """(a) when the launch that failed is the LAST resident launch (one-chunk run, persistent placement error) the
    recovery must leave no error behind -- the next check point after the replay is clean, not a second raise; (b) an error
    recorded before the workspace is re-allocated (a larger chunk) is carried over; (c) a time-out in a window that is about
    to be rolled (more than _REPLAY_MAX_STEPS un-checked steps) is replayed, not swallowed by the fresh snapshot."""
    import warnings
    from ggad_amd.sampler import PyCompatRandom
    from ggad_amd.trainer import BatchSchedule, DGraphTrainer
    n = 30000
    rowptr, col = synth.make_graph(n, 300000, 2, kind="powerlaw", max_degree=400)
    feat_np = O.normalize_rows(synth.make_features(n, 17, 2)).astype(np.float32)
    labels = np.zeros(n, dtype=np.int64)
    pool = np.arange(1000, 1600)
    labels[pool] = 1
    train = np.arange(2000, 20000)
    torch.manual_seed(4)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, 64))
    W = torch.nn.init.xavier_uniform_(torch.empty(64, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(64, 64))

    def make(resident, chunk=3):
        graph = DeviceGraph(rowptr, col, DEV)
        feat = torch.from_numpy(feat_np).to(DEV)
        sched = BatchSchedule(train.copy(), pool.copy(), labels, 60, PyCompatRandom(72), n_pseudo=20, batches_per_epoch=5)
        tr = DGraphTrainer(graph, feat, 64, sched, chunk_batches=chunk, overlap=False, prefetch=False,
                           dense_cus=None if resident else 32)
        tr.engine.load_params(w, W, fc)
        return tr

    def state(tr):
        e = tr.engine
        return [t.cpu().numpy().copy() for t in (e.params, e.exp_avg, e.exp_avg_sq, e.step_counter)]

    chain = make(False)
    chain.run_steps(6)
    torch.cuda.synchronize()
    want = state(chain)

    # (a) the failed launch is the last resident one
    tr = make(True)
    tr.run_steps(6)
    torch.cuda.synchronize()
    tr.engine.set_resident_error(1)                          # both words, as a launch that timed out leaves them
    assert tr.engine.xcd_status()["error"] == 1
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr.check_exchange()
    assert any("replaying 6 optimiser steps" in str(c.message) for c in caught)
    assert tr.resident_fallbacks == 1 and not tr.engine.resident
    assert tr.engine.xcd_status()["error"] == 0
    for a, b in zip(state(tr), want):
        np.testing.assert_array_equal(a, b)                  # the whole run was replayed on the chain from the initial state
    tr.check_exchange()                                      # used to raise: `err` of the last launch was never cleared
    tr.run_steps(2)
    torch.cuda.synchronize()
    tr.check_exchange()
    assert int(tr.engine.step_counter.item()) == 8

    # (b) growth of the workspace keeps a recorded error
    tr = make(True, chunk=2)
    tr.run_steps(2)
    torch.cuda.synchronize()
    tr.engine.set_resident_error(2)
    old = tr.engine.xcd_ws
    tr.engine._xcd_rows = 0                                  # force the re-allocation path on the next chunk
    tr.engine._xcd_caps = (0, 0)
    tr.run_steps(2)
    torch.cuda.synchronize()
    assert tr.engine.xcd_ws is not old and tr.engine.xcd_status()["error"] == 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr.check_exchange()
    assert tr.resident_fallbacks == 1 and tr.engine.xcd_status()["error"] == 0

    # (c) a window that rolls over looks at the error word first
    tr = make(True)
    tr._REPLAY_MAX_STEPS = 4
    tr.run_steps(3)
    tr.run_steps(3)                                          # 6 > 4 un-checked steps: the next run would roll the window
    torch.cuda.synchronize()
    tr.engine.set_resident_error(1)
    tr.engine.params.mul_(1.5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr.run_steps(2)
    assert any("replaying 6 optimiser steps" in str(c.message) for c in caught)
    torch.cuda.synchronize()
    tr.check_exchange()
    assert tr.resident_fallbacks == 1 and int(tr.engine.step_counter.item()) == 8
    ref = make(False)
    ref.run_steps(3)
    ref.run_steps(3)
    ref.run_steps(2)
    torch.cuda.synchronize()
    for a, b in zip(state(tr), state(ref)):
        np.testing.assert_array_equal(a, b)


def test_chunk_parallel_forward_on_hub_batches_equals_six_launch_chain():
    """Batches with hub rows (> 256 entries) take the chunk-parallel forward of chain 0 (k_fwd_chunks + k_loss_pos_ck, relu
    mask recomputed in bwd_flat); chain 2 keeps project -> fwd_rows -> loss_pos.  Same losses / gradients / weights up to the
    order of the row sums; the row-chunk tables of the plan against their host statement."""
    g, batches, labels = _random_case(n=40000, n_entries=500000, f=17, d=64, seed=91, nb=5, bsz=200, n_ano=50)
    order = np.argsort(-np.diff(g["rowptr"]))
    for b in (0, 2, 3):
        batches[b][10:13] = order[3 * b:3 * b + 3]               # three hub rows each
    graph, feat, ch = _setup(g, max_batches=5, hop2="ldsw")
    ch.build(batches, labels)
    torch.cuda.synchronize()
    assert (ch.batch_max_row[[0, 2, 3]] > 256).all()
    # plan tables: pieces of <= 16 consecutive entries of one row
    cl = int(_lib.load().ggad_mb_chunk_len())
    r = np.diff(ch.ent_ptr_host[:ch.n_rows + 1])
    nck = (r + cl - 1) // cl
    ptr_ref = np.concatenate([[0], np.cumsum(nck)])
    assert np.array_equal(ch.row_ck_ptr[:ch.n_rows + 1].cpu().numpy(), ptr_ref)
    tot = int(ptr_ref[-1])
    rows_of = np.repeat(np.arange(ch.n_rows), nck)
    k_in = np.arange(tot) - ptr_ref[rows_of]
    e0 = ch.ent_ptr_host[rows_of] + k_in * cl
    cnt = np.minimum(cl, ch.ent_ptr_host[rows_of + 1] - e0)
    assert np.array_equal(ch.ck_e0[:tot].cpu().numpy(), e0)
    assert np.array_equal(ch.ck_rc[:tot].cpu().numpy(), (rows_of << 6) | cnt)
    torch.manual_seed(4)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, 64))
    W = torch.nn.init.xavier_uniform_(torch.empty(64, 17))
    fc = torch.nn.init.xavier_uniform_(torch.empty(64, 64))
    out = {}
    for chain in (0, 2):
        eng = MiniBatchEngine(17, 64, DEV, lr=1e-3, weight_decay=0.007, chain=chain)
        eng.load_params(w, W, fc)
        grads = []
        for b in range(5):
            eng.loss_and_grads(ch, b, b)
            grads.append(eng.grads.cpu().numpy().copy())
            eng.adam_step()
        torch.cuda.synchronize()
        out[chain] = (eng.losses(5).copy(), np.stack(grads), eng.params.cpu().numpy().copy())
    np.testing.assert_allclose(out[0][0], out[2][0], atol=1e-5, rtol=0)
    np.testing.assert_allclose(out[0][1], out[2][1], atol=3e-6, rtol=1e-4)
    np.testing.assert_allclose(out[0][2], out[2][2], atol=1e-5, rtol=0)
