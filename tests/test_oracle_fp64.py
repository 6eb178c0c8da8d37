"""The float64 mode of the mini-batch oracle (`aggregate_batch` / `encoder_forward` / `batch_loss` with dtype=np.float64, and
`adam_f64`): the high-precision reference the HIP kernels are compared with in tests/test_resident_step_gpu.py.

It must reproduce the reference's captured vectors (tests/golden/minibatch_*.npz, float32 captures) within the tolerances the
float32 oracle meets in tests/test_oracle_golden.py: the float64 result is the truth, the captures carry fp32 round-off.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import ggad_oracle as O

TOL = 2e-6


def _leaves(g, prefix, dtype):
    return O.MiniParams.leaves(g[prefix + ".weight"], g[prefix + ".enc.weight"], g[prefix + ".enc.fc.weight"], dtype)


@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_float64_oracle_reproduces_the_reference_vectors(name):
    g = load_golden(name)
    p = _leaves(g, "init", torch.float64)
    n = len(p.tensors())
    m = [np.zeros(t.shape) for t in p.tensors()]
    v = [np.zeros(t.shape) for t in p.tensors()]
    for step, (nodes, lab) in enumerate(zip(g["batches"], g["labels"])):
        agg = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True, dtype=np.float64)
        assert agg.to_feats.dtype == np.float64 and agg.to_feats_neigh.dtype == np.float64
        if step == 0:
            np.testing.assert_allclose(agg.to_feats, g["agg_to_feats"], atol=TOL, rtol=0)
            perm = np.searchsorted(agg.unique, g["agg_unique"])
            np.testing.assert_allclose(agg.to_feats_neigh[perm], g["agg_to_feats_neigh"], atol=TOL, rtol=0)
            with torch.no_grad():
                ca, nbar, af, afn = O.encoder_forward(p, agg, lab, True, dtype=np.float64)
            for t in (ca, nbar, af, afn):
                assert t.dtype == torch.float64
            np.testing.assert_allclose(ca.numpy(), g["enc_combined_all"], atol=TOL, rtol=0)
            np.testing.assert_allclose(nbar.numpy(), g["enc_to_feats_neigh"], atol=TOL, rtol=0)
            np.testing.assert_allclose(af.numpy(), g["enc_anomaly_feat"], atol=TOL, rtol=0)
            np.testing.assert_allclose(afn.numpy(), g["enc_anomaly_feat_new"], atol=TOL, rtol=0)
        for t in p.tensors():
            t.grad = None
        terms = O.batch_loss(p, agg, lab, dtype=torch.float64)
        assert all(x.dtype == torch.float64 for x in terms)
        terms[0].backward()
        np.testing.assert_allclose([x.item() for x in terms], g["losses"][step], atol=5e-6, rtol=0)
        grads = [t.grad.numpy() for t in p.tensors()]
        if step == 0:
            for key, gr in zip(("grad.weight", "grad.enc.weight", "grad.enc.fc.weight"), grads):
                np.testing.assert_allclose(gr, g[key], atol=TOL, rtol=1e-5, err_msg=key)
        with torch.no_grad():
            for k in range(n):
                pk, m[k], v[k] = O.adam_f64(p.tensors()[k].numpy(), m[k], v[k], grads[k], step + 1)
                p.tensors()[k].copy_(torch.from_numpy(pk))
        if step == 0:
            np.testing.assert_allclose(p.weight.detach().numpy(), g["step1.weight"], atol=TOL, rtol=0)
            np.testing.assert_allclose(p.enc_weight.detach().numpy(), g["step1.enc.weight"], atol=TOL, rtol=0)
            np.testing.assert_allclose(p.enc_fc_weight.detach().numpy(), g["step1.enc.fc.weight"], atol=TOL, rtol=0)
    np.testing.assert_allclose(p.weight.detach().numpy(), g["final.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(p.enc_weight.detach().numpy(), g["final.enc.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(p.enc_fc_weight.detach().numpy(), g["final.enc.fc.weight"], atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_float32_default_is_unchanged_and_float64_is_closer_to_itself(name):
    """dtype=np.float32 (the default) is the same computation as before the dtype argument existed: bit-identical aggregates
    and losses; the float64 result differs from it by fp32 round-off only."""
    g = load_golden(name)
    nodes, lab = g["batches"][0], g["labels"][0]
    a32 = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True)
    b32 = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True, dtype=np.float32)
    assert a32.to_feats.dtype == np.float32
    assert np.array_equal(a32.to_feats, b32.to_feats) and np.array_equal(a32.to_feats_neigh, b32.to_feats_neigh)
    l32 = [x.item() for x in O.batch_loss(_leaves(g, "init", torch.float32), a32, lab)]
    l32b = [x.item() for x in O.batch_loss(_leaves(g, "init", torch.float32), a32, lab, dtype=torch.float32)]
    assert l32 == l32b
    a64 = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True, dtype=np.float64)
    l64 = [x.item() for x in O.batch_loss(_leaves(g, "init", torch.float64), a64, lab, dtype=np.float64)]
    np.testing.assert_allclose(l64, l32, atol=2e-6, rtol=0)
    assert np.abs(a64.to_feats - a32.to_feats).max() > 0          # really a different precision


@pytest.mark.parametrize("step", [1, 2, 10000])
def test_adam_f64_is_torch_adam_in_float64(step):
    """`adam_f64` against torch.optim.Adam itself on float64 tensors (lr 1e-3, weight decay 0.007, betas (0.9, 0.999), eps
    1e-8), from fresh state (step 1) and from preloaded moments at later step numbers: equal to float64 round-off."""
    rng = np.random.default_rng(step)
    p0 = rng.standard_normal((7, 5))
    g = rng.standard_normal((7, 5)) * 1e-3
    m0 = np.zeros_like(p0) if step == 1 else rng.standard_normal((7, 5)) * 1e-3
    v0 = np.zeros_like(p0) if step == 1 else rng.random((7, 5)) * 1e-5
    t = torch.tensor(p0, requires_grad=True)
    opt = torch.optim.Adam([t], lr=1e-3, weight_decay=0.007)
    if step > 1:
        opt.state[t] = dict(step=torch.tensor(float(step - 1), dtype=torch.float32), exp_avg=torch.tensor(m0),
                            exp_avg_sq=torch.tensor(v0))
    t.grad = torch.tensor(g)
    opt.step()
    p1, m1, v1 = O.adam_f64(p0, m0, v0, g, step)
    np.testing.assert_allclose(p1, t.detach().numpy(), atol=1e-15, rtol=1e-13)
    np.testing.assert_allclose(m1, opt.state[t]["exp_avg"].numpy(), atol=1e-18, rtol=1e-13)
    np.testing.assert_allclose(v1, opt.state[t]["exp_avg_sq"].numpy(), atol=1e-20, rtol=1e-13)


# ------------------------------------------------------------------ full graph
def _full_setup(g):
    adjn_rp, adjn_ci, adjn_va, raw_rp, raw_ci, raw_va = O.normalize_adj(g["rowptr"], g["col"])
    return (adjn_rp, adjn_ci, adjn_va), (raw_rp, raw_ci, raw_va)


def _full_leaves(g, dtype):
    return {k: torch.tensor(g["init." + k], dtype=dtype, requires_grad=True) for k in O.FULL_PARAM_ORDER}


@pytest.mark.parametrize("by_column", [False, True])
@pytest.mark.parametrize("name", ["fullgraph_reddit_like.npz", "fullgraph_amazon_like.npz"])
def test_float64_full_graph_oracle_reproduces_the_reference_vectors(name, by_column):
    """`full_forward` / `full_loss` with dtype=float64 (parameters, features, adjacency values, noise and autograd in float64)
    against the reference's float32 captures: forward tensors and affinity of step 0, the four losses of every step, the step-0
    gradients -- at the tolerances the float32 oracle meets in tests/test_oracle_golden.py.  The trajectory is driven by `adam_f64`."""
    g = load_golden(name)
    adjn, raw = _full_setup(g)
    P = _full_leaves(g, torch.float64)
    m = {k: np.zeros(P[k].shape) for k in P}
    v = {k: np.zeros(P[k].shape) for k in P}
    feat = torch.from_numpy(g["features"])
    abn, nrm = g["abn_idx"], g["normal_idx"]
    mean, var, h = float(g["mean"]), float(g["var"]), int(g["n_h"])
    for step in range(len(g["losses"])):
        torch.manual_seed(1000 + step)
        noise = torch.randn(1, len(abn), h)[0] * var + mean               # the float32 draw of `model.py:143`, widened
        for t in P.values():
            t.grad = None
        emb, comb, logits, con, eab = O.full_forward(P, feat, adjn, abn, nrm, noise, True, dtype=torch.float64)
        total, lm, lb, lr, aff = O.full_loss(emb, logits, con, eab, raw, abn, nrm, by_column=by_column, dtype=torch.float64)
        for t in (emb, comb, logits, con, eab, total, lm, lb, lr, aff):
            assert t.dtype == torch.float64
        total.backward()
        np.testing.assert_allclose([total.item(), lm.item(), lb.item(), lr.item()], g["losses"][step], atol=1e-5)
        if step == 0:
            np.testing.assert_allclose(emb.detach().numpy(), g["emb"], atol=TOL)
            np.testing.assert_allclose(comb.detach().numpy(), g["emb_combine"], atol=TOL)
            np.testing.assert_allclose(logits.detach().numpy(), g["logits"], atol=TOL)
            np.testing.assert_allclose(con.detach().numpy(), g["emb_con"], atol=TOL)
            np.testing.assert_allclose(eab.detach().numpy(), g["emb_abnormal"], atol=TOL)
            np.testing.assert_allclose(aff.detach().numpy(), g["affinity"], atol=TOL)
            for k in O.FULL_PARAM_ORDER:
                assert P[k].grad.dtype == torch.float64
                np.testing.assert_allclose(P[k].grad.numpy(), g["grad." + k], atol=3e-6, rtol=1e-4, err_msg=k)
        with torch.no_grad():
            for k in O.FULL_PARAM_ORDER:
                pk, m[k], v[k] = O.adam_f64(P[k].numpy(), m[k], v[k], P[k].grad.numpy(), step + 1, weight_decay=0.0)
                P[k].copy_(torch.from_numpy(pk))
    for k in O.FULL_PARAM_ORDER:
        np.testing.assert_allclose(P[k].detach().numpy(), g["final." + k], atol=3e-5, err_msg=k)


def _degenerate_loss_case(seed, n=60, h=12):
    """A small loss block with every degenerate shape at once: a zero embedding row inside J (node 3) and outside it (node 50,
    a neighbour of node 4 in J), a node of J whose raw column sums to 0 (node 7: no `+ I`, no stored entry in its column), a
    node in both lists (node 5), an index list that is not sorted."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    a = sp.random(n, n, density=0.1, random_state=seed, format="lil", dtype=np.float64)
    a = ((a + a.T) > 0).astype(np.float64).tolil()
    a[4, 50] = a[50, 4] = 1.0
    a[:, 7] = 0.0                                                          # nothing points at node 7 ...
    eye = np.ones(n)
    eye[7] = 0.0                                                           # ... not even itself
    raw = (a.tocsr() + sp.diags(eye)).tocsr()
    raw.eliminate_zeros()
    raw.sort_indices()
    assert raw.sum(0).A1[7] == 0 and raw[4, 50] == 1
    emb = rng.standard_normal((n, h))
    emb[3] = 0.0
    emb[50] = 0.0
    nrm = [3, 4, 7, 20, 5, 11, 30, 2]
    abn = [40, 5, 41]
    return (raw.indptr, raw.indices, raw.data), emb, rng.standard_normal(len(nrm) + len(abn)), rng.standard_normal((len(abn), h)), \
        rng.standard_normal((len(abn), h)), abn, nrm


@pytest.mark.parametrize("name", ["fullgraph_reddit_like.npz", "fullgraph_amazon_like.npz", "degenerate"])
def test_float64_affinity_forms_agree(name):
    """Per-edge and by-column association of the affinity in float64: the same sums in another order, equal to 1e-12 of scale
    in the four losses, the affinity and every input gradient -- on the captured graphs and on a case with zero embedding rows,
    a zero column sum and a node in both lists."""
    if name == "degenerate":
        raw, emb, logits, con, eab, abn, nrm = _degenerate_loss_case(5)
    else:
        g = load_golden(name)
        _, raw = _full_setup(g)
        rng = np.random.default_rng(1)
        abn, nrm = g["abn_idx"], g["normal_idx"]
        emb = rng.standard_normal((int(g["n"]), int(g["n_h"])))
        logits = rng.standard_normal(len(abn) + len(nrm))
        con, eab = rng.standard_normal((len(abn), emb.shape[1])), rng.standard_normal((len(abn), emb.shape[1]))
    res = []
    for by_column in (False, True):
        ins = [torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (emb, logits, con, eab)]
        out = O.full_loss(*ins, raw, abn, nrm, by_column=by_column, dtype=torch.float64)
        out[0].backward(gradient=torch.tensor(1.7, dtype=torch.float64))
        res.append([o.detach() for o in out] + [t.grad for t in ins])
    for i, (a, b) in enumerate(zip(*res)):
        assert a.dtype == torch.float64
        nan = torch.isnan(a)
        assert torch.equal(nan, torch.isnan(b)) and bool(torch.isfinite(a[~nan]).all())
        assert bool(nan.any()) == (name == "degenerate" and i == 5)       # only d emb of the degenerate case, see below
        assert float((a - b)[~nan].abs().max()) <= 1e-12 * max(float(b[~nan].abs().max()), 1.0)
    if name == "degenerate":
        aff, d_emb = res[0][4], res[0][5]
        assert float(aff[7]) == 0.0 and float(aff[3]) == 0.0              # zero column sum / zero row: affinity exactly 0
        # what torch's autograd returns for a zero embedding row, in either precision and either form: NaN on that whole row and
        # nowhere else -- `where(isinf(inv), 0, inv)` hands `pow(norm, -1)` a zero gradient, whose own derivative -norm^-2 is
        # -inf there: 0 * inf.  (The reference's `run.py:177-181` is these very ops.  The HIP kernels return 0 on such a row:
        # tests/test_fullgraph_branches_gpu.py states the difference.)
        assert torch.nonzero(torch.isnan(d_emb).any(1)).flatten().tolist() == [3, 50]
        assert bool(torch.isnan(d_emb[[3, 50]]).all())
        assert float(res[0][1]) > 1e-3                                    # the hinge is active: the gradients above are not all 0


@pytest.mark.parametrize("name", ["fullgraph_reddit_like.npz", "fullgraph_amazon_like.npz"])
def test_float32_full_graph_default_is_unchanged(name):
    """dtype=torch.float32 is the default and the same computation as the call without the argument: bit-identical tensors,
    losses and gradients through both signatures (`_spmm`, `full_forward`, both forms of `full_loss`); float64 differs from it by
    float32 round-off only, and really is another precision.  (One thread: the per-edge form's backward scatters with atomic
    float adds when torch runs it on several, so its gradients are not bit-reproducible from run to run with ANY signature.)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _float32_default_is_unchanged(load_golden(name))
    finally:
        torch.set_num_threads(threads)


def _float32_default_is_unchanged(g):
    adjn, raw = _full_setup(g)
    feat = torch.from_numpy(g["features"])
    abn, nrm = g["abn_idx"], g["normal_idx"]
    torch.manual_seed(1000)
    noise = torch.randn(1, len(abn), int(g["n_h"]))[0] * float(g["var"]) + float(g["mean"])
    x = torch.from_numpy(g["features"])
    assert torch.equal(O._spmm(*adjn, x), O._spmm(*adjn, x, dtype=torch.float32)) and O._spmm(*adjn, x).dtype == torch.float32
    runs = []
    for kw in ({}, {"dtype": torch.float32}, {"dtype": torch.float64}):
        for by_column in (False, True):
            P = _full_leaves(g, kw.get("dtype", torch.float32))
            fw = O.full_forward(P, feat, adjn, abn, nrm, noise, True, **kw)
            ev = O.full_forward(P, feat, adjn, abn, nrm, noise, False, **kw)
            ls = O.full_loss(fw[0], fw[2], fw[3], fw[4], raw, abn, nrm, by_column=by_column, **kw)
            ls[0].backward()
            runs.append([t.detach() for t in fw] + [ev[2].detach(), ev[4].detach()] + [t.detach() for t in ls]
                        + [P[k].grad for k in O.FULL_PARAM_ORDER])
    for a, b in zip(runs[0] + runs[1], runs[2] + runs[3]):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    differs = False
    for a, b in zip(runs[0] + runs[1], runs[4] + runs[5]):
        assert b.dtype == torch.float64
        assert float((a.double() - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1.0)
        differs = differs or float((a.double() - b).abs().max()) > 0
    assert differs


# ------------------------------------------------------------------ the cases of tests/test_fullgraph_branches_gpu.py, CPU side
def _d32(kind, name):
    """(distances of the float32 oracle from the float64 oracle per tensor, classes) for one case of tests/fullgraph_fp64.py;
    the float64 run takes the ReLU / PReLU branches of the float32 run, as the GPU comparison takes the kernels'."""
    import fullgraph_fp64 as C
    if kind == "loss":
        c = C.loss_case(name)
        r64 = C.loss_reference(c, torch.float64)
        C.check_loss_reference(c, r64)                                    # hinge beyond +-1e-3, NaN only where stated
        if c["refused"]:
            return {}, C.LOSS_CLASSES                                     # (never compared: the library refuses the width)
        r32 = C.loss_reference(c, torch.float32)
        for k in C.LOSS_CLASSES:
            assert np.array_equal(np.isnan(r32[k]), np.isnan(r64[k])), (name, k)
        return {k: C.distance(r32[k], r64[k]) for k in C.LOSS_CLASSES}, C.LOSS_CLASSES
    out, classes = {}, None
    for all_five in ((False, True) if kind in ("head", "model") else (None,)):
        if kind == "gcn":
            c = C.gcn_case(name)
            r32 = C.gcn_reference(c, torch.float32)
            masks = C.masks_of(r32["pre"])
            r64 = C.gcn_reference(c, torch.float64, masks["z"])
            classes = {k: v for k, v in C.GCN_CLASSES.items() if k in r64}
        else:
            c = C.head_case(name)
            fn = C.head_reference if kind == "head" else C.model_reference
            r32 = fn(c, torch.float32, all_five)
            masks = C.masks_of(r32["pre"])
            r64 = fn(c, torch.float64, all_five, masks)
            classes = C.HEAD_CLASSES if kind == "head" else C.MODEL_CLASSES
        C.check_masks(masks, r64["pre"])                                  # kinks: within 1e-6 of scale on <= 0.1 % of a tensor
        for k in classes:
            out[k] = max(out.get(k, 0.0), C.distance(r32[k], r64[k]))
    return out, classes


def _branch_cases():
    import fullgraph_fp64 as C
    return ([("loss", k) for k in C.LOSS_CASES] + [("head", k) for k in C.HEAD_CASES] + [("model", k) for k in C.HEAD_CASES]
            + [("gcn", k) for k in C.GCN_CASES])


def test_branch_cases_float32_oracle_is_within_a_quarter_of_every_gpu_bound():
    """The tolerances of tests/test_fullgraph_branches_gpu.py are 4 x the largest distance of the float32 oracle from the float64
    oracle per tensor class over ITS cases (the figures in that module's docstring).  Here that distance is measured again for
    every case and tensor and held against the recorded bound as a band -- torch's float32 sums move a little with the host's
    vector width and thread count, so: 3 x d32 <= bound for every tensor, bound < 8 x the largest d32 of its class (derived from
    the measurement, not padded).  The bounds stay inside what the full-size test grants, and each case's preconditions (hinge
    side, NaN placement, kink shares) hold on the references alone."""
    import fullgraph_fp64 as C
    assert max(C.BOUND[k] for k in (C.FWD, C.LOSS, C.AFF, C.MODEL_FWD)) <= 2e-5
    assert max(C.BOUND[k] for k in (C.DGRAD, C.WGRAD, C.MODEL_WGRAD)) <= 1e-4
    worst = {}
    for kind, name in _branch_cases():
        ds, classes = _d32(kind, name)
        for k, d in ds.items():
            assert d <= C.BOUND[classes[k]] / 3, (kind, name, k, d)
            if d > worst.get(classes[k], (0.0,))[0]:
                worst[classes[k]] = (d, kind, name, k)
    for cls, w in sorted(worst.items()):
        print(f"d32 {cls}: {w[0]:.3e} at {w[1:]} -> bound {C.BOUND[cls]:.1e}")
        assert w[0] > C.BOUND[cls] / 8                                    # the bound is derived from the measurement, not padded
