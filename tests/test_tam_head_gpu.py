"""The opt-in fused TAM head (`ggad_amd/csrc/tam.hip`, `tam_utils.max_message_fused`, `train_cut(..., fused=True)`) on the MI355X:
against the vectors captured from the imported reference (`tests/golden/fullgraph_tam.npz`, the tolerances of `test_tam_gpu.py`),
against the float64 restatement (`tests/tam_head_fp64.py`) at every branch of the kernels, bit-reproducibility, captured against
eager epochs, and the refusals.

Branch bound, per quantity: the larger of 4 x the error of the composed path (`AffinityFn` + torch, float32 -- the code the fused
path stands beside; on a zero-padded embedding where h is no multiple of 4, which its SpMM does not take) against the same float64
values and 1e-6 x the quantity's largest magnitude.  Every ratio is printed."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import tam_head_fp64 as H

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_BRANCH = 4096


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "fullgraph_tam.npz"))


def _dev():
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return dev


def _raw(g):
    n = int(g["n"])
    a = sp.csr_matrix((np.ones(len(g["col"]), np.float32), g["col"], g["rowptr"]), shape=(n, n))
    r = (a + sp.eye(n)).tocsr()
    r.sort_indices()
    return r


def _cut_adj(g, cut, raw, dev):
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd import tam_utils as T
    n = int(g["n"])
    nz = g[f"cut{cut}.adj_nz"]
    pat = sp.csr_matrix((np.ones(len(nz), np.float32), (nz[:, 0], nz[:, 1])), shape=(n, n))
    pat.sort_indices()
    return FullGraphAdj(T.normalize_adj_tensor(pat), raw, dev)


def _model(g, cut, dev):
    from ggad_amd.model_tam import Model
    m = Model(int(g["f"]), int(g["n_h"]), "prelu", 2, "avg").to(dev)
    pre = f"init{cut}."
    m.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    return m


# ---------------------------------------------------------------------------------------------------- 1. golden, single step
@pytest.mark.parametrize("cut", [0, 1])
def test_golden_forward_affinity_loss_gradients(g, cut):
    """`test_tam_gpu.py::test_forward_affinity_loss_gradients` through `max_message_fused`, at that test's tolerances."""
    from ggad_amd import tam_utils as T
    dev = _dev()
    adj = _cut_adj(g, cut, _raw(g), dev)
    model = _model(g, cut, dev)
    feats = torch.from_numpy(g["features"])[None].to(dev)
    emb, f1, f2 = model.forward(feats, adj)
    loss, m, a = T.max_message_fused(emb[0], adj, g["normal_idx"])
    np.testing.assert_allclose(m.detach().cpu().numpy(), g[f"cut{cut}.message_norm"], atol=5e-6)
    np.testing.assert_allclose(a.detach().cpu().numpy(), g[f"cut{cut}.message"], atol=3e-6)
    assert abs(loss.item() - g[f"cut{cut}.losses"][0]) < 2e-4
    loss.backward()
    for k, p in model.named_parameters():
        gk = f"cut{cut}.grad." + k
        if gk in g.files:
            ref = g[gk]
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, atol=3e-5 * max(1.0, float(np.abs(ref).max())), err_msg=k)
        else:
            assert p.grad is None, k


# ---------------------------------------------------------------------------------------------------- 2. golden, trajectory
def _trajectory(g, use_graph, fused, cuts=(0, 1)):
    from ggad_amd import tam_utils as T
    from ggad_amd.fullgraph import FlatAdam
    dev = _dev()
    raw = _raw(g)
    feats = torch.from_numpy(g["features"])[None].to(dev)
    k_steps = len(g["cut0.losses"])
    out = []
    for cut in cuts:
        adj = _cut_adj(g, cut, raw, dev)
        model = _model(g, cut, dev)
        opt = FlatAdam(model.parameters(), lr=float(g["lr"]), weight_decay=0.0)
        opt.zero_grad()
        losses, msg = T.train_cut(model, opt, feats, adj, g["normal_idx"], k_steps, use_graph=use_graph, fused=fused)
        out.append((losses.cpu().numpy(), msg.detach().clone(), {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _fused_trajectory(use_graph):
    return _trajectory(np.load(os.path.join(HERE, "golden", "fullgraph_tam.npz")), use_graph, True)


@pytest.mark.parametrize("use_graph", [False, True])
def test_golden_trajectory_fused(g, use_graph):
    """`test_tam_gpu.py::test_trajectory_with_accumulating_gradients_and_scores` with `fused=True`, at that test's tolerances."""
    from ggad_amd.metrics import average_precision, roc_auc
    dev = _dev()
    msgs = []
    for cut, (losses, msg, sd) in enumerate(_fused_trajectory(use_graph)):
        np.testing.assert_allclose(losses, g[f"cut{cut}.losses"], atol=5e-4)
        np.testing.assert_allclose(msg.cpu().numpy(), g[f"cut{cut}.message_last"], atol=1e-5)
        for k in sd:
            np.testing.assert_allclose(sd[k], g[f"cut{cut}.final." + k], atol=3e-5, err_msg=k)
        msgs.append(msg)
    mean_msg = torch.stack(msgs).mean(0)
    score = 1 - (mean_msg - mean_msg.min()) / (mean_msg.max() - mean_msg.min())
    np.testing.assert_allclose(score.cpu().numpy(), g["score"], atol=2e-5)
    y = torch.from_numpy(g["ano"].astype(np.int64)).to(dev)
    assert abs(roc_auc(score, y) - float(g["auc"])) < 1e-6
    assert abs(average_precision(score, y) - float(g["ap"])) < 1e-6


# ---------------------------------------------------------------------------------------------------- 5. captured vs eager
def test_captured_epochs_equal_eager_epochs_bitwise():
    """Five epochs = two eager ones, the capture, three replays -- against five eager epochs: losses, message, weights bit for bit."""
    for (le, me, se), (lg, mg, sg) in zip(_fused_trajectory(False), _fused_trajectory(True)):
        assert len(le) == 5
        assert np.array_equal(le.view(np.int32), lg.view(np.int32))
        assert torch.equal(me.view(torch.int32), mg.view(torch.int32))
        for k in se:
            assert np.array_equal(se[k].view(np.int32), sg[k].view(np.int32)), k


# ---------------------------------------------------------------------------------------------------- 3. / 4. branches
def _hub_len():
    from ggad_amd import _lib
    return int(_lib.load().ggad_tam_head_hub_len())


@functools.lru_cache(maxsize=None)
def _graph(values: bool, n_diag_only: int):
    """Symmetric R over N_BRANCH nodes with rows of exactly 0, 1 (diagonal only: `n_diag_only` of them), 63 / 64 / 65, hub - 1 / hub /
    hub + 1 and 3,000 stored entries; every other ("ordinary") row has its diagonal, its two neighbours on a ring through the ordinary
    rows, a few random neighbours and its share of the special rows' entries.  `values`: off-diagonal values in [0.5, 2) (symmetric) and a diagonal of 2 instead of all ones.
    Returns (R as scipy CSR float32, dict name -> row)."""
    rng = np.random.default_rng(5 + int(values))
    n, hub = N_BRANCH, _hub_len()
    assert hub + 1 < 3000 < n - 64
    rows = {}
    nxt = iter(range(7, n, 97))                                        # the special rows, spread over the workgroups
    for k in range(3):
        rows[f"empty{k}"] = next(nxt)
    for k in range(n_diag_only):
        rows[f"diag{k}"] = next(nxt)
    lens = {"len63": 63, "len64": 64, "len65": 65, "hub-1": hub - 1, "hub": hub, "hub+1": hub + 1, "long": 3000}
    for k in lens:
        rows[k] = next(nxt)
    special = np.array(sorted(rows.values()))
    pool = np.setdiff1d(np.arange(n), special)
    ri, ci = [], []
    for k, ln in lens.items():                                          # diagonal + ln - 1 ordinary neighbours
        nb = rng.choice(pool, ln - 1, replace=False)
        ri.append(np.full(ln - 1, rows[k])); ci.append(nb)
    a = rng.choice(pool, 3 * n); b = rng.choice(pool, 3 * n)           # ordinary x ordinary
    keep = a != b
    ri.append(a[keep]); ci.append(b[keep])
    ri.append(pool[:-1]); ci.append(pool[1:])                           # a ring: no ordinary row is diagonal-only
    ri, ci = np.concatenate(ri), np.concatenate(ci)
    up = sp.coo_matrix((np.ones(len(ri)), (np.minimum(ri, ci), np.maximum(ri, ci))), shape=(n, n)).tocsr()
    up.sum_duplicates()
    up.data[:] = rng.uniform(0.5, 2.0, up.nnz) if values else 1.0
    diag = np.full(n, 2.0 if values else 1.0)
    diag[[rows[f"empty{k}"] for k in range(3)]] = 0.0
    R = (up + up.T + sp.diags(diag)).tocsr().astype(np.float32)
    R.eliminate_zeros()
    R.sort_indices()
    deg = np.diff(R.indptr)
    for k, ln in lens.items():
        assert deg[rows[k]] == ln, (k, deg[rows[k]])
    assert all(deg[rows[f"empty{k}"]] == 0 for k in range(3)) and all(deg[rows[f"diag{k}"]] == 1 for k in range(n_diag_only))
    assert (deg > hub).sum() == 2 and abs(R - R.T).nnz == 0
    return R, rows


@functools.lru_cache(maxsize=None)
def _adj(values: bool, n_diag_only: int):
    from ggad_amd.fullgraph import FullGraphAdj
    R, rows = _graph(values, n_diag_only)
    return FullGraphAdj(R, R, _dev())                                  # (the normalised adjacency is not used by the head)


# (name, h, values, kind): kind "normal" = signed random embedding with three zero rows, one diagonal-only row (the unique maximum);
# "ties" = the exact-tie construction; "k1" = an index list of one node; "h1" = "normal" for h = 1, where e_hat is a sign and a row
# whose neighbours all share its sign has a = 1 up to rounding: the signs alternate along the ring and the values are not all ones,
# so that every row but the diagonal-only one stays clearly below 1 and the float32 and float64 tie sets agree
CASES = ([("h1", 1, True, "h1")] + [(f"h{h}", h, False, "normal") for h in (32, 63, 64, 65, 128, 255, 256)]
         + [("values_h128", 128, True, "normal"), ("values_h200", 200, True, "normal"), ("k1_h64", 64, False, "k1"),
            ("ties_h3", 3, True, "ties"), ("ties_h64", 64, False, "ties"), ("ties_h130", 130, True, "ties")])


def _inputs(h, values, kind):
    n_diag = 3 if kind == "ties" else 1
    R, rows = _graph(values, n_diag)
    n = R.shape[0]
    rng = np.random.default_rng(1000 + h)
    special = set(rows.values())
    ordinary = np.array([i for i in range(n) if i not in special])
    zero_rows = ordinary[[5, 1500, -3]]
    if kind == "ties":
        # 0 <= a <= 1: three zero rows and the three entry-less rows give a = 0 exactly; the three diagonal-only rows hold a power of
        # two times a basis vector, a = 1 exactly; every other row averages cosines of distinct positive vectors, clearly inside (0, 1)
        e = rng.uniform(0.2, 1.0, (n, h)).astype(np.float32)
        for k in range(3):
            e[rows[f"diag{k}"]] = 0.0
            e[rows[f"diag{k}"], k % h] = 2.0 ** (k - 1)
    elif kind == "h1":
        e = (0.1 + np.abs(rng.standard_normal((n, h)))).astype(np.float32)
        e[ordinary[1::2]] *= -1.0
    else:
        e = rng.standard_normal((n, h)).astype(np.float32)
    e[zero_rows] = 0.0
    return R, rows, e, zero_rows


@functools.lru_cache(maxsize=None)
def _run_case(name):
    """Everything one branch case needs, computed once: the float64 values, the composed path, the fused path through autograd, and two
    direct launches of the entry points into NaN-filled outputs."""
    from ggad_amd import tam_utils as T
    from ggad_amd import _lib
    from ggad_amd._lib import ptr
    _, h, values, kind = next(c for c in CASES if c[0] == name)
    dev = _dev()
    R, rows, e, zero_rows = _inputs(h, values, kind)
    n = R.shape[0]
    adj = _adj(values, 3 if kind == "ties" else 1)
    r_inv = adj.r_inv_host
    pre = H.tam_head_fp64(R.indptr, R.indices, R.data, r_inv, e, [0])
    rng = np.random.default_rng(77)
    if kind == "k1":
        idx = np.array([int(rng.integers(n))], dtype=np.int64)
    else:                                                              # repeats, and the arg-min / arg-max nodes among them
        base = rng.choice(n, 300)
        idx = np.concatenate([base, base[:40], [int(pre["a"].argmin()), int(pre["a"].argmax()), int(pre["a"].argmax())],
                              list(zero_rows[:2]), [rows["long"], rows["empty0"]]]).astype(np.int64)
    ref = H.tam_head_fp64(R.indptr, R.indices, R.data, r_inv, e, idx)

    def composed():
        # the composed path's SpMM takes widths that are multiples of 4 only: at the other widths it runs on the embedding padded with
        # zero columns, which changes no norm, no dot product and no gradient of the first h columns
        hp = (h + 3) // 4 * 4
        x = torch.zeros(n, hp, device=dev)
        x[:, :h] = torch.from_numpy(e).to(dev)
        x.requires_grad_(True)
        loss, m = T.max_message(x, adj, idx)
        a = T.inference(x.detach(), adj)
        loss.backward()
        return dict(a=a, lo=a.min(), hi=a.max(), loss=loss.detach(), m=m.detach(), d_emb=x.grad[:, :h])

    def fused():
        x = torch.from_numpy(e).to(dev).requires_grad_(True)
        loss, m, a = T.max_message_fused(x, adj, idx)
        loss.backward()
        return dict(a=a, lo=a.min(), hi=a.max(), loss=loss.detach(), m=m, d_emb=x.grad)

    res = {}
    for tag, fn in (("composed", composed), ("fused", fused)):
        res[tag] = {k: v.detach().double().cpu().numpy() for k, v in fn().items()}

    # two direct launches into NaN-filled outputs
    head = T.tam_head(adj, idx)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(e).to(dev)
    gup = torch.ones((), dtype=torch.float32, device=dev)
    raw_runs = []
    for _ in range(2):
        o = {k: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
             for k, s in (("a", (n,)), ("scal", (8,)), ("m", (n,)), ("inv", (n,)), ("d_emb", (n, h)))}
        ws = head.workspace(h)
        rc = lib.ggad_tam_head_fwd_f32(*head._args(x), ptr(o["a"]), ptr(o["scal"]), ptr(o["m"]), ptr(o["inv"]), ptr(ws), st)
        assert rc == 0
        rc = lib.ggad_tam_head_bwd_f32(*head._args(x), ptr(o["a"]), ptr(o["scal"]), ptr(o["inv"]), ptr(gup), ptr(o["d_emb"]), ptr(ws), st)
        assert rc == 0
        torch.cuda.synchronize()
        raw_runs.append({k: v.cpu().numpy() for k, v in o.items()})
        assert int(ws.view(torch.int32)[:64 * ((1 + head.n_hub + 63) // 64)].abs().max().item()) == 0      # the ticket words are back at zero
    return dict(ref=ref, res=res, raw=raw_runs, idx=idx, rows=rows, zero_rows=zero_rows, kind=kind)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_branches_against_float64(name):
    c = _run_case(name)
    ref, res = c["ref"], c["res"]
    worst = 0.0
    for q in ("a", "lo", "hi", "loss", "m", "d_emb"):
        want = np.asarray(ref[q], dtype=np.float64)
        err_c = float(np.abs(res["composed"][q] - want).max())
        err_f = float(np.abs(res["fused"][q] - want).max())
        bound = max(4.0 * err_c, 1e-6 * float(np.abs(want).max()))
        ratio = err_f / bound if bound > 0 else (0.0 if err_f == 0 else float("inf"))
        print(f"{name:12s} {q:6s} max|ref| {np.abs(want).max():.4e}  composed err {err_c:.3e}  fused err {err_f:.3e}  bound {bound:.3e}  "
              f"ratio {ratio:.3f}")
        worst = max(worst, ratio)
    print(f"{name:12s} worst ratio {worst:.3f}")
    scal = c["raw"][0]["scal"]
    print(f"{name:12s} n_lo {scal[3]:.0f} (fp64 {ref['n_lo']})  n_hi {scal[4]:.0f} (fp64 {ref['n_hi']})")
    assert worst <= 1.0
    a0 = c["raw"][0]["a"]
    assert scal[1] == a0.min() and scal[2] == a0.max() and scal[3] == (a0 == a0.min()).sum() and scal[4] == (a0 == a0.max()).sum()
    assert np.float64(scal[0]) == res["fused"]["loss"]
    if c["kind"] == "ties":
        assert ref["n_lo"] == 6 and ref["n_hi"] == 3               # (three zero-norm rows + three rows without entries)
        assert ref["lo"] == 0.0 and ref["hi"] == 1.0
        assert scal[1] == 0.0 and scal[2] == 1.0 and scal[3] == ref["n_lo"] and scal[4] == ref["n_hi"]
        tie = np.concatenate([np.nonzero(ref["a"] == 0.0)[0], np.nonzero(ref["a"] == 1.0)[0]])
        inside = np.setdiff1d(np.arange(len(ref["a"])), tie)
        assert ref["a"][inside].min() > 0.01 and ref["a"][inside].max() < 0.999
        assert np.array_equal(c["raw"][0]["a"] == 0.0, ref["a"] == 0.0) and np.array_equal(c["raw"][0]["a"] == 1.0, ref["a"] == 1.0)
    # rows of zero norm and rows without entries: affinity 0 exactly; zero-norm rows get no gradient
    assert np.all(c["raw"][0]["a"][c["zero_rows"]] == 0.0) and np.all(c["raw"][0]["d_emb"][c["zero_rows"]] == 0.0)
    assert all(c["raw"][0]["a"][c["rows"][f"empty{k}"]] == 0.0 for k in range(3))


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_branches_reproducible_and_fully_written(name):
    c = _run_case(name)
    r0, r1 = c["raw"]
    for k in r0:
        assert not np.isnan(r0[k]).any(), k                            # every element written (the outputs were NaN-filled)
        assert np.array_equal(r0[k].view(np.int32), r1[k].view(np.int32)), k
    # the autograd wrapper runs the same launches
    assert np.array_equal(r0["a"].astype(np.float64), c["res"]["fused"]["a"])
    assert np.array_equal(r0["d_emb"].astype(np.float64), c["res"]["fused"]["d_emb"])


# ---------------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("h", [0, 257])
def test_unsupported_width_launches_nothing(h):
    from ggad_amd import _lib
    from ggad_amd import tam_utils as T
    from ggad_amd._lib import ptr
    dev = _dev()
    adj = _adj(False, 1)
    head = T.tam_head(adj, np.arange(10))
    n = head.n
    lib = _lib.load()
    assert lib.ggad_tam_head_supported(n, h) == 0 and lib.ggad_tam_head_supported(n, 256) == 1 and lib.ggad_tam_head_max_dim() == 256
    x = torch.ones(n, max(h, 1), dtype=torch.float32, device=dev)
    poison = 12345.0
    o = {k: torch.full(s, poison, dtype=torch.float32, device=dev)
         for k, s in (("a", (n,)), ("scal", (8,)), ("m", (n,)), ("inv", (n,)), ("d_emb", (n, max(h, 1))))}
    ws = torch.zeros(int(lib.ggad_tam_head_workspace_elems(n, 256, head.n_hub, head.n_pieces)), dtype=torch.float32, device=dev)
    gup = torch.ones((), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    args = list(head._args(x))
    args[8] = h
    assert lib.ggad_tam_head_fwd_f32(*args, ptr(o["a"]), ptr(o["scal"]), ptr(o["m"]), ptr(o["inv"]), ptr(ws), st) == _lib.GGAD_E_UNSUPPORTED
    assert lib.ggad_tam_head_bwd_f32(*args, ptr(o["a"]), ptr(o["scal"]), ptr(o["inv"]), ptr(gup), ptr(o["d_emb"]), ptr(ws),
                                     st) == _lib.GGAD_E_UNSUPPORTED
    torch.cuda.synchronize()
    for k, v in o.items():
        assert bool((v == poison).all()), k
    assert bool((ws == 0).all())
    if h > 0:
        with pytest.raises(ValueError):
            T.max_message_fused(torch.ones(n, h, device=dev), adj, np.arange(10))


def test_asymmetric_raw_adjacency_is_refused():
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd import tam_utils as T
    dev = _dev()
    n = 50
    sym = (sp.random(n, n, density=0.1, random_state=np.random.RandomState(3), format="csr") > 0).astype(np.float32)
    sym = ((sym + sym.T) > 0).astype(np.float32) + sp.eye(n, dtype=np.float32)
    pat = sym.tolil(); pat[3, 40] = 1.0; pat[40, 3] = 0.0                 # pattern
    val = sym.tolil(); val[3, 40] = 1.0; val[40, 3] = 0.5                 # values only
    emb = torch.randn(n, 8, device=dev)
    for bad in (pat, val):
        adj = FullGraphAdj(sym.tocsr(), bad.tocsr(), dev)
        with pytest.raises(ValueError, match="composed path"):
            T.max_message_fused(emb, adj, np.arange(5))
        with pytest.raises(ValueError, match="composed path"):
            T.TamHead(adj, np.arange(5))
        T.max_message(emb, adj, np.arange(5))                              # the composed path takes it
    torch.cuda.synchronize()


def test_default_train_cut_is_the_composed_path_bitwise(g):
    """`fused=False` (the default) = a direct loop over the composed functions, bit for bit."""
    from ggad_amd import tam_utils as T
    from ggad_amd.fullgraph import FlatAdam
    dev = _dev()
    (l_def, m_def, s_def), = _trajectory(g, False, False, cuts=(0,))
    adj = _cut_adj(g, 0, _raw(g), dev)
    model = _model(g, 0, dev)
    feats = torch.from_numpy(g["features"])[None].to(dev)
    opt = FlatAdam(model.parameters(), lr=float(g["lr"]), weight_decay=0.0)
    opt.zero_grad()
    idx = torch.as_tensor(np.asarray(g["normal_idx"], dtype=np.int64), device=dev)
    model.train()
    losses = []
    for _ in range(len(l_def)):
        node_emb, _, _ = model.forward(feats, adj)
        loss, _ = T.max_message(node_emb[0], adj, idx)
        with torch.no_grad():
            msg = T.inference(node_emb[0].detach(), adj)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    assert np.array_equal(torch.stack(losses).cpu().numpy().view(np.int32), l_def.view(np.int32))
    assert torch.equal(msg.view(torch.int32), m_def.view(torch.int32))
    for k, v in model.state_dict().items():
        assert np.array_equal(v.detach().cpu().numpy().view(np.int32), s_def[k].view(np.int32)), k
