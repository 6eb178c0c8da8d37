"""Cases and float64 references of tests/test_fullgraph_branches_gpu.py  --  TEST INFRASTRUCTURE.

Every case is built on the host from a seed (scipy.sparse + `synth.make_graph`, numpy's generator) as float32 arrays; the
references are `oracle/ggad_oracle.py`'s `full_loss` / `full_head` / `gcn_layer` run by torch on the CPU in a given dtype on those
very arrays.  Nothing here touches the GPU, so tests/test_oracle_fp64.py can run the float32 oracle against the float64 oracle on
every case (`d32`, the distance the GPU bounds are derived from) and check the preconditions the GPU comparison relies on.
"""
import numpy as np
import scipy.sparse as sp
import torch

from ggad_amd import synth
from oracle import ggad_oracle as O

G_TOTAL = 1.7                     # upstream gradient of the loss (not 1: a dropped factor shows)
MARGIN = 0.7

# the tensor classes of the tolerance table (module docstring of tests/test_fullgraph_branches_gpu.py)
FWD, LOSS, AFF, DGRAD, WGRAD = "forward", "losses", "affinity", "data_grad", "weight_grad"
MODEL_FWD, MODEL_WGRAD = "model_forward", "model_weight_grad"    # through `Model`: four layers deep, classes of their own
# GPU bound per class = 4 x the largest d32 of the class over all cases (tests/test_oracle_fp64.py asserts d32 <= bound / 4), never
# above what tests/test_fullgraph_fullsize_gpu.py grants (2e-5 forward / losses, 1e-4 gradients)
BOUND = {FWD: 4.6e-6, LOSS: 4.7e-7, AFF: 1.3e-6, DGRAD: 2.7e-6, WGRAD: 7.4e-6, MODEL_FWD: 1.1e-5, MODEL_WGRAD: 1.2e-5}


def distance(got, ref):
    """max |got - ref| / max |ref| over the entries where ref is finite (NaN placement is compared by the caller); an all-zero
    reference demands exact zeros."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    scale = np.abs(ref[ok]).max()
    err = np.abs(got[ok] - ref[ok]).max()
    if scale == 0.0:
        return 0.0 if err == 0.0 else np.inf
    return float(err / scale)


def _graph(n, deg, seed):
    rowptr, col = synth.make_graph(n, deg * n, seed, kind="er")
    return synth.csr_to_scipy(rowptr, col, n).astype(np.float64).tolil()


def _normalize(a):
    """D^-1/2 A D^-1/2 with D = row sums, inf -> 0 (`utils.py:47-54`), float64."""
    a = sp.csr_matrix(a)
    d = np.asarray(a.sum(1)).reshape(-1)
    with np.errstate(divide="ignore"):
        di = np.power(d, -0.5)
    di[np.isinf(di)] = 0.0
    dm = sp.diags(di)
    return a.dot(dm).transpose().dot(dm).tocsr()


def _csr(m):
    m = sp.csr_matrix(m).copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def csr_triple(m):
    return m.indptr.astype(np.int64), m.indices.astype(np.int64), m.data.astype(np.float64)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ================================================================================================ loss block
def _loss(n, h, nn, na, seed=0, deg=8, **kw):
    return dict(n=n, h=h, nn=nn, na=na, seed=seed, deg=deg, **kw)


LOSS_CASES = {}
for _h in (4, 64, 68, 300, 512, 516, 576, 1024, 1028):          # both forms of k_rownorm_bwd_add, G = 16 ... 1, h > 1024: launch sequence
    LOSS_CASES[f"H{_h}"] = _loss(400, _h, 90, 13, seed=_h)
for _h in (1, 63, 65, 301):                                     # not a multiple of 4: the products refuse them (asserted as refusals)
    LOSS_CASES[f"H{_h}"] = _loss(400, _h, 90, 13, seed=_h, refused=True)
for _l in (2, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193, 20011):      # L = Nn + A around LD_ROWS and the 8 x 1024 trips
    _na = 1 if _l == 2 else 5
    LOSS_CASES[f"L{_l}"] = _loss(max(40, _l + _l // 5), 64, _l - _na, _na, seed=_l)
LOSS_CASES["L8193_H300"] = _loss(10000, 300, 8193 - 40, 40, seed=3)
for _a in (1, 7, 8, 9, 31, 32, 33, 844, 3000):                  # REC_ROWS = 8, four partial rows per workgroup, nb_part < G ... >> 8 G
    for _h in (64, 300):
        LOSS_CASES[f"A{_a}_H{_h}"] = _loss(4000, _h, 50, _a, seed=_a + _h)
LOSS_CASES["hinge_inactive_H300"] = _loss(3000, 300, 700, 90, seed=11, inactive=True)
LOSS_CASES["hinge_inactive_H576"] = _loss(600, 576, 100, 20, seed=12, inactive=True)
LOSS_CASES["degenerate_rows_H300"] = _loss(6000, 300, 300, 40, seed=13, degenerate=True)
LOSS_CASES["degenerate_rows_H576"] = _loss(6000, 576, 300, 40, seed=14, degenerate=True)
LOSS_CASES["node_in_both_lists"] = _loss(3000, 300, 700, 90, seed=15, overlap=True)
LOSS_CASES["node_in_both_lists_H576"] = _loss(600, 576, 100, 20, seed=16, overlap=True)
LOSS_CASES["duplicate_in_normal_list"] = _loss(3000, 300, 700, 90, seed=17, duplicate=True)
LOSS_CASES["zero_difference_column"] = _loss(3000, 300, 700, 90, seed=18, zero_column=True)


def loss_case(name):
    """Inputs of one `GgadLossFn` case (a name of LOSS_CASES, or the parameters of a case of the caller's own as `_loss` returns
    them): adjacency (scipy), float32 operands, index lists, and what the case expects."""
    p = LOSS_CASES[name] if isinstance(name, str) else name
    n, h, nn, na = p["n"], p["h"], p["nn"], p["na"]
    rng = np.random.default_rng(1000 + p["seed"])
    a = _graph(n, p["deg"], p["seed"])
    perm = rng.permutation(n)
    nrm, abn = perm[:nn].tolist(), perm[nn:nn + na].tolist()
    rest = perm[nn + na:]
    eye = np.ones(n)
    emb = rng.standard_normal((n, h))
    zero_rows = []
    if p.get("inactive"):
        # normal nodes align with their neighbours, the abnormal ones oppose theirs: mean_n - mean_a > 0.7
        sign = np.ones(n)
        sign[abn] = -1.0
        u = rng.standard_normal(h)
        emb = sign[:, None] * u[None, :] + 0.05 * rng.standard_normal((n, h))
    if p.get("degenerate"):
        hub = nrm[0]                                            # a hub column that thousands of rows touch
        targets = rng.choice(rest, size=4000, replace=False)
        a[hub, targets] = 1.0
        a[targets, hub] = 1.0
        zj, zo, zn, owner, lone = nrm[1], int(rest[0]), int(rest[1]), nrm[2], nrm[3]
        a[owner, zn] = a[zn, owner] = 1.0                       # zn: a zero row outside J that is a neighbour of a row in J
        zero_rows = [zj, zo, zn]                                # inside J, outside J, neighbour of J
        emb[zero_rows] = 0.0
        a[:, lone] = 0.0                                        # a node of J whose raw column sums to 0: nothing points at it,
        a[lone, :] = 0.0
        eye[lone] = 0.0                                         # not even itself (no + I for that node)
    if p.get("overlap"):
        abn[0] = nrm[3]
    if p.get("duplicate"):
        nrm[5] = nrm[4]                                         # adjacent positions: two waves of one workgroup take them
    a = _csr(a)
    raw = _csr(a + sp.diags(eye))
    adj_norm = _csr(_normalize(a) + sp.diags(eye))
    con, eab = rng.standard_normal((na, h)), rng.standard_normal((na, h))
    if p.get("zero_column"):
        eab[:, 7] = con[:, 7]
    c = dict(name=name, n=n, h=h, nrm=nrm, abn=abn, adj_norm=adj_norm, raw=raw, emb=_f32(emb), logits=_f32(rng.standard_normal(nn + na)),
             con=_f32(con), eab=_f32(eab), zero_rows=zero_rows, inactive=bool(p.get("inactive")), refused=bool(p.get("refused")),
             nan_column=7 if p.get("zero_column") else None, seg_unique=not p.get("duplicate"),
             distinct=not (p.get("overlap") or p.get("duplicate")))
    if p.get("degenerate"):
        c.update(hub=hub, lone=lone)
    return c


def loss_reference(c, dtype):
    """`full_loss` (by column) in `dtype` on the case's arrays, upstream gradient 1.7.  Returns a dict of float64 numpy arrays:
    losses (4), aff (at J = nrm ++ abn), m (the hinge argument), d_emb, d_logits, d_con, d_abn."""
    ins = [torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in ("emb", "logits", "con", "eab")]
    total, lm, lb, lr, aff = O.full_loss(*ins, csr_triple(c["raw"]), c["abn"], c["nrm"], margin_c=MARGIN, by_column=True, dtype=dtype)
    total.backward(gradient=torch.tensor(G_TOTAL, dtype=dtype))
    J = torch.as_tensor(c["nrm"] + c["abn"], dtype=torch.long)
    nrm, abn = J[:len(c["nrm"])], J[len(c["nrm"]):]
    m = MARGIN - (aff[nrm].mean() - aff[abn].mean())
    f = lambda t: t.detach().double().numpy()                   # noqa: E731
    return dict(losses=np.array([total.item(), lm.item(), lb.item(), lr.item()], dtype=np.float64), aff=f(aff[J]), m=float(m),
                d_emb=f(ins[0].grad), d_logits=f(ins[1].grad), d_con=f(ins[2].grad), d_abn=f(ins[3].grad))


LOSS_CLASSES = dict(losses=LOSS, aff=AFF, d_emb=DGRAD, d_logits=DGRAD, d_con=DGRAD, d_abn=DGRAD)


def check_loss_reference(c, ref):
    """What the comparison relies on, asserted on the float64 reference alone: the hinge is clearly on one side, NaN sits only
    where torch's autograd is known to put it (the rows of zero embeddings -- `pow(norm, -1)`'s derivative is -inf where
    `where(isinf)` hands it a zero gradient: 0 * inf; the columns where emb_con - emb_abnormal is all zero -- the derivative of
    sqrt at 0 is inf, times d = 0), and the degenerate nodes give the values the reference's formulas give."""
    if c["inactive"]:
        assert ref["m"] < -1e-3, ref["m"]
        assert ref["losses"][1] == 0.0 and not np.any(ref["d_emb"][np.isfinite(ref["d_emb"])])
    else:
        assert ref["m"] > 1e-3, ref["m"]
        assert np.abs(ref["d_emb"][np.isfinite(ref["d_emb"])]).max() > 0
    nan_rows = np.nonzero(np.isnan(ref["d_emb"]).any(1))[0].tolist()
    assert nan_rows == sorted(c["zero_rows"]) and np.isnan(ref["d_emb"][nan_rows]).all()
    for k in ("d_con", "d_abn"):
        nan_cols = np.nonzero(np.isnan(ref[k]).any(0))[0].tolist()
        assert nan_cols == ([] if c["nan_column"] is None else [c["nan_column"]]) and np.isnan(ref[k][:, nan_cols]).all()
    assert np.isfinite(ref["losses"]).all() and np.isfinite(ref["aff"]).all() and np.isfinite(ref["d_logits"]).all()
    if c.get("lone") is not None:
        J = c["nrm"] + c["abn"]
        assert ref["aff"][J.index(c["lone"])] == 0.0 and ref["aff"][J.index(c["zero_rows"][0])] == 0.0


# ================================================================================================ head
def _head(n, h, nn, na, seed, **kw):
    return dict(n=n, h=h, nn=nn, na=na, seed=seed, **kw)


HEAD_CASES = {
    "node_in_both_lists_H64": _head(500, 64, 60, 9, 1, overlap=True),
    "adjacent_abnormal_nodes_H300": _head(900, 300, 200, 12, 2, adjacent=True),
    "abnormal_hub_H300": _head(3000, 300, 150, 6, 3, hub=True),
    "one_abnormal_one_normal_H64": _head(300, 64, 1, 1, 4),
    "plain_H64": _head(700, 64, 120, 17, 5),
    "plain_H300": _head(1200, 300, 260, 33, 6),
    "three_gemm_path_H516": _head(500, 516, 80, 10, 7, three_gemm=True),        # fc1 has 258 > 256 rows: `mlp_score_supported` is False
}


def head_case(name):
    p = HEAD_CASES[name]
    n, h, nn, na = p["n"], p["h"], p["nn"], p["na"]
    rng = np.random.default_rng(2000 + p["seed"])
    a = _graph(n, 8, 100 + p["seed"])
    perm = rng.permutation(n)
    nrm, abn = perm[:nn].tolist(), perm[nn:nn + na].tolist()
    rest = perm[nn + na:]
    if p.get("overlap"):
        abn[1] = nrm[2]
    if p.get("adjacent"):                                       # two abnormal nodes adjacent to each other and to a third
        for i, j in ((abn[0], abn[1]), (abn[0], abn[2]), (abn[1], abn[2])):
            a[i, j] = a[j, i] = 1.0
    if p.get("hub"):                                            # an abnormal hub: its row of A_hat has more than 2,000 entries
        t = rng.choice(rest, size=2300, replace=False)
        a[abn[0], t] = 1.0
        a[t, abn[0]] = 1.0
        a[abn[0], abn[1]] = a[abn[1], abn[0]] = 1.0
    a = _csr(a)
    adj_norm = _csr(_normalize(a) + sp.eye(n))
    raw = _csr(a + sp.eye(n))
    if p.get("hub"):
        assert adj_norm.indptr[abn[0] + 1] - adj_norm.indptr[abn[0]] > 2000
    L = nn + na
    w = lambda o, i: _f32(rng.standard_normal((o, i)) / np.sqrt(i))          # noqa: E731
    f = 32                                                      # the route through `Model` starts at the features
    model = dict(x=_f32(rng.standard_normal((n, f))), g1w=w(h, f), g1b=_f32(0.1 * rng.standard_normal(h)), g1a=_f32([0.25]),
                 g2w=w(h, h), g2b=_f32(0.1 * rng.standard_normal(h)), g2a=_f32([0.2]))
    return dict(model=model, name=name, n=n, h=h, nrm=nrm, abn=abn, adj_norm=adj_norm, raw=raw, emb=_f32(rng.standard_normal((n, h))),
                noise=_f32(0.3 * rng.standard_normal((na, h)) + 0.1), fc4=w(h, h), fc1=w(h // 2, h), fc2=w(h // 4, h // 2), fc3=w(1, h // 4),
                g_out=_f32(rng.standard_normal((n, h))), g_comb=_f32(rng.standard_normal((L, h))), g_f3=_f32(rng.standard_normal(L)),
                g_con=_f32(rng.standard_normal((na, h))), g_abn=_f32(rng.standard_normal((na, h))), three_gemm=bool(p.get("three_gemm")))


HEAD_OUT = ("emb_out", "comb", "f3", "con", "eab")
HEAD_GRAD = ("emb", "fc4", "fc1", "fc2", "fc3")
HEAD_CLASSES = dict(emb_out=FWD, comb=FWD, f3=FWD, con=FWD, eab=FWD, d_emb=DGRAD, d_fc4=WGRAD, d_fc1=WGRAD, d_fc2=WGRAD, d_fc3=WGRAD)
KINK = 1e-6                       # a ReLU / PReLU branch may differ from the float64 sign only within this share of the tensor's scale
KINK_SHARE = 1e-3                 # ... on at most 0.1 % of the tensor's entries


def head_reference(c, dtype, all_five, masks=None):
    """`full_head` in `dtype` from the case's emb on; upstream gradients g_out, g_f3, g_con, g_abn (what training produces:
    the loss reads emb, logits, emb_con, emb_abnormal) and, with `all_five`, g_comb too.  `masks`: ReLU branches to take (see
    `oracle._relu`).  Returns float64 numpy arrays: the five outputs, the five gradients, the three ReLU pre-activation signs'
    carriers (con, f1, f2: post-activation values, whose > 0 is the branch taken) and the pre-activations themselves."""
    P = {k + ".weight": torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in ("fc1", "fc2", "fc3", "fc4")}
    emb = torch.tensor(c["emb"], dtype=dtype, requires_grad=True)
    noise = torch.tensor(c["noise"], dtype=dtype)
    tm = None if masks is None else {k: torch.as_tensor(v) for k, v in masks.items()}
    out, comb, f3, con, eab, hid = O.full_head(P, emb, csr_triple(c["adj_norm"]), c["abn"], c["nrm"], noise, dtype, tm, want_hidden=True)
    g = lambda k: torch.tensor(c[k], dtype=dtype)               # noqa: E731
    s = (out * g("g_out")).sum() + (f3 * g("g_f3")).sum() + (con * g("g_con")).sum() + (eab * g("g_abn")).sum()
    if all_five:
        s = s + (comb * g("g_comb")).sum()
    s.backward()
    f = lambda t: t.detach().double().numpy()                   # noqa: E731
    r = dict(emb_out=f(out), comb=f(comb), f3=f(f3), con=f(con), eab=f(eab), d_emb=f(emb.grad))
    for k in ("fc1", "fc2", "fc3", "fc4"):
        r["d_" + k] = f(P[k + ".weight"].grad)
    r["pre"] = {k: f(v) for k, v in hid.items()}                # pre-activations of con, f1, f2
    return r


MODEL_PARAMS = {"gcn1.fc.weight": "g1w", "gcn1.bias": "g1b", "gcn1.act.weight": "g1a", "gcn2.fc.weight": "g2w", "gcn2.bias": "g2b",
                "gcn2.act.weight": "g2a", "fc1.weight": "fc1", "fc2.weight": "fc2", "fc3.weight": "fc3", "fc4.weight": "fc4"}


MODEL_CLASSES = dict({k: MODEL_FWD for k in HEAD_OUT}, **{"d_" + k: MODEL_WGRAD for k in MODEL_PARAMS})


def model_reference(c, dtype, all_five, masks=None):
    """`Model.forward` from the features on (two `gcn_layer`s, then `full_head`) in `dtype` with the upstream gradients of
    `head_reference`.  `masks`: branches of the two PReLUs ("z1", "z2") and the three ReLUs.  Returns the five outputs, the
    gradients of the ten parameters ("d_" + state_dict name) and the five pre-activations."""
    src = dict(c, **c["model"])
    P = {k: torch.tensor(src[v], dtype=dtype, requires_grad=True) for k, v in MODEL_PARAMS.items()}
    tm = {} if masks is None else {k: torch.as_tensor(v) for k, v in masks.items()}
    adjn = csr_triple(c["adj_norm"])
    x = torch.tensor(src["x"], dtype=dtype)
    h1, z1 = O.gcn_layer(x, P["gcn1.fc.weight"], P["gcn1.bias"], P["gcn1.act.weight"], adjn, dtype, tm.get("z1"), want_pre=True)
    emb, z2 = O.gcn_layer(h1, P["gcn2.fc.weight"], P["gcn2.bias"], P["gcn2.act.weight"], adjn, dtype, tm.get("z2"), want_pre=True)
    noise = torch.tensor(c["noise"], dtype=dtype)
    out, comb, f3, con, eab, hid = O.full_head(P, emb, adjn, c["abn"], c["nrm"], noise, dtype, tm or None, want_hidden=True)
    g = lambda k: torch.tensor(c[k], dtype=dtype)               # noqa: E731
    s = (out * g("g_out")).sum() + (f3 * g("g_f3")).sum() + (con * g("g_con")).sum() + (eab * g("g_abn")).sum()
    if all_five:
        s = s + (comb * g("g_comb")).sum()
    s.backward()
    f = lambda t: t.detach().double().numpy()                   # noqa: E731
    r = dict(emb_out=f(out), comb=f(comb), f3=f(f3), con=f(con), eab=f(eab))
    for k in MODEL_PARAMS:
        r["d_" + k] = f(P[k].grad)
    r["pre"] = dict({k: f(v) for k, v in hid.items()}, z1=f(z1), z2=f(z2))
    return r


def masks_of(pre_or_post):
    return {k: np.asarray(v) > 0 for k, v in pre_or_post.items()}


def check_masks(masks, pre64):
    """The branches a float32 run took against the float64 pre-activations: they may differ only within KINK of the tensor's
    scale, on at most KINK_SHARE of its entries."""
    for k, m in masks.items():
        z = pre64[k]
        flip = m != (z > 0)
        scale = np.abs(z).max()
        assert flip.mean() <= KINK_SHARE, (k, float(flip.mean()))
        assert not flip.any() or np.abs(z[flip]).max() <= KINK * scale, (k, float(np.abs(z[flip]).max() / scale))


# ================================================================================================ GCN layer
SLOPES = (0.25, 0.0, -0.3)
GCN_ROUTES = {"const_F10": 10, "const_F25": 25, "const_F745": 745, "grad_input_F64": 64}
GCN_WIDTHS = (64, 300, 512)
GCN_CASES = {}
for _ri, (_r, _f) in enumerate(GCN_ROUTES.items()):
    for _hi, _h in enumerate(GCN_WIDTHS):
        _a = SLOPES[(_ri + _hi) % 3]                            # every route and every width meets every slope
        GCN_CASES[f"{_r}_H{_h}_slope{_a}"] = dict(route=_r, f=_f, h=_h, slope=_a, seed=10 * _ri + _hi)


def gcn_case(name):
    """One `GcnLayerFn` case: a graph with a hub row (1,100 entries), a row that holds only its diagonal and an empty row (that
    node has no edge and the adjacency is passed without `+ I` for it)."""
    p = GCN_CASES[name]
    n, f, h = 1500, p["f"], p["h"]
    rng = np.random.default_rng(3000 + p["seed"])
    a = _graph(n, 8, 200 + p["seed"])
    hub, diag_only, empty = 5, 17, 29
    t = rng.choice(np.arange(100, n), size=1100, replace=False)
    a[hub, t] = 1.0
    a[t, hub] = 1.0
    for v in (diag_only, empty):
        a[v, :] = 0.0
        a[:, v] = 0.0
    eye = np.ones(n)
    eye[empty] = 0.0
    a = _csr(a)
    adj_norm = _csr(_normalize(a) + sp.diags(eye))
    raw = _csr(a + sp.diags(eye))
    cnt = np.diff(adj_norm.indptr)
    assert cnt[hub] > 1000 and cnt[diag_only] == 1 and cnt[empty] == 0
    return dict(name=name, n=n, f=f, h=h, adj_norm=adj_norm, raw=raw, x=_f32(rng.standard_normal((n, f))),
                w=_f32(rng.standard_normal((h, f)) / np.sqrt(f)), b=_f32(0.1 * rng.standard_normal(h)), a=_f32([p["slope"]]),
                g=_f32(rng.standard_normal((n, h))), x_grad=p["route"].startswith("grad"), hub=hub, diag_only=diag_only, empty=empty)


GCN_CLASSES = dict(out=FWD, dx=DGRAD, dw=WGRAD, db=WGRAD, da=WGRAD)


def gcn_reference(c, dtype, mask=None):
    x = torch.tensor(c["x"], dtype=dtype, requires_grad=c["x_grad"])
    w, b, a = (torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in ("w", "b", "a"))
    out, z = O.gcn_layer(x, w, b, a, csr_triple(c["adj_norm"]), dtype, None if mask is None else torch.as_tensor(mask), want_pre=True)
    out.backward(gradient=torch.tensor(c["g"], dtype=dtype))
    f = lambda t: t.detach().double().numpy()                   # noqa: E731
    r = dict(out=f(out), dw=f(w.grad), db=f(b.grad), da=f(a.grad), pre={"z": f(z)})
    if c["x_grad"]:
        r["dx"] = f(x.grad)
    return r
