"""The row-local kernels of the full-graph GGAD step against the float64 oracle, at every branch: the loss block (`GgadLossFn`:
k_loss_fwd_fused, k_loss_bwd_fused, k_rownorm_bwd_add and the launch sequence they replace), the head (`GgadHeadFn`: k_head_rows,
k_head_emb_put, k_head_con_grad, k_head_emb_grad; with `_HEAD_LEAN` off; op by op through `Model`) and the GCN layer
(`GcnLayerFn` on its three routes).  One autograd node or layer per test, on float32 inputs built on the host
(tests/fullgraph_fp64.py); the reference is `oracle/ggad_oracle.py` (`full_loss`, `full_head`, `gcn_layer`) run by torch in
float64 on the CPU on the same arrays, outputs and every input gradient, upstream gradients that are not 1.  Every case runs twice
and the second run is bit-identical; after every fused-loss call the ticket word is 0.

Kinks.  The hinge: every case asserts on the reference that its argument m is beyond +-1e-3.  ReLU / PReLU: the float64 reference
takes the branches the kernels took (their saved activations; through `Model`, the same kernels run once more on the same inputs),
and those branches may differ from the float64 signs only within 1e-6 of the tensor's scale on at most 0.1 % of its entries.

What float64 torch returns at the degenerate points, stated rather than smoothed over:
  * a column of emb_con - emb_abnormal that is exactly 0: NaN in that column of d emb_con and d emb_abnormal (the derivative of
    sqrt at 0 is inf, times d = 0) and finite values elsewhere.  The kernels agree: kcol = 1 / (H * 0) = inf, times d = 0.
  * a zero embedding row: NaN on that row of d emb (`where(isinf(inv), 0, inv)` hands `pow(norm, -1)` a zero gradient and its
    derivative there is -inf: 0 * inf), in float32 as in float64, per edge as by column (tests/test_oracle_fp64.py).  The
    reference's `run.py:177-181` is these ops, so its training would turn NaN there.  The kernels do NOT agree: k_rownorm_bwd /
    k_rownorm_bwd_add multiply by inv = 0 and return exactly 0 on such a row -- the derivative of the function as written,
    e_hat = 0 wherever |e| = 0.  The cases assert both facts (NaN in the reference, 0 in the kernels) and compare every other row.

Tolerances (measured, tests/fullgraph_fp64.py `BOUND`).  d32 = max |f32 - f64| / max |f64| of the float32 oracle against the float64
oracle on every case of this module (CPU; tests/test_oracle_fp64.py asserts d32 <= bound / 4 for every tensor); the GPU bound of a
class is 4 x its largest d32 -- a correct float32 kernel that sums in another order than torch (64-lane butterflies, split
partials, fused multiply-adds) moves by a small multiple of what torch's own float32 moves.  All are far inside what
tests/test_fullgraph_fullsize_gpu.py grants (2e-5 on forward tensors and losses, 1e-4 on gradients).

    class              largest d32   where                                  bound     largest distance seen on an MI355X
    forward tensors    1.14e-6       GCN out, const_F745_H300               4.6e-6    6.3e-7
    losses             1.15e-7       A844_H300                              4.7e-7    1.1e-7
    affinity           3.10e-7       A31_H300                               1.3e-6    2.2e-7
    data gradients     6.6e-7        GCN dx, grad_input_F64_H300            2.7e-6    6.6e-7
    weight gradients   1.84e-6       GCN da, const_F745_H512_slope0.0       7.4e-6    7.3e-7
    through `Model` (two GCN layers, then the head: four layers deep), classes of their own so that the rows above stay tight:
    forward tensors    2.74e-6       logits, abnormal_hub_H300              1.1e-5    8.2e-7
    weight gradients   2.83e-6       d gcn2.act.weight, adjacent_..._H300   1.2e-5    2.6e-6
(Where the GPU figure equals d32 -- dx, d gcn1.act.weight -- the distance is the float32 rounding of the adjacency values, which the
kernels and the float32 oracle share: `Csr` casts them as `run.py:103-109` does, the float64 oracle keeps them in float64.)

Found by this module and fixed with it: a node that sits TWICE inside one list (`seg_unique` False, launch sequence).  The
scatter-add of c_j S_j onto the rows J ran as one `k_rows_scale` launch per segment, which assumes duplicate-free rows: two waves
read-modify-wrote the same row of `den` and one term was lost (d emb off by 0.12 of its scale in `duplicate_in_normal_list`, fused
switch on or off).  `loss_structs` now deals such lists into duplicate-free rounds (the k-th occurrence of every node) and the
backward launches them one after the other.
"""
import functools
import types

import numpy as np
import pytest
import torch

import fullgraph_fp64 as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd import _lib
    from ggad_amd import fullgraph as FG
    from ggad_amd.model import Model

DEV = "cuda:0"
SEEN = {}                         # class -> (largest distance, case, tensor): printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for cls, (d, name, key) in sorted(SEEN.items()):
        print(f"\n[fullgraph branches] largest distance, {cls}: {d:.3e} ({name}, {key}), bound {C.BOUND[cls]:.1e}")


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _adj(c):
    return FG.FullGraphAdj(c["adj_norm"], c["raw"], DEV)


def _compare(name, got, ref, classes, keys=None):
    for k in (keys or classes):
        g, r = got[k], ref[k]
        assert g.shape == r.shape, (name, k, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.isfinite(g[~np.isnan(r)]).all(), (name, k, "NaN placement")
        d = C.distance(g, r)
        cls = classes[k]
        print(f"{name} {k}: {d:.3e} (bound {C.BOUND[cls]:.1e})")
        if d > SEEN.get(cls, (-1.0,))[0]:
            SEEN[cls] = (d, name, k)
        assert d <= C.BOUND[cls], (name, k, d, C.BOUND[cls])


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


# ================================================================================================ loss block
@functools.lru_cache(maxsize=4)
def _loss_case_and_reference(name):
    c = C.loss_case(name)
    ref = None
    if not c["refused"]:
        ref = C.loss_reference(c, torch.float64)
        C.check_loss_reference(c, ref)
    return c, ref


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "launch_sequence"])
@pytest.mark.parametrize("name", list(C.LOSS_CASES))
def test_loss_block(name, fused, monkeypatch):
    """`GgadLossFn` with `_LOSS_FUSED` on and off against `full_loss` in float64: the four losses, the affinity vector the node
    keeps, d emb, d logits, d emb_con, d emb_abnormal; which path ran is read from `total.grad_fn.fused`."""
    c, ref = _loss_case_and_reference(name)
    monkeypatch.setattr(FG, "_LOSS_FUSED", fused)
    fa = _adj(c)
    ls = fa.loss_structs(c["nrm"], c["abn"])
    assert ls["seg_unique"] == c["seg_unique"] and ls["distinct"] == c["distinct"]
    # a duplicate inside a list: the launch sequence runs whatever the switch says; wider than 1,024: too
    want_fused = fused and c["seg_unique"] and c["h"] <= 1024

    def run():
        ins = [_dev(c[k], True) for k in ("emb", "logits", "con", "eab")]
        out = FG.GgadLossFn.apply(*ins, fa, ls, C.MARGIN)
        node = out[0].grad_fn
        assert node.fused == want_fused
        aff = node.affinity
        out[0].backward(gradient=torch.full((), C.G_TOTAL, device=DEV))
        torch.cuda.synchronize()
        if want_fused:
            assert int(ls["loss_ws_fused"][1].item()) == 0                    # the last workgroup put the ticket back
        return dict(losses=np.array([o.item() for o in out], dtype=np.float32), aff=_np(aff), d_emb=_np(ins[0].grad),
                    d_logits=_np(ins[1].grad), d_con=_np(ins[2].grad), d_abn=_np(ins[3].grad))

    if c["refused"]:
        # H % 4 != 0: the sparse products move 16-byte chunks and say so (before anything is launched)
        with pytest.raises(_lib.GgadKernelError):
            run()
        return
    got = run()
    ref = dict(ref)
    if c["zero_rows"]:
        # zero embedding rows: NaN in torch (checked on the reference), exactly 0 in the kernels -- see the module docstring
        z = c["zero_rows"]
        assert np.isnan(ref["d_emb"][z]).all() and not np.any(got["d_emb"][z]) and np.isfinite(got["d_emb"]).all()
        ref["d_emb"] = ref["d_emb"].copy()
        ref["d_emb"][z] = 0.0
    if c["inactive"]:
        assert got["losses"][1] == 0.0 and not np.any(got["d_emb"]) and not np.isnan(got["d_emb"]).any()      # exactly 0, no NaN
    if c["nan_column"] is not None:
        col = c["nan_column"]
        for k in ("d_con", "d_abn"):
            assert np.isnan(got[k][:, col]).all() and np.isfinite(np.delete(got[k], col, axis=1)).all()
    _compare(f"loss/{name}/{'fused' if fused else 'sequence'}", got, ref, C.LOSS_CLASSES)
    _same_bits(got, run())


# ================================================================================================ head
@functools.lru_cache(maxsize=2)
def _head_case(name):
    return C.head_case(name)


def _head_grads(outs, c, all_five):
    emb_out, comb, f3, con, eab = outs
    tensors = [emb_out, f3, con, eab] + ([comb] if all_five else [])
    grads = [_dev(c[k]).reshape(t.shape) for k, t in zip(("g_out", "g_f3", "g_con", "g_abn", "g_comb"), tensors)]
    torch.autograd.backward(tensors, grads)


@pytest.mark.parametrize("upstream", ["training", "all_five"])
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "not_lean"])
@pytest.mark.parametrize("name", list(C.HEAD_CASES))
def test_head_node(name, lean, upstream, monkeypatch):
    """`GgadHeadFn` against `full_head` in float64 from the same emb: the five outputs, and d emb, d fc4, d fc1, d fc2, d fc3 under
    the upstream pattern of training (g_comb None: the loss does not read emb_combine) and with all five given.  Lean mode also
    keeps its aliasing contract: the returned emb_out is the input, rows abn hold emb_con, every other row is bit-unchanged."""
    c = _head_case(name)
    all_five = upstream == "all_five"
    monkeypatch.setattr(FG, "_HEAD_LEAN", lean)
    fa = _adj(c)
    hs = fa.head_structs(c["nrm"], c["abn"])
    assert hs is not None

    def run():
        emb = _dev(c["emb"], True)
        w = {k: _dev(c[k], True) for k in ("fc4", "fc1", "fc2", "fc3")}
        assert FG.mlp_score_supported(w["fc1"], w["fc2"], w["fc3"]) == (not c["three_gemm"])
        emb_in = emb.clone()                                                 # (lean mode writes into its input: not a leaf)
        before = emb_in.detach().clone()
        outs = FG.GgadHeadFn.apply(emb_in, _dev(c["noise"]), w["fc4"], w["fc1"], w["fc2"], w["fc3"], fa, hs)
        saved = outs[2].grad_fn.saved_tensors                                # (con_pre, emb_con, comb, f1, f2, weights)
        masks = {"con": _np(saved[1]) > 0, "f1": _np(saved[3]) > 0, "f2": _np(saved[4]) > 0}
        res = {k: _np(t) for k, t in zip(C.HEAD_OUT, outs)}
        res["f3"] = res["f3"].reshape(-1)
        if lean:
            abn = torch.as_tensor(c["abn"], device=DEV)
            keep = torch.ones(c["n"], dtype=torch.bool, device=DEV)
            keep[abn] = False
            assert outs[0].data_ptr() == emb_in.data_ptr() and outs[0].shape == emb_in.shape      # emb_out IS the input
            assert torch.equal(emb_in.detach()[abn].view(torch.int32), outs[3].detach().view(torch.int32))
            assert torch.equal(emb_in.detach()[keep].view(torch.int32), before[keep].view(torch.int32))
        else:
            assert outs[0].data_ptr() != emb_in.data_ptr() and torch.equal(emb_in.detach().view(torch.int32), before.view(torch.int32))
        _head_grads(outs, c, all_five)
        torch.cuda.synchronize()
        res["d_emb"] = _np(emb.grad)
        for k in w:
            res["d_" + k] = _np(w[k].grad)
        return res, masks

    got, masks = run()
    ref = C.head_reference(c, torch.float64, all_five, masks)
    C.check_masks(masks, ref["pre"])
    _compare(f"head/{name}/{'lean' if lean else 'not_lean'}/{upstream}", got, ref, C.HEAD_CLASSES)
    _same_bits(got, run()[0])


@pytest.mark.parametrize("upstream", ["training", "all_five"])
@pytest.mark.parametrize("name", list(C.HEAD_CASES))
def test_head_op_by_op_through_model(name, upstream):
    """`Model.forward` with `fused_head = False` (torch indexing, `SpmmRowsFn`, `LinearFn` / `MlpScoreFn`) from the features on,
    against two `gcn_layer`s and `full_head` in float64: the five outputs and the gradients of all ten parameters."""
    c = _head_case(name)
    m = c["model"]
    all_five = upstream == "all_five"
    fa = _adj(c)
    src = dict(c, **m)
    args = types.SimpleNamespace(mean=0.0, var=0.0)

    def build():
        torch.manual_seed(0)
        model = Model(m["x"].shape[1], c["h"], "prelu", 1, "avg")
        sd = model.state_dict()
        for k, v in C.MODEL_PARAMS.items():
            sd[k] = torch.from_numpy(src[v]).reshape(sd[k].shape)
        model.load_state_dict(sd)
        model.to(DEV).train()
        model.fused_head = False
        model.noise_override = _dev(c["noise"])[None]
        return model

    def run():
        model = build()
        outs = model(_dev(m["x"])[None], fa, c["abn"], c["nrm"], True, args)
        assert outs[0].shape == (1, c["n"], c["h"]) and outs[3].shape == (len(c["abn"]), c["h"])
        res = {k: _np(t).reshape(-1) if k == "f3" else _np(t).reshape(-1, c["h"]) for k, t in zip(C.HEAD_OUT, outs)}
        _head_grads(outs, c, all_five)
        torch.cuda.synchronize()
        named = dict(model.named_parameters())
        for k in C.MODEL_PARAMS:
            res["d_" + k] = _np(named[k].grad)
        assert all(p.grad is None for k, p in named.items() if k not in C.MODEL_PARAMS)
        return res, model

    got, model = run()
    # the branches the kernels took: the same kernels once more on the same inputs (they are bit-reproducible, asserted below)
    with torch.no_grad():
        p = dict(model.named_parameters())
        x = _dev(m["x"])
        z = []
        h1 = x
        for pre in ("gcn1", "gcn2"):
            with torch.enable_grad():
                o = FG.GcnLayerFn.apply(h1, p[pre + ".fc.weight"], p[pre + ".bias"], p[pre + ".act.weight"], fa)
            z.append(_np(o.grad_fn.saved_tensors[2]))
            h1 = o.detach().requires_grad_()                                 # (as inside Model: the second layer's input needs a gradient)
        assert np.array_equal(_np(h1)[np.setdiff1d(np.arange(c["n"]), c["abn"])], got["emb_out"][np.setdiff1d(np.arange(c["n"]), c["abn"])])
        comb = _dev(got["comb"])
        if FG.mlp_score_supported(p["fc1.weight"], p["fc2.weight"], p["fc3.weight"]):
            f1, f2, _ = FG.mlp_score_fwd(comb, p["fc1.weight"], p["fc2.weight"], p["fc3.weight"])
        else:
            f1 = FG.gemm(comb, p["fc1.weight"], False, True, relu=True)
            f2 = FG.gemm(f1, p["fc2.weight"], False, True, relu=True)
        assert FG.mlp_score_supported(p["fc1.weight"], p["fc2.weight"], p["fc3.weight"]) == (not c["three_gemm"])
    masks = {"z1": z[0] > 0, "z2": z[1] > 0, "con": got["con"] > 0, "f1": _np(f1) > 0, "f2": _np(f2) > 0}
    ref = C.model_reference(c, torch.float64, all_five, masks)
    C.check_masks(masks, ref["pre"])
    _compare(f"head/{name}/model_unfused/{upstream}", got, ref, C.MODEL_CLASSES)
    _same_bits(got, run()[0])


# ================================================================================================ GCN layer
@pytest.mark.parametrize("name", list(C.GCN_CASES))
def test_gcn_layer(name):
    """`GcnLayerFn` against `gcn_layer` in float64 on a graph with a hub row, a diagonal-only row and an empty row: out, dW, db,
    da and (where the input needs one) dx, on the route through the cached aggregate (F = 10, 25: zero-padded `axp` and weight),
    the padded constant (F = 745) and the general route (an input that needs a gradient)."""
    c = C.gcn_case(name)
    fa = _adj(c)

    def run():
        x = _dev(c["x"], c["x_grad"])
        w, b, a = _dev(c["w"], True), _dev(c["b"], True), _dev(c["a"], True)
        out = FG.GcnLayerFn.apply(x, w, b, a, fa)
        node = out.grad_fn
        reordered = c["f"] < c["h"] and not c["x_grad"]
        assert node.reordered == reordered
        if reordered:
            axp = fa._ax["axp"]
            assert (axp is not None) == (c["f"] % 4 != 0) and (axp is None or axp.shape[1] == max((c["f"] + 3) // 4 * 4, 20))
        else:
            assert (FG.padded_constant(fa, x) is not None) == (c["f"] % 4 != 0 and not c["x_grad"])
        z = _np(node.saved_tensors[2])
        res = dict(out=_np(out))
        out.backward(gradient=_dev(c["g"]))
        torch.cuda.synchronize()
        res.update(dw=_np(w.grad), db=_np(b.grad), da=_np(a.grad))
        if c["x_grad"]:
            res["dx"] = _np(x.grad)
        else:
            assert x.grad is None
        return res, z

    got, z = run()
    assert not np.any(got["out"][c["empty"]] - np.where(c["b"] > 0, c["b"], c["a"][0] * c["b"]))      # the empty row: PReLU(b)
    mask = z > 0
    ref = C.gcn_reference(c, torch.float64, mask)
    C.check_masks({"z": mask}, ref["pre"])
    _compare(f"gcn/{name}", got, ref, C.GCN_CLASSES, [k for k in C.GCN_CLASSES if k in ref])
    _same_bits(got, run()[0])
