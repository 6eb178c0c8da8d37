"""Every entry point whose launch hands partial results to "the last workgroup to finish" (csrc/handoff.h), called the way an epoch
calls it: four times in a row on ONE workspace and the device's shared ticket block (`fullgraph.ticket_block`), fresh data every
call, 32 MB of dirty lines between the calls.  A partial read from a stale line -- the previous call's sums -- is the one thing these
kernels can get wrong without faulting.  Every call must be bit-equal to the same call on a fresh workspace with a freshly zeroed
ticket tensor of its own, and within the float64 reference and tolerance of the entry point's own test (imported from there, or
restated from it line for line where that test keeps them inline); the ticket words are zero afterwards.

Shapes: the smallest with two workgroups (for the two-level kernels: two first-level groups, the last one partial); the counts are
asserted through the library where it exports them."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fullgraph_fp64 as C
import tam_head_fp64 as H
from test_aegis_gpu import _bn_ref
from test_dominant_gpu import _check64, _lists, _params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CALLS = 4


def _lib():
    from ggad_amd import _lib as L
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    from ggad_amd._lib import ptr
    return ptr(t)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _empty(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _ok(rc):
    assert rc == 0, rc


# ------------------------------------------------------------------------------------------------ AEGIS batch norm
BN_M, BN_C = 513, 64


class BnFwd:
    """ggad_aegis_bn_fwd_f32 (k_bn_stats): y = relu(BN(h)), mean, 1 / sqrt(var + eps)."""

    def check_shape(self):
        assert int(_lib().ggad_aegis_bn_groups(BN_M)) >= 2

    def inputs(self, k):
        rng = np.random.default_rng(100 + k)
        h = rng.standard_normal((BN_M, BN_C)) * rng.uniform(0.1, 3, BN_C) + rng.uniform(-2, 2, BN_C) + k
        return dict(h=_f32(h), g=_f32(rng.uniform(0.5, 1.5, BN_C)), b=_f32(rng.uniform(-0.5, 0.5, BN_C)))

    def workspace(self):
        return _empty(int(_lib().ggad_aegis_bn_workspace_elems(BN_M, BN_C)))

    def run(self, x, ws, tick):
        y, mean, invstd = _empty(BN_M, BN_C), _empty(BN_C), _empty(BN_C)
        _ok(_lib().ggad_aegis_bn_fwd_f32(_ptr(x["h"]), BN_M, BN_C, 0, 0, 0, BN_C, _ptr(x["g"]), _ptr(x["b"]), 1e-5, 0.1, 0, 0, 0, 0, 0, BN_M,
                                         _ptr(y), BN_C, 0, 0, 0, _ptr(mean), _ptr(invstd), _ptr(ws), _ptr(tick), _st()))
        return dict(y=y, mean=mean, invstd=invstd)

    def check(self, x, got):
        h64 = x["h"].cpu().double()
        ref = _bn_ref(h64, x["g"].cpu().double(), x["b"].cpu().double(), 0)
        np.testing.assert_allclose(got["y"], ref.numpy(), rtol=1e-5, atol=2e-5)                    # test_bn_forward_backward_vs_float64
        np.testing.assert_allclose(got["mean"], h64.mean(0).numpy(), rtol=1e-5, atol=1e-6)


class BnBwd(BnFwd):
    """ggad_aegis_bn_bwd_f32 (k_bn_bwd_sums): dh, dgamma, dbeta from dy (mean and 1 / std from a forward call of its own)."""

    def inputs(self, k):
        x = BnFwd.inputs(self, k)
        x["dy"] = _f32(np.random.default_rng(200 + k).standard_normal((BN_M, BN_C)))
        f = BnFwd.run(self, x, BnFwd.workspace(self), torch.zeros(4, dtype=torch.int32, device=DEV))
        x.update(mean=f["mean"], invstd=f["invstd"])
        return x

    def run(self, x, ws, tick):
        dh, dg, db = _empty(BN_M, BN_C), _empty(BN_C), _empty(BN_C)
        _ok(_lib().ggad_aegis_bn_bwd_f32(_ptr(x["h"]), BN_M, BN_C, BN_C, _ptr(x["g"]), _ptr(x["b"]), _ptr(x["mean"]), _ptr(x["invstd"]), 0,
                                         _ptr(x["dy"]), BN_C, 0, 0, 0, _ptr(dh), BN_C, _ptr(dg), _ptr(db), 0, 0, _ptr(ws), _ptr(tick), _st()))
        return dict(dh=dh, dgamma=dg, dbeta=db)

    def check(self, x, got):
        ins = [x[k].cpu().double().requires_grad_() for k in ("h", "g", "b")]
        grads = torch.autograd.grad(_bn_ref(*ins, 0), ins, x["dy"].cpu().double())
        for name, r in zip(("dh", "dgamma", "dbeta"), grads):                                      # test_bn_forward_backward_vs_float64
            r = r.numpy()
            np.testing.assert_allclose(got[name], r, rtol=2e-4, atol=2e-5 * (np.abs(r).max() + 1e-3) * max(1, BN_M ** 0.5 / 30), err_msg=name)


# ------------------------------------------------------------------------------------------------ AEGIS losses
LOSS_N, LOSS_F = 129, 10


class AegisLoss:
    """ggad_aegis_loss_fwd_f32 (k_loss_fwd): BCE(p, 0) over 129 rows and the mean attribute error over a list of 57 of them."""

    def check_shape(self):
        assert int(_lib().ggad_aegis_loss_workspace_elems(LOSS_N, 57)) // 2 >= 2      # two floats per workgroup

    def inputs(self, k):
        rng = np.random.default_rng(300 + k)
        zd = np.zeros((LOSS_N, 12), dtype=np.float32)
        zd[:, :LOSS_F] = rng.random((LOSS_N, LOSS_F))
        rows = rng.permutation(LOSS_N)[:57]
        return dict(p=_f32(rng.uniform(0.01, 0.99, LOSS_N)), x=_f32(rng.random((LOSS_N, LOSS_F))), zd=_f32(zd),
                    rows=torch.from_numpy(rows.astype(np.int64)).to(DEV))

    def workspace(self):
        return _empty(int(_lib().ggad_aegis_loss_workspace_elems(LOSS_N, 57)))

    def run(self, x, ws, tick):
        attr, vals = _empty(57), _empty(2)
        _ok(_lib().ggad_aegis_loss_fwd_f32(_ptr(x["p"]), LOSS_N, _ptr(x["x"]), LOSS_F, _ptr(x["zd"]), 12, _ptr(x["rows"]), 57, _ptr(attr),
                                           vals.data_ptr(), vals.data_ptr() + 4, _ptr(ws), _ptr(tick), _st()))
        return dict(attr=attr, vals=vals)

    def check(self, x, got):
        p64, r = x["p"].cpu().double(), x["rows"].cpu()
        lg64 = torch.nn.functional.binary_cross_entropy(p64, torch.zeros_like(p64)).item()
        la64 = torch.mean(torch.sqrt(torch.sum((x["x"].cpu().double()[r] - x["zd"].cpu().double()[r, :LOSS_F]) ** 2, 1))).item()
        assert abs(got["vals"][0] - lg64) < 1e-5 * abs(lg64)                                       # test_losses_vs_float64
        assert abs(got["vals"][1] - la64) < 1e-5 * abs(la64)


# ------------------------------------------------------------------------------------------------ DOMINANT
DOM_N, DOM_F, DOM_H, DOM_M, DOM_T = 400, 10, 300, 200, 70      # ceil(200 / 16) + ceil(70 / 16) = 18 workgroups: groups of 16 and 2


def _dom_rows(k):
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.model_dominant import ae_rows
    rng = np.random.default_rng(400 + k)
    fa = FullGraphAdj(sp.eye(DOM_N, format="csr"), sp.eye(DOM_N, format="csr"), DEV)
    tr, te = _lists(DOM_N, DOM_M, DOM_T, rng)
    return rng, tr, te, ae_rows(fa, tr, te)


class DominantAe:
    """ggad_dominant_ae_f32 (k_dominant_ae, both ticket levels): loss, scores and the four gradients."""

    def check_shape(self):
        # the grid rule of ggad_dominant_ae_f32: one workgroup per 16-row tile of either list up to 256, reduced in groups of 16
        assert -(-DOM_M // 16) + -(-DOM_T // 16) >= 17 and (-(-DOM_M // 16) + -(-DOM_T // 16)) % 16 != 0
        assert int(_lib().ggad_dominant_ae_supported(DOM_F, DOM_H)) == 1

    def inputs(self, k):
        rng, tr, te, rs = _dom_rows(k)
        return dict(x=_f32(rng.random((DOM_N, DOM_F))), ps=_params(DOM_F, DOM_H, 400 + k), tr=tr, te=te, rs=rs)

    def workspace(self):
        return _empty(int(_lib().ggad_dominant_ae_workspace_elems(DOM_M, DOM_T, DOM_F, DOM_H)))

    def run(self, x, ws, tick):
        w1, b1, w2, b2 = [p.detach() for p in x["ps"]]
        loss, score = _empty(1), _empty(DOM_T)
        g = [_empty(*p.shape) for p in x["ps"]]
        _ok(_lib().ggad_dominant_ae_f32(_ptr(x["x"]), DOM_F, _ptr(x["rs"]["rows"]), DOM_M, DOM_T, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), DOM_H,
                                        _ptr(score), _ptr(loss), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(g[3]), _ptr(ws), _ptr(tick), _st()))
        return dict(loss=loss, score=score, dw1=g[0], db1=g[1], dw2=g[2], db2=g[3])

    def check(self, x, got):
        _check64(DOM_F, x["ps"], x["x"], x["tr"], x["te"], (float(got["loss"][0]), got["score"], [got[k] for k in ("dw1", "db1", "dw2", "db2")]))


class DominantRecon(DominantAe):
    """ggad_dominant_recon_f32 (k_dominant_recon) on x_ = W2 relu(W1 x + b1) + b2 formed by torch: loss, scores, and dX_ carried back
    to the four parameters by torch's autograd, so that the reference and tolerances of the fused path apply as they stand."""

    def check_shape(self):
        assert int(_lib().ggad_dominant_recon_workspace_elems(DOM_N, DOM_M, DOM_T)) >= 2          # one float per workgroup

    def inputs(self, k):
        x = DominantAe.inputs(self, k)
        w1, b1, w2, b2 = x["ps"]
        x["xh"] = torch.relu(x["x"] @ w1.t() + b1) @ w2.t() + b2
        return x

    def workspace(self):
        return _empty(int(_lib().ggad_dominant_recon_workspace_elems(DOM_N, DOM_M, DOM_T)))

    def run(self, x, ws, tick):
        loss, score, dxh = _empty(1), _empty(DOM_T), _empty(DOM_N, DOM_F)
        rs = x["rs"]
        _ok(_lib().ggad_dominant_recon_f32(_ptr(x["x"]), _ptr(x["xh"].detach()), DOM_N, DOM_F, _ptr(rs["rows"]), DOM_M, DOM_T, _ptr(rs["pos"]),
                                           _ptr(score), _ptr(loss), _ptr(dxh), _ptr(ws), _ptr(tick), _st()))
        return dict(loss=loss, score=score, dxh=dxh)

    def check(self, x, got):
        grads = torch.autograd.grad(x["xh"], x["ps"], torch.from_numpy(got["dxh"]).to(DEV), retain_graph=True)
        _check64(DOM_F, x["ps"], x["x"], x["tr"], x["te"], (float(got["loss"][0]), got["score"], [g.cpu().numpy() for g in grads]))


# ------------------------------------------------------------------------------------------------ TAM head
TAM_N, TAM_HUB_DEG, TAM_W = 1300, 1031, 64      # 6 reduce workgroups of 256 rows; one hub of 1,031 entries = 3 pieces of 512


def _tam_adj():
    """Symmetric R = I + a ring + node 7 joined to 1,030 others, all ones."""
    from ggad_amd.fullgraph import FullGraphAdj
    n = TAM_N
    ring = np.arange(n)
    nb = np.setdiff1d(np.arange(n), [6, 7, 8])[:TAM_HUB_DEG - 3]
    up = sp.coo_matrix((np.ones(n + len(nb)), (np.r_[ring, np.full(len(nb), 7)], np.r_[(ring + 1) % n, nb])), shape=(n, n))
    R = ((up + up.T + sp.eye(n)) > 0).astype(np.float32).tocsr()
    R.sort_indices()
    assert np.diff(R.indptr)[7] == TAM_HUB_DEG and abs(R - R.T).nnz == 0
    return R, FullGraphAdj(R, R, DEV)


class TamFwd:
    """ggad_tam_head_fwd_f32 (k_tam_reduce): a, the scalar block, m.  The ticket words are in the head's own zeroed workspace."""
    bwd = False

    def __init__(self):
        self.R = self.adj = self.head = None

    def check_shape(self):
        from ggad_amd import tam_utils as T
        self.R, self.adj = _tam_adj()
        self.idx = np.random.default_rng(5).choice(TAM_N, 200).astype(np.int64)
        self.head = T.tam_head(self.adj, self.idx)
        hub = int(_lib().ggad_tam_head_hub_len())
        assert self.head.n_hub == 1 and self.head.n_pieces == -(-TAM_HUB_DEG // hub) >= 3 and TAM_HUB_DEG > 1024
        assert -(-TAM_N // 256) >= 2                                  # the grid rule of k_tam_reduce: 256 rows per workgroup up to 256

    def inputs(self, k):
        return dict(e=_f32(np.random.default_rng(500 + k).standard_normal((TAM_N, TAM_W)) + 0.1 * k))

    def workspace(self):
        return torch.zeros(int(_lib().ggad_tam_head_workspace_elems(TAM_N, TAM_W, self.head.n_hub, self.head.n_pieces)), dtype=torch.float32,
                           device=DEV)

    def run(self, x, ws, tick):
        o = dict(a=_empty(TAM_N), scal=_empty(8), m=_empty(TAM_N), inv=_empty(TAM_N))
        args = self.head._args(x["e"])
        _ok(_lib().ggad_tam_head_fwd_f32(*args, _ptr(o["a"]), _ptr(o["scal"]), _ptr(o["m"]), _ptr(o["inv"]), _ptr(ws), _st()))
        if self.bwd:
            o["d_emb"] = _empty(TAM_N, TAM_W)
            gup = torch.ones((), dtype=torch.float32, device=DEV)
            _ok(_lib().ggad_tam_head_bwd_f32(*args, _ptr(o["a"]), _ptr(o["scal"]), _ptr(o["inv"]), _ptr(gup), _ptr(o["d_emb"]), _ptr(ws), _st()))
        return o

    def tickets_zero(self, ws):
        return int(ws.view(torch.int32)[:64 * ((1 + self.head.n_hub + 63) // 64)].abs().max().item()) == 0

    def check(self, x, got):
        """test_branches_against_float64's bound: 4 x the composed path's own error against float64, or 1e-6 of the magnitude."""
        from ggad_amd import tam_utils as T
        R = self.R
        ref = H.tam_head_fp64(R.indptr, R.indices, R.data, self.adj.r_inv_host, x["e"].cpu().numpy(), self.idx)
        e = x["e"].clone().requires_grad_(True)
        loss, m = T.max_message(e, self.adj, self.idx)
        a = T.inference(e.detach(), self.adj)
        loss.backward()
        comp = dict(a=a, loss=loss.detach(), m=m.detach(), d_emb=e.grad)
        mine = dict(a=got["a"], loss=got["scal"][0], m=got["m"])
        if self.bwd:
            mine["d_emb"] = got["d_emb"]
        for q, v in mine.items():
            want = np.asarray(ref[q], dtype=np.float64)
            err_c = float(np.abs(comp[q].double().cpu().numpy() - want).max())
            err_f = float(np.abs(np.asarray(v, dtype=np.float64) - want).max())
            assert err_f <= max(4.0 * err_c, 1e-6 * float(np.abs(want).max())), (q, err_f, err_c)


class TamBwd(TamFwd):
    """ggad_tam_head_bwd_f32 behind its forward (k_tam_gather, backward form: the hub's three pieces and their wave ticket): d_emb."""
    bwd = True


# ------------------------------------------------------------------------------------------------ the fused GGAD loss block
class FusedLoss:
    """ggad_full_loss_fused_f32 (k_loss_fwd_fused) through `GgadLossFn`, whose kept workspace and ticket are the ones handed in:
    L = 8 + 9 = 17 rows of width 12 (two row-dot workgroups) and 9 rows of emb_con (two partial blocks of 8)."""

    def check_shape(self):
        assert int(_lib().ggad_full_loss_fused_workspace_elems(9, 12)) == 2 * 12

    def inputs(self, k):
        from ggad_amd import fullgraph as FG
        c = C.loss_case(C._loss(40, 12, 8, 9, seed=600 + k))
        ref = C.loss_reference(c, torch.float64)
        C.check_loss_reference(c, ref)
        fa = FG.FullGraphAdj(c["adj_norm"], c["raw"], DEV)
        ls = fa.loss_structs(c["nrm"], c["abn"])
        assert ls["seg_unique"]
        return dict(c=c, ref=ref, fa=fa, ls=ls)

    def workspace(self):
        return _empty(int(_lib().ggad_full_loss_fused_workspace_elems(9, 12)))

    def run(self, x, ws, tick):
        from ggad_amd import fullgraph as FG
        c = x["c"]
        ls = dict(x["ls"], loss_ws_fused=(ws, tick))
        ins = [_f32(c[k]).requires_grad_(True) for k in ("emb", "logits", "con", "eab")]
        out = FG.GgadLossFn.apply(*ins, x["fa"], ls, C.MARGIN)
        assert out[0].grad_fn.fused
        aff = out[0].grad_fn.affinity
        out[0].backward(gradient=torch.full((), C.G_TOTAL, device=DEV))
        return dict(losses=torch.stack([o.detach() for o in out]), aff=aff, d_emb=ins[0].grad, d_logits=ins[1].grad, d_con=ins[2].grad,
                    d_abn=ins[3].grad)

    def check(self, x, got):
        for k, cls in C.LOSS_CLASSES.items():                                                     # test_loss_block
            d = C.distance(got[k], x["ref"][k])
            assert d <= C.BOUND[cls], (k, d, C.BOUND[cls])


# ------------------------------------------------------------------------------------------------ PReLU backward in one launch
PB_M, PB_W = 513, 64


class PreluOne:
    """ggad_prelu_bwd_one_f32 (k_prelu_bwd_one, the fence-free form, both levels): dz, db, da."""

    def check_shape(self):
        s = int(_lib().ggad_prelu_bwd_splits(PB_M))
        assert s > 4 and s % 4 != 0, s                                 # PB_GRP = 4: two first-level groups or more, the last one partial

    def inputs(self, k):
        g = torch.Generator().manual_seed(700 + k)
        return dict(z=(torch.randn(PB_M, PB_W, generator=g) * (1.0 + k)).to(DEV), g=(torch.randn(PB_M, PB_W, generator=g) + 0.1 * k).to(DEV),
                    a=torch.tensor([0.25], device=DEV))

    def workspace(self):
        return _empty(int(_lib().ggad_prelu_bwd_one_workspace_elems(PB_M, PB_W)))

    def run(self, x, ws, tick):
        dz, db, da = _empty(PB_M, PB_W), _empty(PB_W), _empty(1)
        _ok(_lib().ggad_prelu_bwd_one_f32(_ptr(x["g"]), _ptr(x["z"]), _ptr(x["a"]), PB_M, PB_W, _ptr(dz), PB_W, _ptr(db), _ptr(da), _ptr(ws),
                                          _ptr(tick), _st()))
        return dict(dz=dz, db=db, da=da)

    def check(self, x, got):
        z, g = x["z"].cpu().double(), x["g"].cpu().double()
        ref_dz = torch.where(z > 0, g, 0.25 * g)                       # test_prelu_backward_one_launch_same_workspace_changing_data
        ref_da = torch.where(z > 0, torch.zeros_like(g), g * z).sum()
        assert np.array_equal(got["dz"], ref_dz.float().numpy())
        assert np.abs(got["db"] - ref_dz.sum(0).numpy()).max() <= 2e-5 * (1.0 + ref_dz.abs().sum(0).max().item())
        assert abs(float(got["da"][0]) - ref_da.item()) <= 2e-5 * (1.0 + (g * z).abs().sum().item())


ENTRY_POINTS = {"aegis_bn_fwd": BnFwd, "aegis_bn_bwd": BnBwd, "aegis_loss_fwd": AegisLoss, "dominant_ae": DominantAe,
                "dominant_recon": DominantRecon, "tam_head_fwd": TamFwd, "tam_head_bwd": TamBwd, "full_loss_fused": FusedLoss,
                "prelu_bwd_one": PreluOne}


def _host(o):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_four_calls_on_one_workspace_and_the_shared_tickets(name):
    from ggad_amd.fullgraph import ticket_block
    ep = ENTRY_POINTS[name]()
    ep.check_shape()
    block = ticket_block(DEV)
    assert not block.any()
    ws = ep.workspace()
    junk = torch.zeros(8 << 20, device=DEV)
    for k in range(CALLS):
        x = ep.inputs(k)
        got = _host(ep.run(x, ws, block))
        junk.add_(1.0)                                                 # 32 MB of dirty lines between the calls
        own_ws, own_tick = ep.workspace(), torch.zeros_like(block)
        alone = _host(ep.run(x, own_ws, own_tick))
        assert got.keys() == alone.keys()
        for q in got:
            assert not np.isnan(got[q]).any(), (k, q)                  # (the outputs were NaN-filled: every element written)
            assert got[q].tobytes() == alone[q].tobytes(), (k, q)
        ep.check(x, got)
        assert not own_tick.any()
    assert not block.any()
    if hasattr(ep, "tickets_zero"):
        assert ep.tickets_zero(ws)
