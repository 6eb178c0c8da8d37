"""Every full-graph kernel that takes a workspace, held to float64 on DIRTY, REUSED memory (tests/dirty.py; the rule: DESIGN.md 4b).

In production no workspace is ever clean: a captured epoch replays on the same buffers, `fullgraph._XS_WORKSPACE` is one staging
buffer per stream that every SpMM of an epoch shares whatever its width, `Csr` plans keep their `part` buffers, `FullGraphAdj` keeps
`loss_ws`, and memory fresh from the allocator may hold any bit pattern.  The other tests call an entry point once per shape on a
block that is fresh (very often zero) or still holds the previous, correct answer of the same call, so four defects pass them:
an output element that is never stored, a workspace word read before it is written (also when multiplied by a zero weight:
0 * NaN), a smaller call reading the stale tail a larger one left, and an unwritten need for zeroed memory.

Here each entry point runs through the C ABI on a workspace the test owns -- `dirty.run_sequence`: a larger case A, a smaller case B
(smaller in every dimension that sizes the workspace, another width where there is one), A, B, fresh data every call, the workspace
NaN-filled before the first call only, outputs NaN-filled with NaN guards and padding, 32 MB of dirty lines between the calls.
Every call is bit-equal to the same call on a fresh NaN workspace of its own size, leaves no NaN where the header promises a store
and no mark outside, and meets the float64 reference at the tolerance of the entry point's own test (imported, or restated line for
line where that test keeps it inline).  `check_shape` proves the branch each case is there for.  Three wrapper-level tests poison the
production caches themselves."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import dirty as D
import fullgraph_fp64 as C
import gaan_fp64 as GR
import mt_randn_ref as MR

pytestmark = pytest.mark.gpu

DEV = D.DEV
NAN = float("nan")


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


def _ok(rc):
    assert rc == 0, (rc, _lib().ggad_last_error())


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ 1, 2: GEMM split-K, tiled / LDS-DMA
def _gemm_splits(M, N, K):
    """`gemm_splits` of csrc/gemm.hip restated (64 x 64 tiles): (splits, K per split rounded up to BK = 32)."""
    tiles = _cdiv(M, 64) * _cdiv(N, 64)
    if K < 512 or tiles >= 256:
        return 1, K
    splits = max(1, min(512 // tiles, _cdiv(K, 256) if K >= 2048 else _cdiv(K, 128), 128))
    return splits, _cdiv(_cdiv(K, splits), 32) * 32


class Gemm:
    """ggad_gemm_f32 through split-K (k_gemm_f32 or k_gemm_dma, then k_splitk_reduce) with bias + ReLU into a row-strided C."""

    def __init__(self, trans_b, dma):
        self.tb, self.dma = trans_b, dma
        self.shape = {"A": (1088, 128, 1932 if dma else 1930), "B": (64, 64, 520 if dma else 522)}

    def check_shape(self):
        assert os.environ.get("GGAD_GEMM_TM") is None and os.environ.get("GGAD_GEMM_SPLIT_TARGET") is None
        assert os.environ.get("GGAD_GEMM_DMA") != "0"
        want = {"A": (15, 2), "B": (5, 0)}                             # (splits, splits that start at or behind K)
        for case, (M, N, K) in self.shape.items():
            splits, kps = _gemm_splits(M, N, K)
            empty = sum(1 for s in range(splits) if s * kps >= K)
            assert (splits, empty) == want[case], (case, splits, kps, empty)
            assert int(_lib().ggad_gemm_workspace_elems(M, N, K)) == splits * M * N
            # the launcher's condition for k_gemm_dma (NN: A k-fast, B n-fast; NT: both k-fast): whole 16-byte chunks inside one row
            a_ok = K % 4 == 0
            b_ok = (K % 4 == 0) if self.tb else (N % 4 == 0)
            assert (a_ok and b_ok and K >= 32) == self.dma

    def inputs(self, case, k):
        M, N, K = self.shape[case]
        rng = np.random.default_rng(1000 + 10 * k + self.tb)
        return dict(case=case, a=_f32(rng.standard_normal((M, K))), b=_f32(rng.standard_normal((N, K) if self.tb else (K, N))),
                    bias=_f32(rng.standard_normal(N)))

    def workspace(self, case):
        return D.nan_like(int(_lib().ggad_gemm_workspace_elems(*self.shape[case])))

    def run(self, x, ws):
        M, N, K = self.shape[x["case"]]
        c = D.padded(M, N, N + 4)
        sbk, sbn = (1, K) if self.tb else (N, 1)
        _ok(_lib().ggad_gemm_f32(_ptr(x["a"]), _ptr(x["b"]), c.data_ptr(), M, N, K, K, 1, sbk, sbn, N + 4, _ptr(x["bias"]), 1, _ptr(ws), _st()))
        return dict(c=c)

    def check(self, x, got):
        b = x["b"].cpu().numpy().astype(np.float64)
        ref = x["a"].cpu().numpy().astype(np.float64) @ (b.T if self.tb else b)
        scale = np.abs(ref).max() + 1.0                                                          # test_gemm_f32_all_layouts
        assert np.abs(got["c"] - np.maximum(ref + x["bias"].cpu().numpy(), 0)).max() / scale < 2e-6


# ------------------------------------------------------------------------------------------------ 3: the row-range kernel of mlp.hip
class GemmTN:
    """ggad_gemm_f32, "TN" without epilogue and K long: k_mlp_wgrad over row ranges + k_mlp_wgrad_reduce (ggad_int_wgrad_tn)."""
    shape = {"A": (20, 300, 1500), "B": (10, 64, 1024)}

    def check_shape(self):
        assert os.environ.get("GGAD_GEMM_WGRAD_TN") != "0"
        for case, (M, N, K) in self.shape.items():
            splits, _ = _gemm_splits(M, N, K)
            assert K >= 1024 and min(M, N) <= 32 and max(M, N) <= 512                            # what ggad_int_wgrad_tn_ws takes
            ranges = min(max(1, K // 64), 64)
            tn = ranges * M * N + 16
            assert splits > 1 and tn > splits * M * N
            assert int(_lib().ggad_gemm_workspace_elems(M, N, K)) == max(splits * M * N, tn)
        assert min(max(1, 1500 // 64), 64) != min(max(1, 1024 // 64), 64)                      # another number of ranges in B

    def inputs(self, case, k):
        M, N, K = self.shape[case]
        rng = np.random.default_rng(1100 + k)
        return dict(case=case, a=_f32(rng.standard_normal((K, M))), b=_f32(rng.standard_normal((K, N))))

    def workspace(self, case):
        return D.nan_like(int(_lib().ggad_gemm_workspace_elems(*self.shape[case])))

    def run(self, x, ws):
        M, N, K = self.shape[x["case"]]
        c = D.nan_like(M, N)
        assert ws.data_ptr() % 16 == 0
        _ok(_lib().ggad_gemm_f32(_ptr(x["a"]), _ptr(x["b"]), _ptr(c), M, N, K, 1, M, N, 1, N, 0, 0, _ptr(ws), _st()))
        return dict(c=c)

    def check(self, x, got):
        ref = x["a"].cpu().numpy().astype(np.float64).T @ x["b"].cpu().numpy().astype(np.float64)
        assert np.abs(got["c"] - ref).max() / (np.abs(ref).max() + 1.0) < 2e-6                  # test_gemm_f32_all_layouts


# ------------------------------------------------------------------------------------------------ 4: the scorer's weight gradients
class ScoreWgrad:
    """ggad_mlp_score_wgrad_f32: dW1 = dz1^T x, dW2 = dz2^T f1, dW3 = g3^T f2 over R rows; x row-strided with NaN padding."""
    shape = {"A": (1203, 300), "B": (37, 64)}

    def _dims(self, case):
        r, h = self.shape[case]
        return r, h, h // 2, h // 4

    def check_shape(self):
        for case in self.shape:
            r, h, h1, h2 = self._dims(case)
            assert int(_lib().ggad_mlp_score_supported(h, h1, h2)) == 1
            ranges = min(max(1, r // 64), 64)                                                     # wg_splits of csrc/mlp.hip
            assert int(_lib().ggad_mlp_score_wgrad_workspace_elems(r, h, h1, h2)) == ranges * (h1 * h + h2 * h1 + h2) + 16
        assert min(max(1, 1203 // 64), 64) == 18 and min(max(1, 37 // 64), 64) == 1

    def inputs(self, case, k):
        r, h, h1, h2 = self._dims(case)
        rng = np.random.default_rng(1200 + k)
        xs = D.padded(r, h, h + 4)
        xs.copy_(_f32(rng.standard_normal((r, h))))
        return dict(case=case, x=xs, dz1=_f32(rng.standard_normal((r, h1))), f1=_f32(rng.standard_normal((r, h1))),
                    dz2=_f32(rng.standard_normal((r, h2))), f2=_f32(rng.standard_normal((r, h2))), g3=_f32(rng.standard_normal((r, 1))))

    def workspace(self, case):
        return D.nan_like(int(_lib().ggad_mlp_score_wgrad_workspace_elems(*self._dims(case))))

    def run(self, x, ws):
        r, h, h1, h2 = self._dims(x["case"])
        o = dict(dw1=D.nan_like(h1, h), dw2=D.nan_like(h2, h1), dw3=D.nan_like(1, h2))
        _ok(_lib().ggad_mlp_score_wgrad_f32(x["x"].data_ptr(), h + 4, _ptr(x["dz1"]), _ptr(x["f1"]), _ptr(x["dz2"]), _ptr(x["f2"]), _ptr(x["g3"]),
                                            r, h, h1, h2, _ptr(o["dw1"]), _ptr(o["dw2"]), _ptr(o["dw3"]), _ptr(ws), _st()))
        D.guards_intact(x["x"])                                                                   # (the operand's padding still holds NaN)
        return o

    def check(self, x, got):
        for name, p, q in (("dw1", "dz1", "x"), ("dw2", "dz2", "f1"), ("dw3", "g3", "f2")):
            ref = (x[p].double().T @ x[q].double()).cpu().numpy()
            assert np.abs(got[name] - ref).max() / (np.abs(ref).max() + 1.0) < 2e-6, name       # test_fused_scorer_mlp_weight_gradients


# ------------------------------------------------------------------------------------------------ 5: PReLU backward in two launches
class PreluTwo:
    """ggad_prelu_bwd_ld_f32 / ggad_prelu_bwd_f32: k_prelu_bwd_v4 (vector) or k_prelu_bwd (scalar), then k_prelu_bwd_final."""

    def __init__(self, vector, sums=True):
        self.vector, self.sums = vector, sums
        self.shape = {"A": (513, 64), "B": (5, 12)} if vector else {"A": (513, 30), "B": (7, 6)}
        self.pad = 4 if vector else 0                                  # (the scalar kernel writes dense rows)

    def _ws_elems(self, case):
        M, W = self.shape[case]
        return 2 * int(_lib().ggad_prelu_bwd_splits(M)) * W

    def check_shape(self):
        # the launcher's condition for the vector kernel; the 16-byte alignment of g, z, dz and the workspace is asserted in run()
        for case, (M, W) in self.shape.items():
            S = int(_lib().ggad_prelu_bwd_splits(M))
            assert S == min(max(_cdiv(M, 64), 1), 256)
            assert (W % 4 == 0 and (W + self.pad) % 4 == 0 and W <= 1024 and (S * W) % 4 == 0) == self.vector, case
        assert int(_lib().ggad_prelu_bwd_splits(self.shape["A"][0])) > int(_lib().ggad_prelu_bwd_splits(self.shape["B"][0]))

    def inputs(self, case, k):
        M, W = self.shape[case]
        g = torch.Generator().manual_seed(1300 + k)
        return dict(case=case, z=(torch.randn(M, W, generator=g) * (1.0 + k)).to(DEV), g=(torch.randn(M, W, generator=g) + 0.1 * k).to(DEV),
                    a=torch.tensor([0.25], device=DEV))

    def workspace(self, case):
        return D.nan_like(self._ws_elems(case))

    def run(self, x, ws):
        M, W = self.shape[x["case"]]
        o = dict(dz=D.padded(M, W, W + self.pad))
        if self.sums:
            o.update(db=D.nan_like(W), da=D.nan_like(1))
        db, da = (_ptr(o["db"]), _ptr(o["da"])) if self.sums else (0, 0)
        assert all(p % 16 == 0 for p in (x["g"].data_ptr(), x["z"].data_ptr(), o["dz"].data_ptr(), ws.data_ptr()))
        if self.pad:
            _ok(_lib().ggad_prelu_bwd_ld_f32(_ptr(x["g"]), _ptr(x["z"]), _ptr(x["a"]), M, W, o["dz"].data_ptr(), W + self.pad, db, da, _ptr(ws),
                                             _st()))
        else:
            _ok(_lib().ggad_prelu_bwd_f32(_ptr(x["g"]), _ptr(x["z"]), _ptr(x["a"]), M, W, o["dz"].data_ptr(), db, da, _ptr(ws), _st()))
        return o

    def check(self, x, got):
        z, g = x["z"].cpu().double(), x["g"].cpu().double()
        ref_dz = torch.where(z > 0, g, 0.25 * g)                       # test_prelu_backward_kernel_against_autograd
        assert np.array_equal(got["dz"], ref_dz.float().numpy())
        if self.sums:
            ref_da = torch.where(z > 0, torch.zeros_like(g), g * z).sum()
            assert np.abs(got["db"] - ref_dz.sum(0).numpy()).max() <= 2e-5 * (1.0 + ref_dz.abs().sum(0).max().item())
            assert abs(float(got["da"][0]) - ref_da.item()) <= 2e-5 * (1.0 + (g * z).abs().sum().item())


# ------------------------------------------------------------------------------------------------ 6: the unfused loss block
class FullLoss:
    """ggad_full_loss_f32 (k_full_loss, k_rec_part, k_rec_apply) on the loss cases with the most and the fewest rows of emb_con; the
    affinity vector it reads is the float64 reference's, rounded."""
    name = {"A": "A3000_H300", "B": "A1_H64"}

    def check_shape(self):
        na = [p["na"] for p in C.LOSS_CASES.values() if not p.get("refused")]
        assert C.LOSS_CASES[self.name["A"]]["na"] == max(na) and C.LOSS_CASES[self.name["B"]]["na"] == min(na)
        for case, name in self.name.items():
            p = C.LOSS_CASES[name]
            assert int(_lib().ggad_full_loss_workspace_elems(p["na"], p["h"])) == _cdiv(p["na"], 8) * p["h"]      # REC_ROWS = 8

    def inputs(self, case, k):
        p = dict(C.LOSS_CASES[self.name[case]])
        p["seed"] += 1000 * (k // 2)                                   # fresh data at the second visit of a case
        c = C.loss_case(p)
        ref = C.loss_reference(c, torch.float64)
        C.check_loss_reference(c, ref)
        return dict(case=case, c=c, ref=ref, logits=_f32(c["logits"]), aff=_f32(ref["aff"]), con=_f32(c["con"]), eab=_f32(c["eab"]))

    def workspace(self, case):
        p = C.LOSS_CASES[self.name[case]]
        return D.nan_like(int(_lib().ggad_full_loss_workspace_elems(p["na"], p["h"])))

    def run(self, x, ws):
        c = x["c"]
        nn_, na, h = len(c["nrm"]), len(c["abn"]), c["h"]
        o = dict(losses=D.nan_like(4), d_logits=D.nan_like(nn_ + na), g_aff=D.nan_like(nn_ + na), dD=D.nan_like(na, h))
        _ok(_lib().ggad_full_loss_f32(_ptr(x["logits"]), _ptr(x["aff"]), nn_, na, _ptr(x["con"]), _ptr(x["eab"]), h, C.MARGIN, _ptr(o["losses"]),
                                      _ptr(o["d_logits"]), _ptr(o["g_aff"]), _ptr(o["dD"]), _ptr(ws), _st()))
        return o

    def check(self, x, got):
        ref, g = x["ref"], C.G_TOTAL                                   # test_loss_block's classes and bounds
        assert C.distance(got["losses"], ref["losses"]) <= C.BOUND[C.LOSS]
        assert C.distance(got["d_logits"].astype(np.float64) * g, ref["d_logits"]) <= C.BOUND[C.DGRAD]
        assert C.distance(got["dD"].astype(np.float64) * g, ref["d_con"]) <= C.BOUND[C.DGRAD]
        assert C.distance(got["dD"].astype(np.float64) * -g, ref["d_abn"]) <= C.BOUND[C.DGRAD]
        nn_ = len(x["c"]["nrm"])                                       # the hinge is active in both cases (check_loss_reference)
        assert np.array_equal(got["g_aff"][:nn_], np.full(nn_, -1.0 / nn_, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ 7, 8: SpMM with partial sums
def _sparse_case(n, full_rows, empty_rows, seed):
    rng = np.random.default_rng(seed)
    a = sp.random(n, n, density=8.0 / n, random_state=seed, format="lil", dtype=np.float32)
    for r in full_rows:
        a[r, :] = rng.standard_normal(n).astype(np.float32)
    for r in empty_rows:
        a[r, :] = 0
    return a.tocsr()


class SpmmSeg:
    """ggad_spmm_csr_f32 (k_spmm_seg + k_spmm_combine over `part`) with bias + PReLU + out_pre into row-strided outputs."""
    mats = {"A": (600, (100, 400), (7, 8, 599), 300), "B": (300, (5,), (9,), 28)}
    entry = "ggad_spmm_csr_f32"

    def _plan(self, csr):
        return csr.plan()

    def check_shape(self):
        from ggad_amd import fullgraph as FG
        assert os.environ.get("GGAD_SPMM_COL_RANGES") is None
        self.csr, self.plan, self.w = {}, {}, {}
        for case, (n, full, empty, w) in self.mats.items():
            csr = FG.Csr(_sparse_case(n, full, empty, 21), DEV)
            deg = np.diff(csr.host.indptr)
            assert (deg == 0).sum() >= len(empty) and (deg == n).sum() == len(full)
            self.csr[case], self.plan[case], self.w[case] = csr, self._plan(csr), w
        pa, pb = self.plan["A"], self.plan["B"]
        assert pa["n_multi"] > 0 and int((pa["seg_out"] < 0).sum().item()) >= 2 * pa["n_multi"]
        assert pb["n_seg"] < pa["n_seg"] and self.w["B"] < self.w["A"]
        empty_seg = (pa["seg_end"] - pa["seg_beg"] == 0)
        assert int(empty_seg.sum().item()) >= 3 and bool((pa["seg_out"][empty_seg] >= 0).all())  # an empty row = one empty segment, stored in place

    def inputs(self, case, k):
        rng = np.random.default_rng(1400 + k)
        n, w = self.csr[case].shape[1], self.w[case]
        return dict(case=case, x=_f32(rng.standard_normal((n, w))), bias=_f32(rng.standard_normal(w)), slope=torch.tensor([0.25], device=DEV))

    def workspace(self, case):
        p = self.plan[case]
        return D.nan_like(p["n_seg"] * self.w[case]) if p["n_multi"] > 0 else None

    def _launch(self, csr, p, x, w, opt, ws):
        _ok(_lib().ggad_spmm_csr_f32(_ptr(csr.col), _ptr(csr.val), _ptr(p["seg_beg"]), _ptr(p["seg_end"]), _ptr(p["seg_out"]), p["n_seg"],
                                     _ptr(p["multi_row"]), _ptr(p["multi_first"]), _ptr(p["multi_count"]), p["n_multi"], _ptr(x["x"]), w, w,
                                     *opt, _ptr(ws), _st()))

    def run(self, x, ws):
        case = x["case"]
        csr, p, w = self.csr[case], self.plan[case], self.w[case]
        o = dict(out=D.padded(p["n_out"], w, w + 4), pre=D.padded(p["n_out"], w, w + 4))
        self._launch(csr, p, x, w, (_ptr(x["bias"]), _ptr(x["slope"]), o["out"].data_ptr(), w + 4, o["pre"].data_ptr()), ws)
        return o

    def check(self, x, got):
        csr = self.csr[x["case"]]
        ref = csr.host.astype(np.float64) @ x["x"].cpu().numpy().astype(np.float64) + x["bias"].cpu().numpy().astype(np.float64)
        scale = np.abs(ref).max() + 1.0                                                          # test_spmm_launches_the_kernel_its_route_names
        assert np.abs(got["pre"] - ref).max() / scale < 2e-6
        assert np.abs(got["out"] - np.where(ref > 0, ref, 0.25 * ref)).max() / scale < 2e-6


class SpmmSliced(SpmmSeg):
    """ggad_spmm_sliced_f32 (k_slice_major into `xs_workspace`, k_spmm_sliced, k_spmm_combine over `part`) on the same matrices through
    `Csr.sliced_plan`; W = 300 (ten slices, three lanes of the last one used), then 36 (two slices, one lane of the second used)."""
    mats = {"A": (600, (100, 400), (7, 8, 599), 300), "B": (300, (5,), (9,), 36)}

    def _plan(self, csr):
        return csr.sliced_plan(csr.plan())

    def check_shape(self):
        SpmmSeg.check_shape(self)
        seg = int(_lib().ggad_spmm_sliced_seg_len())
        assert 300 < seg < 600 and self.plan["B"]["n_multi"] == 0                                # two pieces per full row of A, none in B
        for case, w in self.w.items():
            n = self.csr[case].shape[1]
            assert (w // 4) % 8 != 0                                                             # the last slice is partial: zero-filled lanes
            assert int(_lib().ggad_spmm_sliced_workspace_elems(n, w)) == n * _cdiv(w // 4, 8) * 8 * 4

    def workspace(self, case):
        n, w = self.csr[case].shape[1], self.w[case]
        return (D.nan_like(int(_lib().ggad_spmm_sliced_workspace_elems(n, w))), SpmmSeg.workspace(self, case))

    def _launch(self, csr, p, x, w, opt, ws):
        _ok(_lib().ggad_spmm_sliced_f32(_ptr(csr.col), _ptr(csr.val), _ptr(p["seg_beg"]), _ptr(p["seg_end"]), _ptr(p["seg_out"]), p["n_seg"],
                                        _ptr(p["multi_row"]), _ptr(p["multi_first"]), _ptr(p["multi_count"]), p["n_multi"], _ptr(x["x"]), w, w,
                                        csr.shape[1], _ptr(ws[0]), *opt, _ptr(ws[1]), _st()))


# ------------------------------------------------------------------------------------------------ 9, 10: the LDS panel and ring products
class SpmmPanel(SpmmSeg):
    """ggad_spmm_panel_f32 (k_slice_major into `xs_workspace`, k_spmm_panel): 0/1 pattern matrices shorter than one panel."""
    mats = {"A": (900, 900, 0.2, 64), "B": (150, 200, 0.5, 36)}
    kind = "panel"

    def check_shape(self):
        from ggad_amd import fullgraph as FG
        lib = _lib()
        assert int(lib.ggad_spmm_panel_available()) == 1 and int(lib.ggad_spmm_ring_available()) == 1
        self.csr, self.plan, self.w = {}, {}, {}
        for case, (n_rows, n_src, dens, w) in self.mats.items():
            a = sp.random(n_rows, n_src, density=dens, random_state=7, format="csr", dtype=np.float32)   # test_spmm_launches_the_kernel_its_route_names
            a.data[:] = 1.0
            csr = FG.Csr(a, DEV)
            plan = (csr.panel_plan if self.kind == "panel" else csr.ring_plan)(_cdiv(w // 4, 8))
            assert plan is not None
            self.csr[case], self.plan[case], self.w[case] = csr, plan, w
            if self.kind == "panel":
                assert plan["n_chunks"] == 1 and n_src % int(lib.ggad_spmm_panel_rows()) != 0    # one panel, partial
            else:
                rs = int(lib.ggad_spmm_ring_slot_rows())
                assert plan["n_phases"] == _cdiv(n_src, rs) and n_src % rs != 0                  # the last phase stages a partial slot
        assert self.plan["A"]["n_phases" if self.kind == "ring" else "n_chunks"] >= self.plan["B"]["n_phases" if self.kind == "ring" else "n_chunks"]
        assert (self.w["B"] // 4) % 8 != 0

    def workspace(self, case):
        n, w = self.csr[case].shape[1], self.w[case]
        return D.nan_like(int(_lib().ggad_spmm_sliced_workspace_elems(n, w)))

    def run(self, x, ws):
        case = x["case"]
        csr, pp, w = self.csr[case], self.plan[case], self.w[case]
        n_out = csr.shape[0]
        o = dict(out=D.padded(n_out, w, w + 4), pre=D.padded(n_out, w, w + 4))
        opt = (_ptr(x["bias"]), _ptr(x["slope"]), o["out"].data_ptr(), w + 4, o["pre"].data_ptr())
        if self.kind == "panel":
            _ok(_lib().ggad_spmm_panel_f32(_ptr(pp["wg"]), pp["n_wg"], _ptr(pp["dir"]), _ptr(pp["stream"]), _ptr(pp["row_tab"]), pp["n_chunks"],
                                           _ptr(pp["cs"]), _ptr(pp["rs"]), _ptr(pp["diag"]), _ptr(x["x"]), w, w, csr.shape[1], _ptr(ws), *opt, _st()))
        else:
            _ok(_lib().ggad_spmm_ring_f32(_ptr(pp["wg"]), pp["n_wg"], _ptr(pp["wave_sb"]), _ptr(pp["idx"]), _ptr(pp["ctl"]), _ptr(pp["row_tab"]),
                                          pp["n_phases"], pp["walkers"], _ptr(pp["cs"]), _ptr(pp["rs"]), _ptr(pp["diag"]), _ptr(x["x"]), w, w,
                                          csr.shape[1], _ptr(ws), *opt, _st()))
        return o


class SpmmRing(SpmmPanel):
    """ggad_spmm_ring_f32 (k_slice_major into `xs_workspace`, k_spmm_ring) on the same two matrices: three phases, then one."""
    kind = "ring"


# ------------------------------------------------------------------------------------------------ 11: AnomalyDAE column sums
class AdaeColsum:
    """ggad_adae_colsum_f32 (k_colsum_part over fixed row ranges, k_colsum_fin), with and without the row weights."""
    shape = {"A": (1000, 93), "B": (17, 10)}

    def __init__(self, weighted):
        self.weighted = weighted

    def check_shape(self):
        parts = int(_lib().ggad_adae_colsum_workspace_elems(1))
        assert parts > 17                                              # B: most row ranges are empty and still store their zero
        for n, f in self.shape.values():
            assert int(_lib().ggad_adae_colsum_workspace_elems(f)) == parts * f

    def inputs(self, case, k):
        n, f = self.shape[case]
        rng = np.random.default_rng(1500 + k)
        return dict(case=case, m=_f32(rng.standard_normal((n, f))), w=_f32(rng.standard_normal(n)) if self.weighted else None)

    def workspace(self, case):
        return D.nan_like(int(_lib().ggad_adae_colsum_workspace_elems(self.shape[case][1])))

    def run(self, x, ws):
        n, f = self.shape[x["case"]]
        o = dict(out=D.nan_like(f))
        _ok(_lib().ggad_adae_colsum_f32(_ptr(x["m"]), _ptr(x["w"]), n, f, _ptr(o["out"]), _ptr(ws), _st()))
        return o

    def check(self, x, got):
        m = x["m"].cpu().numpy().astype(np.float64)
        ref = (m * x["w"].cpu().numpy().astype(np.float64)[:, None]).sum(0) if self.weighted else m.sum(0)
        # the bias / attention gradients of test_gat_forward_backward_vs_float64 are these sums
        np.testing.assert_allclose(got["out"], ref, rtol=2e-4, atol=2e-5 * (np.abs(ref).max() + 1))


# ------------------------------------------------------------------------------------------------ 12, 13: AnomalyDAE reconstruction loss
class AdaeStru:
    """ggad_adae_stru_fwd_f32, then ggad_adae_stru_bwd_f32 and ggad_adae_attr_bwd_f32 from its outputs, at two shapes of
    test_recon_loss_forward_backward_vs_float64: every row of dz written, only the listed rows of dxhat touched."""
    shape = {"A": (301, 70, 93, 0.15), "B": (97, 15, 25, 3.0)}         # n, n_rows, F, scale of z
    G = 2.5

    def check_shape(self):
        lib = _lib()
        a, b = self.shape["A"], self.shape["B"]
        assert int(lib.ggad_adae_stru_fwd_workspace_elems(a[1], a[0])) > int(lib.ggad_adae_stru_fwd_workspace_elems(b[1], b[0])) > 0
        assert int(lib.ggad_adae_stru_bwd_workspace_elems(a[1], a[0], a[2])) > int(lib.ggad_adae_stru_bwd_workspace_elems(b[1], b[0], b[2])) > 0

    def inputs(self, case, k):
        from ggad_amd.model_anomalydae import row_structs
        from test_anomalydae_gpu import _full, _rand_adj
        n, n_rows, f, scale = self.shape[case]
        rng = np.random.default_rng(1600 + k)
        a = _rand_adj(n, n_rows + k)
        rows = np.concatenate([[n - 2, n - 1], rng.permutation(n - 2)])[:n_rows].astype(np.int64)
        return dict(case=case, a=a, rows=rows, rs=row_structs(_full(a), rows), z=_f32(rng.standard_normal((n, f)) * scale),
                    x=_f32(rng.random((n, f))), xh=_f32(rng.standard_normal((n, f))), g=torch.tensor([self.G], device=DEV))

    def workspace(self, case):
        n, n_rows, f, _ = self.shape[case]
        return (D.nan_like(int(_lib().ggad_adae_stru_fwd_workspace_elems(n_rows, n))),
                D.nan_like(int(_lib().ggad_adae_stru_bwd_workspace_elems(n_rows, n, f))))

    def run(self, x, ws):
        n, nr, f, _ = self.shape[x["case"]]
        rs = x["rs"]
        o = dict(s_edge=D.nan_like(max(rs["nnz"], 1)), attr=D.nan_like(nr), stru=D.nan_like(nr), score=D.nan_like(nr), loss=D.nan_like(1),
                 dz=D.nan_like(n, f), dxhat=D.nan_like(n, f))
        lib = _lib()
        _ok(lib.ggad_adae_stru_fwd_f32(_ptr(x["z"]), n, f, _ptr(rs["rows"]), nr, _ptr(rs["rptr"]), _ptr(rs["rcol"]), _ptr(rs["rval"]), _ptr(x["x"]),
                                       _ptr(x["xh"]), _ptr(ws[0]), _ptr(o["s_edge"]), _ptr(o["attr"]), _ptr(o["stru"]), _ptr(o["score"]),
                                       _ptr(o["loss"]), _st()))
        _ok(lib.ggad_adae_stru_bwd_f32(_ptr(x["z"]), n, f, _ptr(rs["rows"]), nr, _ptr(rs["rptr"]), _ptr(rs["rcol"]), _ptr(rs["rval"]),
                                       _ptr(o["s_edge"]), _ptr(rs["pos"]), _ptr(rs["tptr"]), _ptr(rs["trow"]), _ptr(rs["tedge"]), _ptr(o["stru"]),
                                       _ptr(x["g"]), _ptr(ws[1]), _ptr(o["dz"]), _st()))
        _ok(lib.ggad_adae_attr_bwd_f32(_ptr(x["x"]), _ptr(x["xh"]), _ptr(rs["rows"]), nr, f, _ptr(o["attr"]), _ptr(x["g"]), _ptr(o["dxhat"]), _st()))
        return o

    def untouched(self, x, name):
        if name != "dxhat":
            return None
        n, _, f, _ = self.shape[x["case"]]
        keep = np.ones((n, f), dtype=bool)
        keep[x["rows"]] = False
        return keep

    def check(self, x, got):
        z64 = x["z"].cpu().double().requires_grad_(True)               # test_recon_loss_forward_backward_vs_float64
        xh64 = x["xh"].cpu().double().requires_grad_(True)
        A, r = torch.from_numpy(x["a"]), torch.from_numpy(x["rows"])
        s_ = torch.sigmoid(z64 @ z64.T)
        attr = torch.sqrt(torch.sum((x["x"].cpu().double()[r] - xh64[r]) ** 2, 1))
        stru = torch.sqrt(torch.sum((A[r] - s_[r]) ** 2, 1))
        sc = 0.5 * attr + 0.5 * stru
        ref = sc.mean()
        (self.G * ref).backward()
        assert abs(float(got["loss"][0]) - ref.item()) < 2e-6 * (1 + abs(ref.item()))
        np.testing.assert_allclose(got["score"], sc.detach().numpy(), rtol=2e-6, atol=2e-5)
        gz = z64.grad.numpy()
        np.testing.assert_allclose(got["dz"], gz, rtol=2e-4, atol=1e-5 * (np.abs(gz).max() + 1e-3))
        rows = x["rows"]
        np.testing.assert_allclose(got["dxhat"][rows], xh64.grad.numpy()[rows], rtol=1e-5, atol=1e-8)


# ------------------------------------------------------------------------------------------------ 14: the GAAN edge loss
_GAAN = {}


def _gaan_case(kind):
    if kind not in _GAAN:
        from ggad_amd.fullgraph import FullGraphAdj
        from ggad_amd.model_gaan import edge_list, edge_structs
        from test_gaan_gpu import _pattern
        a, idx = _pattern(kind)
        es = edge_structs(FullGraphAdj(a, a, DEV), idx)
        erow, ecol, _ = edge_list(a, idx)
        _GAAN[kind] = (a.shape[0], es, erow, ecol)
    return _GAAN[kind]


class GaanEdge:
    """ggad_gaan_edge_fwd_f32 (k_gaan_fwd, k_gaan_fwd_final over `ws`) and ggad_gaan_edge_bwd_f32 from its `a`, on the edge sets of
    test_edge_loss_vs_float64_at_every_branch: all rows, then a subset (fewer entries, fewer workgroup partials)."""
    kind = {"A": "all", "B": "subset"}
    G = 1.7

    def check_shape(self):
        ma, mb = _gaan_case("all")[1]["m"], _gaan_case("subset")[1]["m"]
        lib = _lib()
        assert ma > mb > 0 and int(lib.ggad_gaan_edge_fwd_workspace_elems(ma)) >= int(lib.ggad_gaan_edge_fwd_workspace_elems(mb)) >= 4

    def inputs(self, case, k):
        from test_gaan_gpu import _emb
        n, es, erow, ecol = _gaan_case(self.kind[case])
        rng = np.random.default_rng(1700 + k)
        return dict(case=case, emb=_f32(_emb(n, rng, 0.25)), z=_f32(_emb(n, rng, 0.6)), g=torch.tensor([self.G], device=DEV))

    def workspace(self, case):
        return D.nan_like(int(_lib().ggad_gaan_edge_fwd_workspace_elems(_gaan_case(self.kind[case])[1]["m"])))

    def run(self, x, ws):
        n, es, _, _ = _gaan_case(self.kind[x["case"]])
        c = int(_lib().ggad_gaan_edge_channels())
        o = dict(vals=D.nan_like(3), a=D.nan_like(es["m"]), dE=D.nan_like(n, c))
        _ok(_lib().ggad_gaan_edge_fwd_f32(_ptr(x["emb"]), _ptr(x["z"]), n, c, _ptr(es["erow"]), _ptr(es["ecol"]), es["m"], _ptr(o["a"]), _ptr(ws),
                                          _ptr(o["vals"]), _st()))
        _ok(_lib().ggad_gaan_edge_bwd_f32(_ptr(x["emb"]), n, c, _ptr(es["pos"]), _ptr(es["rptr"]), _ptr(es["ecol"]), _ptr(es["tptr"]),
                                          _ptr(es["trow"]), _ptr(es["tedge"]), _ptr(o["a"]), es["m"], _ptr(x["g"]), _ptr(es["small"]), es["n_small"],
                                          _ptr(es["big"]), es["n_big"], _ptr(o["dE"]), _st()))
        return o

    def check(self, x, got):
        _, _, erow, ecol = _gaan_case(self.kind[x["case"]])
        loss, lf, lr, dE = GR.edge_loss_ref(x["emb"].cpu().numpy(), x["z"].cpu().numpy(), erow, ecol, g=self.G)
        v = got["vals"]                                                # test_edge_loss_vs_float64_at_every_branch
        assert abs(v[0] - loss) <= 2e-5 * abs(loss) and abs(v[1] - lf) <= 2e-5 * abs(lf) and abs(v[2] - lr) <= 2e-5 * abs(lr)
        np.testing.assert_allclose(got["dE"], dE, rtol=1e-4, atol=1e-5 * np.abs(dE).max())


# ------------------------------------------------------------------------------------------------ 15: the AEGIS loss backward
class AegisLossBwd:
    """ggad_aegis_loss_bwd_f32 (no workspace): dp, and dzd with EVERY element written -- zero on the rows that are not listed and in
    the padding columns -- at two sizes of test_losses_vs_float64."""
    shape = {"A": (293, 93, 57), "B": (301, 10, 301)}                  # n, F, listed rows

    def check_shape(self):
        assert all((f + 3) // 4 * 4 > f for _, f, _ in self.shape.values())                      # padding columns in both

    def inputs(self, case, k):
        n, f, nr = self.shape[case]
        rng = np.random.default_rng(1800 + k)
        fp = (f + 3) // 4 * 4
        rows = rng.permutation(n)[:nr]
        pos = np.full(n, -1, dtype=np.int32)
        pos[rows] = np.arange(nr, dtype=np.int32)
        p = rng.uniform(0.01, 0.99, n).astype(np.float32)
        p[:3] = [0.0, 1.0 - 1e-8, 0.5]
        zd = np.zeros((n, fp), dtype=np.float32)
        zd[:, :f] = rng.random((n, f))
        x = rng.random((n, f)).astype(np.float32)
        attr = np.sqrt(((x[rows].astype(np.float64) - zd[rows, :f]) ** 2).sum(1))
        return dict(case=case, rows=rows, pos=torch.from_numpy(pos).to(DEV), p=_f32(p), zd=_f32(zd), x=_f32(x), attr=_f32(attr),
                    gg=torch.tensor([2.0], device=DEV), ga=torch.tensor([3.0], device=DEV))

    def workspace(self, case):
        return None

    def run(self, x, ws):
        n, f, nr = self.shape[x["case"]]
        fp = (f + 3) // 4 * 4
        o = dict(dp=D.nan_like(n), dzd=D.nan_like(n, fp))
        _ok(_lib().ggad_aegis_loss_bwd_f32(_ptr(x["p"]), n, _ptr(x["gg"]), _ptr(o["dp"]), _ptr(x["x"]), f, _ptr(x["zd"]), fp, _ptr(x["pos"]), nr,
                                           _ptr(x["attr"]), _ptr(x["ga"]), _ptr(o["dzd"]), _st()))
        return o

    def check(self, x, got):
        n, f, nr = self.shape[x["case"]]
        p64 = x["p"].cpu().double().requires_grad_(True)               # test_losses_vs_float64
        z64 = x["zd"].cpu().double().requires_grad_(True)
        r = torch.from_numpy(x["rows"])
        lg64 = torch.nn.functional.binary_cross_entropy(p64, torch.zeros_like(p64))
        la64 = torch.mean(torch.sqrt(torch.sum((x["x"].cpu().double()[r] - z64[r, :f]) ** 2, 1)))
        torch.autograd.backward([2.0 * lg64, 3.0 * la64])
        np.testing.assert_allclose(got["dp"], p64.grad.numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(got["dzd"], z64.grad.numpy(), rtol=1e-5, atol=1e-7)
        unlisted = np.setdiff1d(np.arange(n), x["rows"])
        assert not np.any(got["dzd"][:, f:]) and not np.any(got["dzd"][unlisted])               # exact zeros, as the header states


ENTRY_POINTS = {
    "gemm_splitk_tiled_nn": lambda: Gemm(False, False), "gemm_splitk_tiled_nt": lambda: Gemm(True, False),
    "gemm_splitk_dma_nn": lambda: Gemm(False, True), "gemm_splitk_dma_nt": lambda: Gemm(True, True),
    "gemm_tn_row_ranges": GemmTN, "mlp_score_wgrad": ScoreWgrad,
    "prelu_bwd_vector": lambda: PreluTwo(True), "prelu_bwd_scalar": lambda: PreluTwo(False),
    "prelu_bwd_vector_no_sums": lambda: PreluTwo(True, False), "prelu_bwd_scalar_no_sums": lambda: PreluTwo(False, False),
    "full_loss": FullLoss, "spmm_csr": SpmmSeg, "spmm_sliced": SpmmSliced, "spmm_panel": SpmmPanel, "spmm_ring": SpmmRing,
    "adae_colsum": lambda: AdaeColsum(False), "adae_colsum_weighted": lambda: AdaeColsum(True), "adae_stru": AdaeStru,
    "gaan_edge": GaanEdge, "aegis_loss_bwd": AegisLossBwd,
}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_a_b_a_b_on_one_nan_filled_workspace(name):
    D.run_sequence(ENTRY_POINTS[name]())


# ------------------------------------------------------------------------------------------------ 16: the exclusive scan
def test_exclusive_scan_on_a_shrinking_input_and_a_poisoned_workspace():
    """ggad_exclusive_scan_i32 with n = 100000, 2049, 5 and 100000 again on ONE int32 workspace filled with -1 before the first call
    (its words are tile sums and tile offsets, added to outputs and never used as addresses: plan.hip): exact, out[n] included, and
    nothing written behind out[n] or outside the workspace."""
    lib = _lib()
    sizes = (100000, 2049, 5, 100000)
    n_ws = int(lib.ggad_scan_workspace_elems(sizes[0]))
    assert n_ws == _cdiv(sizes[0], 2048) + 1 and int(lib.ggad_scan_workspace_elems(5)) == 2
    ws_block, ws = D.int_like(n_ws, -1)
    for k, n in enumerate(sizes):
        a = np.random.default_rng(1900 + k).integers(0, 50, size=n).astype(np.int32)
        x = torch.from_numpy(a).to(DEV)
        ref = np.concatenate([[0], np.cumsum(a.astype(np.int64))])
        outs = []
        for w_block, w in ((ws_block, ws), D.int_like(int(lib.ggad_scan_workspace_elems(n)), -1)):
            out_block, out = D.int_like(n + 1, -7)
            _ok(lib.ggad_exclusive_scan_i32(_ptr(x), _ptr(out), n, _ptr(w), _st()))
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().astype(np.int64), ref), (k, n)
            assert bool((out_block[:D.GUARD] == -7).all()) and bool((out_block[D.GUARD + n + 1:] == -7).all())
            assert bool((w_block[:D.GUARD] == -1).all()) and bool((w_block[D.GUARD + w.numel():] == -1).all())
            outs.append(out.cpu().numpy())
            D.dirty_lines()
        assert outs[0].tobytes() == outs[1].tobytes()


# ------------------------------------------------------------------------------------------------ 17: torch.randn's stream on the device
def test_device_randn_on_a_poisoned_scratch():
    """ggad_mt_randn_f32 with n = 4099, then 17, then both again, as consecutive draws of ONE generator on ONE scratch filled with NaN
    bits before the first call: the state after every draw exactly the restatement's (tests/mt_randn_ref.py), the values within
    test_kernel_against_the_stream's bound of the float64 formula, and bit-equal to the same draw on a scratch of its own size."""
    from ggad_amd import rng
    from test_device_noise_gpu import _host_state, _rel, _torch_deviation
    keep = torch.get_rng_state()
    try:
        st = _host_state(0)
        bound = 2.0 * _torch_deviation("fresh")
    finally:
        torch.set_rng_state(keep)
    words, pos = rng.parse_rng_state(st)
    sizes = (4099, 17, 4099, 17)
    lib = _lib()
    assert int(lib.ggad_mt_randn_scratch_elems(4099)) > int(lib.ggad_mt_randn_scratch_elems(17)) > 0
    mt = rng.DeviceMT(DEV, words, pos, st)
    scratch = D.nan_like(int(lib.ggad_mt_randn_scratch_elems(sizes[0])))
    mt.scratch = scratch.view(torch.int32)
    for k, n in enumerate(sizes):
        own = rng.DeviceMT(DEV, words, pos, st)
        own_scratch = D.nan_like(int(lib.ggad_mt_randn_scratch_elems(n)))
        own.scratch = own_scratch.view(torch.int32)
        u, words, pos = MR.draw_uniforms(words, pos, n)
        v64, r64 = MR.box_muller(u, n, np.float64)
        buf, buf2 = D.nan_like(n), D.nan_like(n)
        mt.randn_(buf)
        D.dirty_lines()
        own.randn_(buf2)
        torch.cuda.synchronize()
        for m in (mt, own):
            got_words, got_pos = m.state_host()
            assert got_pos == pos and np.array_equal(got_words, words), (k, n)
        got = buf.cpu().numpy()
        assert np.isfinite(got).all() and torch.equal(buf.view(torch.int32), buf2.view(torch.int32)), (k, n)
        assert _rel(got, v64, r64) <= bound, (k, n)
        for t in (buf, buf2, scratch, own_scratch):
            D.guards_intact(t)


# ------------------------------------------------------------------------------------------------ the three production caches
def _spmm_ok(FG, csr, x):
    got = FG.spmm(csr, x).cpu().numpy()
    ref = csr.host.astype(np.float64) @ x.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any()
    assert np.abs(got - ref).max() / (np.abs(ref).max() + 1.0) < 2e-6                            # test_spmm_lds_panel_single_partial_panel_and_rectangular


@pytest.mark.parametrize("kind", ["ring", "panel", "sliced"])
def test_the_shared_staging_buffer_poisoned_between_products_of_different_width(kind, monkeypatch):
    """`fullgraph._XS_WORKSPACE`: one buffer per stream, shared by every product of an epoch and only ever growing.  The 900-row
    product at W = 64 sizes it; then it is NaN-filled; then the 150 x 200 product at W = 36 (a partial last slice) and the 900-row one
    again with fresh data run on it, each against scipy in float64."""
    from ggad_amd import fullgraph as FG
    env = {"ring": {"GGAD_SPMM_PANEL": "1", "GGAD_SPMM_RING": "1"}, "panel": {"GGAD_SPMM_PANEL": "1", "GGAD_SPMM_RING": "0"},
           "sliced": {"GGAD_SPMM_SLICED": "1", "GGAD_SPMM_PANEL": "0"}}[kind]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(5)
    mats = []
    for n_rows, n_src, dens, w in ((900, 900, 0.2, 64), (150, 200, 0.5, 36)):
        a = sp.random(n_rows, n_src, density=dens, random_state=7, format="csr", dtype=np.float32)
        a.data[:] = 1.0
        mats.append((FG.Csr(a, DEV), n_src, w))
    big, small = mats
    x = _f32(rng.standard_normal((big[1], big[2])))
    assert FG.spmm_route(big[0], big[0].plan(), x).kind == kind
    _spmm_ok(FG, big[0], x)
    key = (str(x.device), torch.cuda.current_stream(x.device).cuda_stream)
    xs = FG._XS_WORKSPACE[key]
    assert xs.numel() >= int(_lib().ggad_spmm_sliced_workspace_elems(big[1], big[2]))
    xs.fill_(NAN)
    xsmall = _f32(rng.standard_normal((small[1], small[2])))
    assert FG.spmm_route(small[0], small[0].plan(), xsmall).kind == kind
    _spmm_ok(FG, small[0], xsmall)
    D.dirty_lines()
    _spmm_ok(FG, big[0], _f32(rng.standard_normal((big[1], big[2]))))
    assert FG._XS_WORKSPACE[key] is xs                                                           # the same buffer served all three


def test_the_cached_partial_sum_buffers_poisoned_between_products(monkeypatch):
    """`plan["part"]` of the whole-matrix plan and of a row subset (`csr.plan(rows, ...)`), NaN-filled after a first product at
    W = 300, then read by products at W = 28 (the stale tail behind n_seg x 28) and at W = 300 with fresh data."""
    from ggad_amd import fullgraph as FG
    for k, v in {"GGAD_SPMM_SLICED": "0", "GGAD_SPMM_PANEL": "0", "GGAD_SPMM_ROWSLICE": "0"}.items():
        monkeypatch.setenv(k, v)
    csr = FG.Csr(_sparse_case(600, (100, 400), (7, 8, 599), 21), DEV)
    rows = np.array([100, 7, 3, 599, 400, 8, 250])
    sub = csr.plan(rows, key=("dirty", 0))
    rng = np.random.default_rng(6)
    ref_m = csr.host.astype(np.float64)

    def product(w, plan):
        x = _f32(rng.standard_normal((600, w)))
        assert FG.spmm_route(csr, plan if plan is not None else csr.plan(), x).kind == "seg"
        got = FG.spmm(csr, x, plan=plan).cpu().numpy()
        ref = ref_m @ x.cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any()
        assert np.abs(got - (ref if plan is None else ref[rows])).max() / (np.abs(ref).max() + 1.0) < 2e-6      # test_spmm_sliced_column_ranges_and_empty_rows
        return got

    product(300, None)
    product(300, sub)
    assert csr.plan()["n_multi"] > 0 and sub["n_multi"] > 0
    for w in (28, 300):
        csr.plan()["part"].fill_(NAN)
        sub["part"].fill_(NAN)
        got = product(w, sub)
        assert not np.any(got[[1, 3, 5]])                                                        # the empty rows 7, 599, 8: stored zeros
        D.dirty_lines()
        product(w, None)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "launch_sequence"])
def test_the_cached_loss_workspace_poisoned_between_two_loss_blocks(fused, monkeypatch):
    """`loss_ws` / `loss_ws_fused` kept on the loss structures of `FullGraphAdj`: NaN-filled between two loss blocks on different
    data (the ticket word beside the fused one is left alone: the header requires it to be zero).  Bounds of test_loss_block."""
    from ggad_amd import fullgraph as FG
    monkeypatch.setattr(FG, "_LOSS_FUSED", fused)
    c = C.loss_case(C._loss(40, 12, 8, 9, seed=600))
    fa = FG.FullGraphAdj(c["adj_norm"], c["raw"], DEV)
    ls = fa.loss_structs(c["nrm"], c["abn"])
    key = "loss_ws_fused" if fused else "loss_ws"
    for k in range(3):
        rng = np.random.default_rng(2000 + k)
        if k:
            c = dict(c, emb=C._f32(rng.standard_normal(c["emb"].shape)), logits=C._f32(rng.standard_normal(c["logits"].shape)),
                     con=C._f32(rng.standard_normal(c["con"].shape)), eab=C._f32(rng.standard_normal(c["eab"].shape)))
            ws = ls[key][0] if fused else ls[key]
            ws.fill_(NAN)
        ref = C.loss_reference(c, torch.float64)
        C.check_loss_reference(c, ref)
        ins = [_f32(c[q]).requires_grad_(True) for q in ("emb", "logits", "con", "eab")]
        out = FG.GgadLossFn.apply(*ins, fa, ls, C.MARGIN)
        assert out[0].grad_fn.fused == fused
        aff = out[0].grad_fn.affinity
        out[0].backward(gradient=torch.full((), C.G_TOTAL, device=DEV))
        got = D.host(dict(losses=torch.stack([o.detach() for o in out]), aff=aff, d_emb=ins[0].grad, d_logits=ins[1].grad, d_con=ins[2].grad,
                          d_abn=ins[3].grad))
        for q, cls in C.LOSS_CLASSES.items():
            assert not np.isnan(got[q]).any(), (k, q)
            d = C.distance(got[q], ref[q])
            assert d <= C.BOUND[cls], (k, q, d, C.BOUND[cls])
        D.dirty_lines()
    if fused:
        assert int(ls[key][1].item()) == 0
