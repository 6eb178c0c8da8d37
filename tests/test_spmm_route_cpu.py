"""`fullgraph.spmm_route` -- the one place that chooses the kernel of a sparse product -- decides what the `if / elif` chain of
`spmm()` decided before the choice moved there, and `padded_rows` pads where it padded.  That chain is written out below from the
kept threshold predicates and the LDS kernels' eligibility condition as it stood.  Host only: the matrices live in `Csr(m, "cpu")`,
the operands are CPU tensors (the decision reads their shape, strides and address, never their values) and the one question that
needs a device -- does it have the LDS for the panel / ring kernel -- is answered through `fullgraph._lds_kernels`.

Every kind is reached with no switch forced (`UNFORCED`); the forced values of every switch, a matrix without entries and an
operand whose row count is not the matrix's column count are compared with the chain as well."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from ggad_amd import _lib, synth
from ggad_amd import fullgraph as FG
from ggad_amd.csr import Csr
from ggad_amd.utils import normalize_adj

SWITCHES = ("GGAD_SPMM_SLICED", "GGAD_SPMM_ROWSLICE", "GGAD_SPMM_PANEL", "GGAD_SPMM_PANEL_MIN_NNZ", "GGAD_SPMM_PANEL_MIN_ROW",
            "GGAD_SPMM_RING", "GGAD_SPMM_COL_RANGES", "GGAD_SPMM_ROWLINE", "GGAD_RING_XCD", "GGAD_RING_SUBSET_STEPS")
N = 6000


def _graph(n, entries, seed, **kw):
    rowptr, col = synth.make_graph(n, entries, seed, kind="powerlaw", **kw)
    return (normalize_adj(synth.csr_to_scipy(rowptr, col, n)) + sp.eye(n)).tocsr()


@pytest.fixture(scope="module")
def mats():
    """name -> (Csr, segment plan): built once, the plans cached on them as in a run."""
    d16, d70, small = _graph(N, 16 * N, 1, max_degree=750), _graph(N, 70 * N, 2, max_degree=750), _graph(500, 4000, 3)
    weighted = d70.copy()
    weighted.data = weighted.data * np.random.default_rng(4).uniform(0.5, 1.5, size=weighted.nnz)
    out = {k: Csr(m, "cpu") for k, m in (("d16", d16), ("d70", d70), ("d70w", weighted), ("small", small),
                                          ("empty", sp.csr_matrix((500, 500), dtype=np.float32)))}
    out = {k: (c, c.plan()) for k, c in out.items()}
    rows = np.random.default_rng(5).permutation(N)[:5000]                  # (350 K entries: above the panel floors)
    out["d70rows"] = (out["d70"][0], out["d70"][0].plan(rows, key=("rows", "route")))
    return out


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _operand(n, w, padded=False):
    """An (n, w) operand; `padded`: its rows on 128-byte lines, as `padded_rows` makes them on a device (a CPU allocation is only
    64-byte aligned: the view starts at the next line of a slightly larger buffer)."""
    if not padded:
        return torch.empty(n, w)
    ld = (w + 31) // 32 * 32
    buf = torch.empty(n * ld + 32)
    off = (-buf.data_ptr() // 4) % 32
    return buf[off:off + n * ld].view(n, ld)[:, :w]


def _chain_panel(csr, p, X, lds):
    """`_use_panel` as it stood: the ring / panel plan, or None."""
    force = os.environ.get("GGAD_SPMM_PANEL")
    if force == "0" or X.shape[0] != csr.shape[1]:
        return None
    if not lds[0]:
        return None
    w = X.shape[1]
    nnz = p.get("nnz", csr.nnz)
    min_nnz = int(os.environ.get("GGAD_SPMM_PANEL_MIN_NNZ", str(1 << 18)))
    min_row = int(os.environ.get("GGAD_SPMM_PANEL_MIN_ROW", "32"))
    if force != "1" and not (w >= 64 and nnz >= min_row * p["n_out"] and nnz >= min_nnz):
        return None
    ring = os.environ.get("GGAD_SPMM_RING", "1") != "0" and lds[1]
    for build in ((Csr.ring_plan, Csr.panel_plan) if ring else (Csr.panel_plan,)):
        if p.get("rows") is not None:
            plan = build(csr, (w // 4 + 7) // 8, p["rows"], p.setdefault("panel_cache", {}))
        else:
            plan = build(csr, (w // 4 + 7) // 8)
        if plan is not None:
            return plan
    return None


def _chain(csr, p, X, lds):
    """The branch `spmm()` took."""
    if X.dim() == 2 and X.stride(1) == 1 and X.stride(0) > X.shape[1] and csr.nnz > 0 and FG._use_rowline(X):
        return "rowline"
    pp = _chain_panel(csr, p, X, lds)
    if pp is not None:
        return "ring" if "wave_sb" in pp else "panel"
    if FG._use_sliced(csr, p, X):
        return "sliced"
    if FG._use_rowslice(csr, p, X):
        return "rowslice"
    return "seg"


def _chain_pads(csr, p, n_rows, W, lds):
    """The condition under which `padded_rows` returned the padded view."""
    ld = (W + 31) // 32 * 32
    if ld == W or os.environ.get("GGAD_SPMM_ROWLINE", "1") == "0":
        return False
    X = torch.empty(n_rows, ld)[:, :W]
    return bool(csr.nnz > 0 and FG._use_rowline(X) and _chain_panel(csr, p, X, lds) is None and not FG._use_sliced(csr, p, X)
                and FG._use_rowslice(csr, p, X))


BOTH = ((True, True), (False, False))
# (matrix, width, LDS kernels available (panel, ring), switches, padded operand) -> kind, with no switch forced but the last of the ring rows
UNFORCED = ([("d16", w, lds, {}, False, "seg") for w in (28, 64) for lds in BOTH]
            + [("d16", w, lds, {}, False, "rowslice") for w in (160, 300) for lds in BOTH]
            + [("d16", 300, lds, {}, True, "rowline") for lds in BOTH]
            + [("d70", w, (True, True), {}, False, "ring") for w in (64, 160, 300)]
            + [("d70", 300, (True, False), {}, False, "panel"), ("d70", 300, (True, True), {"GGAD_SPMM_RING": "0"}, False, "panel"),
               ("d70", 300, (False, False), {}, False, "sliced"), ("d70", 64, (False, False), {}, False, "seg"),
               ("d70", 160, (False, False), {}, False, "seg")]
            + [("d70w", 300, lds, {}, False, "sliced") for lds in BOTH]
            + [("d70rows", 300, lds, {}, False, "sliced") for lds in BOTH]
            + [("small", w, lds, {}, False, "rowslice") for w in (160, 300) for lds in BOTH]
            + [("small", w, lds, {}, False, "seg") for w in (28, 64) for lds in BOTH])


@pytest.mark.parametrize("name,w,lds,env,padded,kind", UNFORCED)
def test_route_reaches_every_kind_as_the_chain_did(mats, name, w, lds, env, padded, kind, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(FG, "_lds_kernels", lambda dev: lds)
    csr, p = mats[name]
    X = _operand(csr.shape[1], w, padded)
    route = FG.spmm_route(csr, p, X)
    assert route.kind == _chain(csr, p, X, lds) == kind
    tables = {"rowline": lambda: csr.rowslice_plan(p, lines=True), "ring": lambda: _chain_panel(csr, p, X, lds),
              "panel": lambda: _chain_panel(csr, p, X, lds), "sliced": lambda: p["long"][1], "rowslice": lambda: csr.rowslice_plan(p),
              "seg": lambda: p}[kind]()
    assert route.tables is tables                                          # (cached plans: the same object on every call)


def test_unforced_grid_reaches_all_six_kinds():
    assert {c[-1] for c in UNFORCED if not c[3]} == {"rowline", "ring", "panel", "sliced", "rowslice", "seg"}


FORCED = ([{k: v} for k in ("GGAD_SPMM_SLICED", "GGAD_SPMM_ROWSLICE", "GGAD_SPMM_PANEL", "GGAD_SPMM_RING") for v in ("0", "1")]
          + [{"GGAD_SPMM_PANEL_MIN_NNZ": "1000"}, {"GGAD_SPMM_PANEL_MIN_NNZ": str(1 << 20)}, {"GGAD_SPMM_PANEL_MIN_ROW": "8"},
             {"GGAD_SPMM_PANEL_MIN_ROW": "128"}, {"GGAD_SPMM_COL_RANGES": "3"}, {"GGAD_SPMM_ROWLINE": "0"},
             {"GGAD_SPMM_PANEL": "1", "GGAD_SPMM_RING": "0"}, {"GGAD_SPMM_PANEL": "0", "GGAD_SPMM_SLICED": "1"},
             {"GGAD_SPMM_PANEL": "0", "GGAD_SPMM_SLICED": "0", "GGAD_SPMM_ROWSLICE": "1"}])


@pytest.mark.parametrize("env", FORCED, ids=lambda e: ",".join(f"{k[10:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("lds", [(True, True), (True, False), (False, False)])
def test_route_under_every_switch_as_the_chain_did(mats, env, lds, monkeypatch):
    """Every switch at its forced values, over all matrices (whole, row subset, non-factoring, tiny, empty), narrow and wide
    operands, plain and padded, and an operand with the wrong number of rows."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(FG, "_lds_kernels", lambda dev: lds)
    seen = set()
    for name, (csr, p) in mats.items():
        for w in (28, 64, 300):
            for X in (_operand(csr.shape[1], w), _operand(csr.shape[1], w, padded=True), _operand(csr.shape[1] + 5, w)):
                kind = FG.spmm_route(csr, p, X).kind
                assert kind == _chain(csr, p, X, lds), (name, w, tuple(X.shape), X.stride(0))
                seen.add(kind)
    assert len(seen) >= 2


def test_long_segment_plan_follows_the_column_range_switch(mats, monkeypatch):
    """The sliced kernel's plan is the one of the range count in force at the call, not the one of the first call."""
    monkeypatch.setenv("GGAD_SPMM_SLICED", "1")
    monkeypatch.setenv("GGAD_SPMM_PANEL", "0")
    csr, p = mats["d70"]
    X = _operand(N, 300)
    plans = {}
    for ranges in ("1", "3", "1", "3"):
        monkeypatch.setenv("GGAD_SPMM_COL_RANGES", ranges)
        kind, t = FG.spmm_route(csr, p, X)
        assert kind == "sliced" and plans.setdefault(ranges, t) is t
        want = csr.plan(None, key=None, seg=int(_lib.load().ggad_spmm_sliced_seg_len()), col_ranges=int(ranges))
        assert t["n_seg"] == want["n_seg"] and torch.equal(t["seg_beg"], want["seg_beg"]) and torch.equal(t["seg_out"], want["seg_out"])
    assert plans["3"]["n_seg"] > plans["1"]["n_seg"]


@pytest.mark.parametrize("lds", BOTH)
@pytest.mark.parametrize("env", [{}, {"GGAD_SPMM_ROWLINE": "0"}, {"GGAD_SPMM_ROWSLICE": "0"}, {"GGAD_SPMM_ROWSLICE": "1"},
                                 {"GGAD_SPMM_SLICED": "1"}, {"GGAD_SPMM_PANEL": "1"}, {"GGAD_SPMM_PANEL": "0"}],
                         ids=lambda e: ",".join(f"{k[10:]}={v}" for k, v in e.items()) or "unforced")
def test_padded_rows_pads_where_the_chain_padded(mats, env, lds, monkeypatch):
    """`padded_rows` allocates its own probe, and a CPU allocation never starts on a 128-byte line: `_use_rowline` is asked here with
    an aligned address in place of the probe's (its stride, width and row count as they are), for `padded_rows` and the chain alike,
    so that both answers occur.  Both answers occur with no switch forced."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(FG, "_lds_kernels", lambda dev: lds)
    lib = _lib.load()
    monkeypatch.setattr(FG, "_use_rowline", lambda X: bool(lib.ggad_spmm_rowline_supported(128, X.stride(0), X.shape[1], X.shape[0])))
    seen = set()
    for name, (csr, p) in mats.items():
        if p.get("rows") is not None:
            continue                                                       # (every caller names a whole matrix)
        for w in (64, 160, 256, 300, 512, 516):
            got = FG.padded_rows(csr.shape[1], w, "cpu", (csr, None))
            assert tuple(got.shape) == (csr.shape[1], w) and got.stride(1) == 1 and got.stride(0) in (w, (w + 31) // 32 * 32)
            assert (got.stride(0) != w) == _chain_pads(csr, p, csr.shape[1], w, lds), (name, w)
            seen.add(got.stride(0) != w)
            assert FG.padded_rows(csr.shape[1], w, "cpu").is_contiguous()                     # no consumer: never padded
    assert env or seen == {True, False}
