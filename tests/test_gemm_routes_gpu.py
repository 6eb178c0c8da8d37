"""Every kernel behind `ggad_gemm_f32` against float64, with the kernel that ran NAMED (`ggad_gemm_last_route`, ABI 11).

`ggad_gemm_f32` chooses among k_gemm_slab, k_gemm_bres, k_mlp_wgrad (the "TN" row-range route), k_gemm_small, k_gemm_dma and
k_gemm_f32, the last two with k_splitk_reduce behind them ("GEMM routes").  tests/gemm_fp64.py holds one case per branch
of that choice -- every template instance of the slab and resident-operand kernels, both sides of every threshold, the five
(vp, vq) forms of the row-range kernel, split-K with empty trailing splits -- and the route each must report.  Per case, plain and
with bias + ReLU: the route and variant; max |got - ref| / (max |ref| + 1) < 2e-6 against numpy in float64 on the same float32
operands (the bound of test_gemm_f32_all_layouts); operands in NaN-padded blocks, C a view of a NaN block whose padding and guards
stay NaN while no NaN is left inside; the workspace NaN-filled before the first call, the partials of empty splits exact zeros; a
second call bit-identical.  The switches the library reads once per process run in a child process each.

`pytest -s` prints the error of every case and the largest per route and variant.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dirty as D
import gemm_fp64 as G
from conftest import ROOT

pytestmark = pytest.mark.gpu

WORST = {}                        # (route, variant) -> (largest error, case) over the cases run so far


READ_ONCE = ("the library reads GGAD_GEMM_DMA, _SCALAR, _TM and _DMA_BUFS at the first GEMM of the process: if one of them was set then "
             "(test_gemm_f32_all_layouts[dma=0] sets GGAD_GEMM_DMA=0), the DMA / TILED routes of this process are not the table's")


def _check(name, which, r, want, hint=""):
    route, variant, empty = want
    label = G.describe(r["route"], r["variant"])
    extra = "" if "err_numpy_f32" not in r else f"   (numpy float32 product: {r['err_numpy_f32']:.3e})"
    print(f"\n[gemm route] {name:<40} {which:<5} {label:<40} err {r['err']:.3e}{extra}", end="")
    assert (r["route"], r["variant"]) == (route, variant), (name, which, label, "expected " + G.describe(route, variant), hint)
    if route in G.SPLIT_ROUTES:
        assert r["empty"] == empty, (name, which, r["empty"], empty)
        assert r["empty_zero"] is (True if empty else None), (name, which, "partials of the empty splits are not zeros")
    assert r["nans"] == 0, (name, which, r["nans"])
    assert r["err"] < G.BOUND, (name, which, r["err"])
    assert r["repeat_equal"], (name, which)
    key = (r["route"], r["variant"])
    if key not in WORST or r["err"] > WORST[key][0]:
        WORST[key] = (r["err"], name + " " + which)


@pytest.mark.parametrize("name", list(G.CASES))
def test_gemm_takes_the_route_its_case_names_and_matches_float64(name):
    c = G.CASES[name]
    got = G.run_case(c)
    for which in ("plain", "br"):
        want = G.expected(c, which)
        _check(name, which, got[which], want, READ_ONCE if {want[0], got[which]["route"]} & set(G.ROUTES[5:]) else "")


@pytest.mark.parametrize("m,n,k,ks", [(4096, 128, 260, 17), (4097, 128, 276, 18), (4095, 128, 260, 0), (4096, 176, 276, 0)])
def test_linear_prelu_records_slab_or_nothing(m, n, k, ks):
    """`ggad_linear_prelu_f32` at K = 260 / 276 (k_gemm_slab<17>, <18>): SLAB where the shape is taken -- z and out against float64 --,
    NONE with GGAD_E_UNSUPPORTED and both outputs untouched where it is not (M < 4096; 11 column tiles)."""
    from ggad_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(m + n + k)
    a, w = rng.standard_normal((m, k)).astype(np.float32), (0.2 * rng.standard_normal((n, k))).astype(np.float32)
    b, slope = rng.standard_normal(n).astype(np.float32), np.float32(0.25)
    da, dw, db = (torch.from_numpy(x).to(D.DEV) for x in (a, w, b))
    pa = torch.tensor([slope], device=D.DEV)
    z, out = D.padded(m, n, n + 4), D.padded(m, n, n + 8)
    _lib.call("ggad_gemm_f32", da.data_ptr(), dw.data_ptr(), D.padded(m, n, n).data_ptr(), m, n, k, k, 1, 1, k, n, 0, 0, 0)
    assert _lib.gemm_last_route()[0] != "NONE"                 # (so that NONE below is this call's record)
    rc = int(lib.ggad_linear_prelu_f32(da.data_ptr(), k, dw.data_ptr(), k, db.data_ptr(), pa.data_ptr(), m, n, k, z.data_ptr(), n + 4,
                                       out.data_ptr(), n + 8, _lib.current_stream()))
    route = _lib.gemm_last_route()
    torch.cuda.synchronize()
    D.guards_intact(z)
    D.guards_intact(out)
    if ks == 0:
        assert rc == _lib.GGAD_E_UNSUPPORTED and route == ("NONE", 0)
        assert bool(torch.isnan(z).all()) and bool(torch.isnan(out).all())
        return
    assert rc == 0 and route == ("SLAB", ks)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + b
    ez = G.distance(z.cpu().numpy(), ref)
    eo = G.distance(out.cpu().numpy(), np.where(ref > 0, ref, float(slope) * ref))
    print(f"\n[gemm route] linear_prelu {m}x{n}x{k}  SLAB<{ks}>  z {ez:.3e}  out {eo:.3e}", end="")
    assert ez < G.BOUND and eo < G.BOUND


# One child at a time; a child runs the cases of G.SWITCH_GROUP (each plain and with bias + ReLU, twice) after importing torch and
# loading the library.  Measured on an MI355X: 3.0 s for a child that was the first GPU process on the machine, 2.6 - 2.8 s for the
# four started by this test, nearly all of it start-up; the limit is about three times the first figure.
CHILD_SECONDS = 3.0
CHILD_TIMEOUT = 3.3 * CHILD_SECONDS
CHILD_FAILED = []                 # the switch whose child did not exit with status 0: no further child is started in this process


def _run_child(switch, env):
    """One child, and only if every earlier one exited with status 0: after a fault, an abort or a timeout of a child nothing more
    is started on the card by this module."""
    assert not CHILD_FAILED, f"the child of {CHILD_FAILED[0]} did not exit with status 0: not starting another"
    CHILD_FAILED.append(switch)                    # (until this child is known to have ended well)
    p = subprocess.run([sys.executable, os.path.join("tests", "gemm_fp64.py"), "--group", ",".join(G.SWITCH_GROUP)], cwd=ROOT, env=env,
                       timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    assert p.returncode == 0, (switch, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    CHILD_FAILED.remove(switch)
    return p


@pytest.mark.parametrize("switch", G.SWITCHES)
def test_read_once_switches_in_a_fresh_process(switch):
    """GGAD_GEMM_DMA=0, _SCALAR=1, _TM=128 and _DMA_BUFS=3 are `static const` in the library, read at the first call of a process:
    each gets a process of its own that runs the tiled / DMA cases (four layouts, aligned and not, with and without split-K, with
    empty splits) and reports what ran.  DMA=0: what DMA took runs on k_gemm_f32 with vec = 1; SCALAR=1: vec = 0; TM=128: the 128-row
    tile with its own split counts; DMA_BUFS=3: the three-buffer k_gemm_dma."""
    key, val = switch.split("=")
    env = dict(os.environ)
    for s in G.SWITCHES:
        env.pop(s.split("=")[0], None)
    env[key] = val
    p = _run_child(switch, env)
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    cases = [c for c in G.CASES.values() if c["group"] in G.SWITCH_GROUP]
    assert [ln["name"] for ln in lines] == [c["name"] for c in cases]
    seen = set()
    for c, ln in zip(cases, lines):
        for which in ("plain", "br"):
            _check(f"{switch} {c['name']}", which, ln[which], G.expected_under(c, switch, which))
            r, v = ln[which]["route"], ln[which]["variant"]
            seen.add((r, v >> 8 & 3, v >> 10) if r.startswith("TILED") else (r, v >> 8, 64))      # (route, vec or buffers, tile rows)
    # the switch did switch something: the forms it exists for ran, with and without split-K
    routes = {r for r, _, _ in seen}
    if key == "GGAD_GEMM_DMA":
        assert {(r, v, 64) for r in ("TILED", "TILED_SPLITK") for v in (1, 2)} == seen
    elif key == "GGAD_GEMM_SCALAR":
        assert {("TILED", 0, 64), ("TILED_SPLITK", 0, 64), ("DMA", 2, 64), ("DMA_SPLITK", 2, 64)} == seen
    elif key == "GGAD_GEMM_TM":
        assert {(r, v, 128) for r in ("TILED", "TILED_SPLITK") for v in (1, 2)} == seen
    else:
        assert {("DMA", 3, 64), ("DMA_SPLITK", 3, 64)} <= seen and not any(r.startswith("DMA") and v != 3 for r, v, _ in seen)
        assert routes == set(G.ROUTES[5:])


def test_largest_error_per_route():
    """The table of `-s` (last in the file: the children's forms are in it).  With the whole case list run in this process, every
    route, every template instance of the slab and resident-operand kernels and every (vp, vq) form has a line."""
    print()
    for (route, variant), (err, name) in sorted(WORST.items()):
        print(f"[gemm route, largest error] {G.describe(route, variant):<44} {err:.3e}   {name}")
    ran = set(WORST)
    want = {G.expected(c, which)[:2] for c in G.CASES.values() for which in ("plain", "br")}
    if ran >= want:                 # (a selection with -k runs fewer)
        assert {r for r, _ in ran} == set(G.ROUTES) - {"NONE"}
        assert {v for r, v in ran if r == "BRES"} == set(range(8, 21))
        assert {v for r, v in ran if r == "SLAB"} == {2, 4, 16, 17, 18, 19, 20}
        assert {v for r, v in ran if r == "WGRAD_TN"} == {G.v_tn(*p) for p in ((2, 4), (2, 2), (1, 4), (1, 2), (1, 1))}
        print(f"[gemm route, largest error] all {len(want)} forms of the table ran in this process: completeness asserted")
    else:
        print(f"[gemm route, largest error] {len(want - ran)} of the table's {len(want)} forms did not run (or failed) in this process: "
              "completeness NOT asserted here (tests/test_gemm_routes_cpu.py asserts it on the table)")
