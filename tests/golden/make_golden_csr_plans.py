#!/usr/bin/env python3
"""Record the panel and ring SpMM plans (`Csr.panel_plan`, `Csr.ring_plan`) of commit 862a044, the last one before the two
builders shared their round layout, dealing and workgroup table.  A plan is a set of integer tables: equal tables mean that the
kernels read the same bytes.  CPU only (`Csr(m, "cpu")`); needs the library (`python -m ggad_amd.build`).

    python tests/golden/make_golden_csr_plans.py     # in a checkout of 862a044 with this file added: writes csr_plans_862a044.json

Per case the file holds a sha256 of the input's `indptr` and `indices`, what `value_factors()` found, and for either plan `null`
or: a sha256 per integer table, the integer scalars, the `repr` of the float scalars (plain IEEE divisions of integer counts).
The float vectors `rs`, `cs`, `diag` are not recorded (they would tie the file to one numpy build's `power`);
tests/test_csr_plans_cpu.py compares them with `value_factors()` of its own run.

The inputs are built with integer arithmetic only, so they depend on no library's random stream.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

GOLDEN = os.path.join(HERE, "csr_plans_862a044.json")
TABLES = ("wg", "dir", "stream", "row_tab", "wave_sb", "idx", "ctl")
INTS = ("n_wg", "n_chunks", "n_phases", "blocks", "rounds", "quads", "walkers")
FLOATS = ("fill", "phase_skew", "steps_per_phase")
VECTORS = ("rs", "cs", "diag")
SWITCHES = ("GGAD_RING_XCD", "GGAD_RING_SUBSET_STEPS")
ROWS = [7, 1499, 3, 3, 640, 0] + list(range(100, 160))                    # a row subset with a repeated row


def adjacency(n, k):
    """0/1, symmetric, empty diagonal: row i gets the columns (7 i + 13 t^2 + t) mod n, t = 1..k; 12 hub rows at the multiples of
    n // 12, each joined to every second node from h mod 2 on."""
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    t = np.tile(np.arange(1, k + 1, dtype=np.int64), n)
    r, c = [i], [(7 * i + 13 * t * t + t) % n]
    for h in (np.arange(12, dtype=np.int64) * (n // 12)).tolist():
        to = np.arange(h % 2, n, 2, dtype=np.int64)
        r.append(np.full(len(to), h, dtype=np.int64))
        c.append(to)
    r, c = np.concatenate(r), np.concatenate(c)
    a = sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(n, n)).tocsr()
    a = ((a + a.T) > 0).astype(np.float64).tolil()
    a.setdiag(0)
    a = a.tocsr()
    a.eliminate_zeros()
    return a


def finish(a, mode):
    """outside: D^-1/2 A D^-1/2 + I;  inside: D^-1/2 (A + I) D^-1/2;  pattern: all ones."""
    if mode == "pattern":
        return a
    n = a.shape[0]
    if mode == "inside":
        a = a + sp.eye(n)
    d = np.asarray(a.sum(1)).reshape(-1)
    with np.errstate(divide="ignore"):
        r = np.power(d, -0.5)
    r[np.isinf(r)] = 0.0
    m = sp.diags(r) @ a @ sp.diags(r)
    return (m if mode == "inside" else m + sp.eye(n)).tocsr()


def _graph(n, k, mode):
    return lambda: finish(adjacency(n, k), mode)


def _three_entries():
    return sp.coo_matrix((np.ones(3), ([0, 1500, 2999], [1, 7, 2998])), shape=(3000, 3000)).tocsr()


def _unfactorable():
    m = finish(adjacency(2992, 40), "outside")
    m.sum_duplicates()
    m.sort_indices()
    m.data = m.data * (1.0 + (np.arange(m.nnz, dtype=np.int64) % 7) / 10.0)
    return m


def _case(name, matrix, n_slices, rows=None, env=None):
    return dict(name=name, matrix=matrix, n_slices=n_slices, rows=rows, env=env or {})


CASES = [
    _case("n2992_k40_outside_s3", _graph(2992, 40, "outside"), 3),
    _case("n2992_k40_inside_s10", _graph(2992, 40, "inside"), 10),
    _case("n3845_k40_outside_s10", _graph(3845, 40, "outside"), 10),
    _case("n12011_k20_outside_s10", _graph(12011, 20, "outside"), 10),
    _case("n26017_k20_pattern_s10", _graph(26017, 20, "pattern"), 10),
    _case("n26017_k20_outside_s16", _graph(26017, 20, "outside"), 16),
    _case("n1500_k30_pattern_s2", _graph(1500, 30, "pattern"), 2),
    _case("n1500_k30_pattern_s2_xcd_block", _graph(1500, 30, "pattern"), 2, env={"GGAD_RING_XCD": "block"}),
    _case("n1500_k30_pattern_s2_rows", _graph(1500, 30, "pattern"), 2, rows=ROWS),
    _case("n1500_k30_outside_s2_rows", _graph(1500, 30, "outside"), 2, rows=ROWS),
    _case("n100_k20_pattern_s1", _graph(100, 20, "pattern"), 1),
    _case("n2992_k40_outside_s3_subset_steps_0", _graph(2992, 40, "outside"), 3, env={"GGAD_RING_SUBSET_STEPS": "0"}),
    _case("n3000_three_entries_s3", _three_entries, 3),
    _case("n64_all_zero_s1", lambda: sp.csr_matrix((64, 64), dtype=np.float64), 1),
    _case("n2992_k40_outside_s3_values_scaled", _unfactorable, 3),
]


def _sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


def plans(case):
    """(csr, panel plan, ring plan) of a case, from a fresh `Csr`; the caller has set the case's environment."""
    from ggad_amd.fullgraph import Csr
    csr = Csr(case["matrix"](), "cpu")
    if case["rows"] is None:
        return csr, csr.panel_plan(case["n_slices"]), csr.ring_plan(case["n_slices"])
    rows = np.asarray(case["rows"])
    return csr, csr.panel_plan(case["n_slices"], rows, {}), csr.ring_plan(case["n_slices"], rows, {})


def describe_plan(p):
    if p is None:
        return None
    assert set(p) <= set(TABLES + INTS + FLOATS + VECTORS), sorted(p)
    d = dict(keys=sorted(p))
    d["tables"] = {k: dict(dtype=str(p[k].dtype), numel=int(p[k].numel()), sha256=_sha(p[k].numpy())) for k in TABLES if k in p}
    d["ints"] = {k: int(p[k]) for k in INTS if k in p}
    d["floats"] = {k: repr(float(p[k])) for k in FLOATS if k in p}
    return d


def describe(csr, panel, ring):
    fac = csr.value_factors()
    kind = "none" if fac is False else "ones" if fac[0] is None else "factors+diag" if fac[2] is not None else "factors"
    return dict(input=dict(shape=list(csr.shape), nnz=int(csr.nnz), indptr=_sha(csr.host.indptr.astype(np.int64)),
                           indices=_sha(csr.host.indices.astype(np.int64))),
                value_factors=kind, panel=describe_plan(panel), ring=describe_plan(ring))


def main():
    out = {}
    for case in CASES:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(case["env"])
        out[case["name"]] = describe(*plans(case))
        p, r = out[case["name"]]["panel"], out[case["name"]]["ring"]
        print(case["name"], "panel", None if p is None else (p["ints"], p["floats"]), "ring", None if r is None else (r["ints"], r["floats"]))
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", GOLDEN)


if __name__ == "__main__":
    main()
