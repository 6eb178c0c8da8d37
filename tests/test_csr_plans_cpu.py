"""The panel and ring SpMM plans (`Csr.panel_plan`, `Csr.ring_plan` in ggad_amd/csr.py) are, table for table, those of the commit
before their builders shared one round layout, dealing and workgroup table (tests/golden/csr_plans_862a044.json, written there by
tests/golden/make_golden_csr_plans.py, which also builds the inputs): the kernels read the same bytes.  The float vectors of a plan
are compared with `value_factors()` of the same run."""
import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_csr_plans", os.path.join(HERE, "golden", "make_golden_csr_plans.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.GOLDEN) as _fh:
    GOLDEN = json.load(_fh)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(c["name"] for c in G.CASES) and len(GOLDEN) == len(G.CASES)


@pytest.mark.parametrize("case", G.CASES, ids=[c["name"] for c in G.CASES])
def test_plans_equal_the_recorded_ones(case, monkeypatch):
    for k in G.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    want = GOLDEN[case["name"]]
    csr, panel, ring = G.plans(case)
    got = G.describe(csr, panel, ring)
    assert got["input"] == want["input"], "the input matrix moved, not the plan"
    assert got["value_factors"] == want["value_factors"]
    fac = csr.value_factors()
    for name, plan in (("panel", panel), ("ring", ring)):
        if want[name] is None:
            assert plan is None, name
            continue
        assert plan is not None, name
        for part in ("keys", "ints", "floats", "tables"):
            assert got[name][part] == want[name][part], (name, part)
        for v, f in zip(G.VECTORS, fac):                                  # passed through from value_factors()
            if f is None:
                assert plan[v] is None, (name, v)
            else:
                f = f[np.asarray(case["rows"])] if v == "rs" and case["rows"] is not None else f
                assert plan[v].dtype.is_floating_point and np.array_equal(plan[v].numpy(), f), (name, v)
