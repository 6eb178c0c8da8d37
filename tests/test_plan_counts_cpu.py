"""The case table of tests/plan_counts_ref.py against its own declarations -- no GPU (the library loads without one).

What the GPU test takes on trust is checked here: every graph reaches the pairs per (tile, batch), the entries per batch, the
largest count, the owner occurrences and the degrees its case declares; the thresholds come from the sources; and the reference
counts, turned into x2 in float64, are the oracle's (`O.aggregate_batch`) -- or, for the two-centre star, the closed form."""
import numpy as np
import pytest

import plan_counts_ref as PR
from oracle import ggad_oracle as O


def test_constants_come_from_the_sources_and_give_the_table_of_the_issue():
    C = PR.constants()
    for fname, pats in PR.SOURCE_PATTERNS.items():
        with open(PR.os.path.join(PR.CSRC, fname)) as fh:
            text = fh.read()
        for name, pat in pats.items():
            assert len(PR.re.findall(pat, text)) == 1, (fname, name)
    assert set(PR.pair_targets()) == {0, 1, 1024, 1025, 4096, 4097, 16384, 16385, 20481, 98240, 98241}
    assert (C.MAXOWN, C.SLICE, C.TILE, C.RANGE_DEG, C.RANGES) == (6144, 256, 32768, 256, 8)
    assert PR.effective_range_deg(0) == 2 ** 31 - 1 and PR.effective_range_deg(256) == 256 and PR.effective_range_deg(100) == 256
    with pytest.raises(AssertionError):
        PR._once("constexpr int TW_T = 1; constexpr int TW_T = 2;", PR.SOURCE_PATTERNS["hop2_ldsw.hip"]["TW_T"], "twice")
    with pytest.raises(AssertionError):
        PR._once("", PR.SOURCE_PATTERNS["hop2_ldsw.hip"]["TW_T"], "never")


def test_the_case_list_is_complete():
    assert set(PR._build_cases()) == set(PR.CASE_NAMES)
    br = PR.branches()
    assert set(PR.pair_targets().values()) <= set(br) and len(br) == sum(len(PR.case(n)["reaches"]) for n in PR.CASE_NAMES)
    for group in (PR.RANGE_CASES, PR.TILE_MAJOR_CASES, PR.GLOBAL_CASES) + PR.REBUILDS:
        assert set(group) <= set(PR.CASE_NAMES)
    assert len(PR.GLOBAL_CASES) == 6
    for big, small in PR.REBUILDS:                                 # same graph, fewer entries the second time
        assert PR.case(big)["graph"]() is PR.case(small)["graph"]()
        assert sum(PR.reached(small).n_own.values()) < sum(PR.reached(big).n_own.values())


@pytest.mark.parametrize("name", PR.CASE_NAMES)
def test_case_reaches_what_it_declares(name):
    C = PR.constants()
    c = PR.case(name)
    g, d = c["g"], c["declares"]
    got = PR.reached(name)
    # the graph itself: symmetric, rows sorted and duplicate-free, no self loops
    rp, ci = g.rowptr.astype(np.int64), g.col.astype(np.int64)
    src = np.repeat(np.arange(g.n), np.diff(rp))
    assert (src != ci).all()
    key = src * g.n + ci
    assert (np.diff(key) > 0).all() and np.array_equal(np.sort(ci * g.n + src), key)
    assert got.n_tiles == d["n_tiles"]
    for k, p in d.get("P", {}).items():
        assert got.P[k] == p, ("P", k, got.P[k], p)
    for b, k in d["n_own"].items():
        assert got.n_own[b] == k, ("n_own", b, got.n_own[b], k)
    assert len(d["n_own"]) == len(c["batches"])
    assert got.max_count == d["max_count"]
    for u, m in d.get("m_u", {}).items():
        assert got.m_u[u] == m, ("m_u", u, got.m_u[u], m)
    for u, k in d.get("deg", {}).items():
        assert got.deg[u] == k, ("deg", u)
    for (s, t), p in d.get("slab_P", {}).items():
        assert got.slab_P[(0, s, t)] == p, ("slab", s, t)
    assert c["hop2"] == ("global" if max(got.n_own.values()) >= 65536 else "ldsw")
    if name == "pairs":
        # the bracket cases: > 128 consecutive pairs of one owner in tile 1; >= 200 owners in a row without a pair in it
        pcs, _ = PR.reference(name)
        nb = len(c["batches"])
        fat, gap = pcs[nb - 2], pcs[nb - 1]
        owner = np.repeat(np.arange(len(fat.U)), np.diff(fat.ptr))
        assert np.bincount(owner[fat.ids >> C.SHIFT == 1]).max() > 128
        owner = np.repeat(np.arange(len(gap.U)), np.diff(gap.ptr))
        has = np.nonzero(np.bincount(owner[gap.ids >> C.SHIFT == 1], minlength=len(gap.U)))[0]
        assert len(has) == 2 and has[1] - has[0] - 1 >= 200
        assert {got.P[(1, b)] for b in range(nb - 2)} == set(PR.pair_targets())
    if name.startswith("star"):
        a = g.a
        leaves = set(np.concatenate((ci[rp[a]:rp[a + 1]], [g.n - 1])).tolist())
        assert a % 2 == 0 and {0, C.TILE - 1, C.TILE, g.n - 1} <= leaves and (g.n - 1) >> C.SHIFT == got.n_tiles - 1 and g.n % C.TILE != 0


@pytest.mark.parametrize("name", PR.CASE_NAMES)
def test_reference_counts_give_the_oracle_s_x2(name):
    c = PR.case(name)
    g = c["g"]
    pcs, x2s = PR.reference(name)
    if name.startswith("star"):
        a, L = g.a, g.L
        f64 = g.feat.astype(np.float64)
        bc, x2 = pcs[0], x2s[0]
        leaf = bc.U != a
        assert int(bc.cp.max()) == L and np.array_equal(bc.U[leaf], np.concatenate((np.arange(a), np.arange(a + 2, g.n))))
        want = (f64[a] + f64[a + 1]) / (np.sqrt(2.0) * np.sqrt(float(L)))
        np.testing.assert_allclose(x2[leaf], np.broadcast_to(want, (L, PR.F)), rtol=1e-12, atol=0)
        np.testing.assert_allclose(x2[~leaf][0], f64[bc.U[leaf]].sum(0) / np.sqrt(float(L)), rtol=1e-10, atol=1e-13)
        return
    for bc, x2, nodes in zip(pcs, x2s, c["batches"]):
        if len(bc.U) > 7000:
            continue
        agg = O.aggregate_batch(g.rowptr, g.col, g.feat, nodes, True, dtype=np.float64)
        assert np.array_equal(agg.unique, bc.U)
        # 1e-12 relative; sums of signed terms of ~1e-2 may cancel, hence the floor of 1e-14 absolute
        np.testing.assert_allclose(x2, agg.to_feats_neigh, rtol=1e-12, atol=1e-14, equal_nan=True)
        assert np.array_equal(np.isnan(x2).any(1), np.diff(bc.ptr) == 0)
