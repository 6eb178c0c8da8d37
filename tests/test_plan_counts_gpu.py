"""The integers of the mini-batch plan, exact, on graphs built to reach every branch of the pair counting and of the group builder
(case table and numpy restatement: tests/plan_counts_ref.py; the table is checked against its declarations without a GPU in
tests/test_plan_counts_cpu.py).

Every run asserts with `==` what the batch alone fixes -- the 2-hop counts c'_k in pc[], own_deg, own_rp, seg_t, the plan counters
-- and as sets / disjoint intervals what an atomic hands out (pw_base, group records, work items, the big list), and holds x2 of
every owner to the float64 reference at the bounds test_minibatch_gpu.py uses: 2e-6 up to 256 neighbours, 2e-5 for hubs."""
import numpy as np
import pytest
import torch

import plan_counts_ref as PR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd import _lib
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.minibatch import BatchChunk

DEV = "cuda:0"
F = PR.F
_DEVICE = {}


def _device(g, stride):
    """DeviceGraph and feature table (rows of `stride` floats; 32 = the trainer's 128-byte rows) of a case graph, made once."""
    key = (id(g), stride)
    if key not in _DEVICE:
        graph = _DEVICE[(id(g), 0)] = _DEVICE.get((id(g), 0)) or DeviceGraph(g.rowptr, g.col, DEV)
        table = torch.zeros(g.n, stride, dtype=torch.float32, device=DEV)
        table[:, :F] = torch.from_numpy(g.feat).to(DEV)
        _DEVICE[key] = (graph, table)
    return _DEVICE[key]


def _chunk(name, node_major=True, stride=32, xcd_skip=-1):
    c = PR.case(name)
    graph, table = _device(c["g"], stride)
    ch = BatchChunk(graph, table, 64, max_batches=len(c["batches"]), rows_cap=64, ent_cap=64, train=True, hop2="ldsw",
                    node_major=node_major, feat_dim=F)
    ch.xcd_skip = xcd_skip
    return ch


def _build(ch, name):
    batches = PR.case(name)["batches"]
    ch.build(batches, [np.zeros(len(b), dtype=np.int64) for b in batches])
    torch.cuda.synchronize()


def _x2_by_column(ch, name):
    """x2 of the owners of every batch, in the order of the reference's U_b."""
    ne = ch.n_ents
    x2 = ch.x2[:ne * F].view(-1, F).cpu().numpy()
    ent_col, ent_own = ch.ent_col[:ne].cpu().numpy(), ch.ent_own[:ne].cpu().numpy()
    out = []
    for b in range(len(PR.case(name)["batches"])):
        e0, e1 = ch.batch_ents(b)
        ents = np.arange(e0, e1)[ent_own[e0:e1] == np.arange(e0, e1)]
        out.append(x2[ents[np.argsort(ent_col[ents], kind="stable")]])
    return out


def _check_x2(ch, name):
    pcs, refs = PR.reference(name)
    for b, (bc, ref, got) in enumerate(zip(pcs, refs, _x2_by_column(ch, name))):
        assert got.shape == ref.shape
        deg = np.diff(bc.ptr)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), f"{name} batch {b}: NaN rows (degree-0 owners) differ"
        err = np.where(nan, 0.0, np.abs(got.astype(np.float64) - ref)).max(axis=1)
        hub = deg > 256
        print(f"{name} batch {b}: max |x2 - ref| {err[~hub].max(initial=0.0):.3e} (<= 256 neighbours, bound 2e-6), "
              f"{err[hub].max(initial=0.0):.3e} (hubs, bound 2e-5)")
        bad = np.nonzero(err > np.where(hub, 2e-5, 2e-6))[0]
        assert len(bad) == 0, f"{name} batch {b}: x2 of owner {int(bc.U[bad[0]])} ({int(deg[bad[0]])} neighbours) off by {err[bad[0]]:.3e}"


def _check(ch, name, range_option=0):
    c = PR.case(name)
    g = c["g"]
    assert ch.last_hop2 == c["hop2"]
    if c["hop2"] == "ldsw":
        PR.assert_plan_integers_exact(ch, g.rowptr, g.col, c["batches"], PR.effective_range_deg(range_option))
    _check_x2(ch, name)
    assert int(ch.cnt1.abs().sum()) == 0 and (ch.cnt2 is None or int(ch.cnt2.abs().sum()) == 0)


def _default_range_option():
    import os
    return int(os.environ.get("GGAD_RANGE_DEG", "0") or 0)


PER_CASE = [(n, nm) for n in PR.CASE_NAMES for nm in (True, False)]


def test_the_case_list_is_complete():
    """The parametrisations below are the table: every case in both gathers, and the sub-lists the table names."""
    assert {n for n, _ in PER_CASE} == set(PR._build_cases()) and len(PER_CASE) == 2 * len(PR.CASE_NAMES)
    assert set(PR.pair_targets().values()) <= set(PR.branches())
    hop2 = {n: PR.case(n)["hop2"] for n in PR.CASE_NAMES}
    assert [n for n in PR.CASE_NAMES if hop2[n] == "global"] == ["star65600"]
    assert all(hop2[n] == "ldsw" for n in PR.RANGE_CASES + PR.TILE_MAJOR_CASES + PR.GLOBAL_CASES)
    assert _default_range_option() == 0, "the table's big-owner expectations assume the id ranges are off by default"


@pytest.mark.parametrize("name,node_major", PER_CASE)
def test_plan_integers_and_x2(name, node_major):
    """node_major: work lists + k_gather2_items on the trainer's padded rows (the matrix-core slice); otherwise k_gather2_w, one wave
    per owner entry on rows of 17 floats, no lists.  The 65,601-entry star must report the device-atomic path by itself."""
    ch = _chunk(name, node_major=node_major, stride=32 if node_major else F)
    _build(ch, name)
    _check(ch, name)


@pytest.mark.parametrize("name", PR.RANGE_CASES)
def test_plan_integers_with_id_ranges(name):
    """`ggad_mb_set_gather_options(-1, 256)`: an owner of 257 neighbours goes on the big list with its range bounds, one of 256 does
    not (rows of 17 floats: the VALU slice of the items kernel)."""
    lib = _lib.load()
    ch = _chunk(name, stride=F)
    lib.ggad_mb_set_gather_options(-1, 256)
    try:
        _build(ch, name)
    finally:
        lib.ggad_mb_set_gather_options(-1, _default_range_option())
    _check(ch, name, range_option=256)
    if name == "degrees":
        gp = PR.group_plan(ch.ent_col[ch.owner_entries()].cpu().numpy(), PR.case(name)["g"].rowptr, 256)
        assert sorted(gp.deg[gp.big].tolist()) == [257, 512, 513] and 256 in gp.deg[~gp.big].tolist()


@pytest.mark.parametrize("big,small", PR.REBUILDS)
def test_rebuild_on_dirty_tables(big, small):
    """A smaller chunk after a larger one on the same BatchChunk: pc, grp, items and the counters are reused as the first build left
    them."""
    ch = _chunk(big)
    _build(ch, big)
    _check(ch, big)
    _build(ch, small)
    _check(ch, small)


@pytest.mark.parametrize("name", PR.TILE_MAJOR_CASES)
def test_tile_major_and_xcd_skip(name, monkeypatch):
    """GGAD_TILE_MAJOR (read when a BatchChunk fills its descriptor, so one process serves both values) and one XCD left out: the
    integers are exact in every run -- the second plane of seg_t against tile_start included -- and x2 is bit-identical."""
    first = None
    for tile_major in (0, 1):
        for skip in (-1, 0, 5):
            monkeypatch.setenv("GGAD_TILE_MAJOR", str(tile_major))
            ch = _chunk(name, xcd_skip=skip)
            _build(ch, name)
            assert (ch.plan.col_t is not None) == bool(tile_major)
            _check(ch, name)
            bits = [x.view(np.int32) for x in _x2_by_column(ch, name)]
            if first is None:
                first = bits
            assert all(np.array_equal(a, b) for a, b in zip(first, bits)), (tile_major, skip)


@pytest.mark.parametrize("name", PR.GLOBAL_CASES)
def test_device_atomic_counts(name):
    """`ggad_mb_count2` on the tables of a built plan and a zeroed counter block: cnt2[slot n + k] == c'_k, 0 elsewhere; all zero
    again after `ggad_mb_plan_reset(..., with_hop2=1)`."""
    c = PR.case(name)
    g = c["g"]
    ch = _chunk(name)
    _build(ch, name)
    graph = ch.g
    nb, n = len(c["batches"]), g.n
    cnt2 = torch.zeros(nb * n, dtype=torch.int32, device=DEV)
    _lib.call("ggad_mb_count2", graph.rowptr.data_ptr(), graph.col.data_ptr(), ch.ent_col.data_ptr(), ch.ent_slot.data_ptr(),
              ch.ent_total_ptr(), ch.n_ents, n, ch.own1.data_ptr(), cnt2.data_ptr())
    torch.cuda.synchronize()
    pcs, _ = PR.reference(name)
    want = np.stack([np.bincount(bc.ids, minlength=n) for bc in pcs])
    assert np.array_equal(cnt2.cpu().numpy().reshape(nb, n), want)
    _lib.call("ggad_mb_plan_reset", graph.rowptr.data_ptr(), graph.col.data_ptr(), ch.ent_col.data_ptr(), ch.ent_slot.data_ptr(),
              ch.ent_own.data_ptr(), ch.ent_total_ptr(), ch.n_ents, n, ch.cnt1.data_ptr(), cnt2.data_ptr(), 1)
    torch.cuda.synchronize()
    assert int(cnt2.abs().sum()) == 0 and int(ch.cnt1.abs().sum()) == 0
