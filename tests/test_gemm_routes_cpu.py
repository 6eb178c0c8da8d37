"""The case table of tests/gemm_fp64.py against the library's own arithmetic -- no GPU (the library loads without one).

What the GPU test takes from the table on trust is checked here: the split counts and the number of empty trailing splits it
declares are the ones `ggad_gemm_workspace_elems` sizes the workspace for, and the table reaches every route, every template
instance of k_gemm_bres and k_gemm_slab, every (vp, vq) form of the row-range kernel and every threshold from both sides."""
import pytest

import gemm_fp64 as G
from ggad_amd import _lib


def _calls(c):
    return [G.expected(c, which) for which in ("plain", "br")]


@pytest.mark.parametrize("name", list(G.CASES))
def test_declared_splits_are_the_library_s(name):
    c = G.CASES[name]
    M, N, K = c["M"], c["N"], c["K"]
    splits, kps = G.gemm_splits(M, N, K)
    ws = int(_lib.load().ggad_gemm_workspace_elems(M, N, K))
    assert ws == (0 if splits == 1 else max(splits * M * N, G.wgrad_tn_ws(K, M, N)))
    for route, variant, empty in _calls(c):
        if not c["ws"]:                            # a caller without a workspace: nothing can split
            assert splits > 1 and route in ("SMALL", "DMA", "TILED") and G.splits_of(variant) <= 1 and empty == 0
        elif route in G.SPLIT_ROUTES:
            assert G.splits_of(variant) == splits > 1 and kps % 32 == 0
            assert empty == G.empty_splits(M, N, K) == sum(1 for s in range(splits) if s * kps >= K)
        elif route == "WGRAD_TN":
            assert splits > 1 and 0 < G.wgrad_tn_ws(K, M, N) <= ws and c["ta"] and not c["tb"] and c["pad"][2] == 0
        else:
            assert splits == 1 and empty == 0      # SLAB, BRES, SMALL, and DMA / TILED without a workspace


def test_the_issue_s_empty_split_shapes():
    assert (G.gemm_splits(300, 300, 5124), G.empty_splits(300, 300, 5124)) == ((20, 288), 2)
    assert (G.gemm_splits(300, 300, 5200), G.empty_splits(300, 300, 5200)) == ((20, 288), 1)
    assert (G.gemm_splits(512, 512, 1025), G.empty_splits(512, 512, 1025)) == ((8, 160), 1)
    assert (G.gemm_splits(64, 64, 16385), G.empty_splits(64, 64, 16385)) == ((65, 256), 0)
    assert (G.gemm_splits(300, 298, 5124), G.empty_splits(300, 298, 5124)) == ((20, 288), 2)
    # 128-row tiles (GGAD_GEMM_TM=128) count other tiles: the child of that switch is held to this arithmetic
    assert G.gemm_splits(300, 300, 5124, 128) == (21, 256) and G.empty_splits(300, 300, 5124, 128) == 0
    assert G.gemm_splits(512, 512, 1025, 128) == (9, 128) and G.empty_splits(512, 512, 1025, 128) == 0
    # ... and leave none of the shapes above with an empty split; K = 8705 / 8708 have three there (none at 64-row tiles)
    for k in (8705, 8708):
        assert (G.gemm_splits(300, 300, k), G.empty_splits(300, 300, k)) == ((20, 448), 0)
        assert (G.gemm_splits(300, 300, k, 128), G.empty_splits(300, 300, k, 128)) == ((34, 288), 3)
    group = [c for c in G.CASES.values() if c["group"] in G.SWITCH_GROUP]
    # every child meets an empty split in each form of its kernels: vec of k_gemm_f32, "dma" for k_gemm_dma
    forms = {"GGAD_GEMM_DMA=0": {1, 2}, "GGAD_GEMM_SCALAR=1": {0, "dma"}, "GGAD_GEMM_TM=128": {1, 2}, "GGAD_GEMM_DMA_BUFS=3": {1, 2, "dma"}}
    for switch in G.SWITCHES:
        want = [G.expected_under(c, switch, "plain") for c in group]
        assert {v >> 8 & 3 if r == "TILED_SPLITK" else "dma" for r, v, e in want if r in G.SPLIT_ROUTES and e} == forms[switch], switch

def test_table_reaches_every_route_instance_and_threshold():
    calls = [(c, r) for c in G.CASES.values() for r in _calls(c)]
    assert {r[0] for _, r in calls} == set(G.ROUTES) - {"NONE"}
    assert {r[1] for _, r in calls if r[0] == "BRES"} == set(range(8, 21))
    assert {r[1] for _, r in calls if r[0] == "SLAB"} == {2, 4, 16, 17, 18, 19, 20}
    assert {r[1] for _, r in calls if r[0] == "WGRAD_TN"} == {G.v_tn(*p) for p in ((2, 4), (2, 2), (1, 4), (1, 2), (1, 1))}
    assert {r[1] >> 8 & 3 for _, r in calls if r[0] == "TILED"} == {1, 2} == {r[1] >> 8 & 3 for _, r in calls if r[0] == "TILED_SPLITK"}
    for route in G.SPLIT_ROUTES:                   # with and without an empty split, aligned and not
        assert {r[2] > 0 for _, r in calls if r[0] == route} == {True, False}
    for c, r in calls:                             # the instance is the one K selects, the kernels' own preconditions hold
        if r[0] in ("SLAB", "BRES"):
            assert r[1] == (c["K"] + 15) // 16 and c["K"] % 4 == 0 and not c["ta"] and c["pad"][0] % 4 == 0
            assert c["M"] >= (4096 if r[0] == "SLAB" else 16384) and (c["tb"] or (c["N"] % 4 == 0 and c["pad"][1] % 4 == 0))
        if r[0] == "BRES":
            assert 128 <= c["K"] <= 320 and 64 < c["N"] <= 1024
        if r[0] == "SMALL":
            assert 1 <= c["K"] <= 512 and c["M"] <= 1024 and c["M"] * c["N"] <= 524288 and -(-c["M"] // 32) * -(-c["N"] // 32) <= 1024
    by = lambda g, **kw: [c for c in G.CASES.values() if c["group"] == g and all(c[k] == v for k, v in kw.items())]      # noqa: E731
    # both sides of every threshold the issue lists
    assert by("bres", N=1024)[0]["route"] == "BRES" and by("bres", N=1028)[0]["route"] != "BRES"
    assert {c["M"] for c in by("bres")} >= {16384, 16385, 16399} and {c["N"] for c in by("bres")} >= {65, 81, 96}
    assert by("slab", M=4095)[0]["route"] != "SLAB" and by("slab", N=176)[0]["route"] != "SLAB" and by("slab", N=1284)[0]["route"] != "SLAB"
    assert all(c["route"] == "SLAB" for c in by("slab", N=1280) + by("slab", N=113)) and {c["M"] for c in by("slab")} >= {4096, 4097, 4111}
    assert {(c["K"], c["route"]) for c in by("small", M=100, ws=False)} == {(512, "SMALL"), (513, "TILED")} == {(c["K"], c["route"]) for c in by("small", M=2)}
    assert {(c["K"], c["route"]) for c in by("small", M=100, ws=True)} == {(512, "DMA_SPLITK"), (513, "TILED_SPLITK")}
    assert {(c["M"], c["route"]) for c in by("small", K=64)} == {(1024, "SMALL"), (1025, "DMA")}
    assert {(c["N"], c["route"]) for c in by("small", K=16, M=1024)} == {(512, "SMALL"), (513, "TILED")}
    assert {(c["N"], c["route"]) for c in by("small", K=16, M=1)} == {(32768, "SMALL"), (40000, "TILED")}      # 1,024 tiles of 32 x 32 / more
    assert 40000 <= 524288 and -(-40000 // 32) > 1024 == -(-32768 // 32)                  # (declined by the tile count alone)
    assert {(c["ta"], c["tb"]) for c in by("small", K=100, route="SMALL")} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(c["K"], c["route"]) for c in by("wgrad", M=32, N=64, pad=(0, 0, 0))} == {(1024, "WGRAD_TN"), (1023, "DMA_SPLITK")}
    assert by("wgrad", M=33)[0]["route"] != "WGRAD_TN" and by("wgrad", N=516)[0]["route"] != "WGRAD_TN" and by("wgrad", N=512)[0]["route"] == "WGRAD_TN"
    for g in ("dma", "tiled"):                     # the children's subset: four layouts, with and without split-K
        for split in (False, True):
            assert {(c["ta"], c["tb"]) for c in by(g) if (c["route"] in G.SPLIT_ROUTES) == split} == {(a, b) for a in (False, True) for b in (False, True)}, (g, split)
    assert {G.splits_of(c["variant"]) for c in by("dma", M=1088)} == {1, 4, 16, 8}
    assert any(max(c["pad"]) > 0 for c in by("bres")) and all(any(c["pad"][i] > 0 for c in G.CASES.values()) for i in range(3))


def test_switch_expectations():
    """What a child process must report under each read-once switch, on the cases where it matters."""
    c = G.CASES["dma-300x300x5124-NN"]
    assert G.expected_under(c, "GGAD_GEMM_DMA=0", "plain") == ("TILED_SPLITK", G.v_tiled(20, 1), 2)
    assert G.expected_under(c, "GGAD_GEMM_SCALAR=1", "plain") == ("DMA_SPLITK", G.v_dma(20), 2)
    assert G.expected_under(c, "GGAD_GEMM_TM=128", "br") == ("TILED_SPLITK", G.v_tiled(21, 1, 128), 0)
    assert G.expected_under(c, "GGAD_GEMM_DMA_BUFS=3", "plain") == ("DMA_SPLITK", G.v_dma(20, 3), 2)
    c = G.CASES["tiled-1027x131x37-TN"]
    assert G.expected_under(c, "GGAD_GEMM_SCALAR=1", "plain") == ("TILED", G.v_tiled(1, 0), 0)
    assert G.expected_under(c, "GGAD_GEMM_TM=128", "plain") == ("TILED", G.v_tiled(1, 2, 128), 0)
    assert G.expected_under(c, "GGAD_GEMM_DMA=0", "plain") == G.expected(c, "plain")


def test_route_record_without_a_launch():
    """NONE after a call that launched nothing: invalid arguments (no GPU is touched), and on a thread that never called."""
    import threading
    lib = _lib.load()
    assert lib.ggad_gemm_f32(None, None, None, 4, 4, 4, 4, 1, 4, 1, 4, None, 0, None, None) == _lib.GGAD_E_INVALID
    assert _lib.gemm_last_route() == ("NONE", 0)
    assert lib.ggad_linear_prelu_f32(None, 4, None, 4, None, None, 4, 4, 4, None, 4, None, 4, None) == _lib.GGAD_E_INVALID
    assert _lib.gemm_last_route() == ("NONE", 0)
    seen = []
    t = threading.Thread(target=lambda: seen.append(int(lib.ggad_gemm_last_route())))
    t.start()
    t.join()
    assert seen == [0]
    assert _lib.GEMM_ROUTES == G.ROUTES
