"""What tests/test_feature_widths_gpu.py relies on before a GPU is touched: the shared inputs hold the rows and batches they
promise, the float64 reference of every step case meets the conditions under which the step check means something, and the shapes
the narrow chain cannot take are refused at construction."""
import numpy as np
import pytest

from ggad_amd import _lib
import width_reference as WR


def test_graph_and_batches_hold_what_the_gpu_tests_need():
    rowptr, col = WR.graph()                                  # (asserts no degree-0 node, the hub, the pendant, 16- and 17-entry rows)
    closed = WR.closed_sizes(rowptr, col)
    assert len(rowptr) - 1 == WR.N_NODES and np.diff(rowptr).min() >= 1
    (_, nodes, lab), (_, n3, l3), (_, n130, l130) = WR.batches()
    assert len(nodes) == 48 and len(n3) == 3 and l3.tolist() == [0, 1, 1] and len(n130) == 130
    sizes = closed[nodes]
    assert sizes[2] == closed.max() >= WR.HUB_MIN and lab[2] == 0 and sizes[18] >= WR.HUB_MIN and lab[18] == 1
    assert {2, 16, 17} <= set(sizes.tolist())
    assert nodes[20] == nodes[21] and lab[20] == lab[21] and nodes[30] == nodes[12] and lab[30] != lab[12]
    ones = np.flatnonzero(lab == 1)
    assert (np.diff(ones) > 1).any() and ones.min() < 40 and 0 < (l130 == 1).sum() < 130       # label-1 rows in the middle


@pytest.mark.parametrize("f", [1, 17, 65])
def test_features_have_unit_rows(f):
    x = WR.feat(f).astype(np.float64)
    np.testing.assert_allclose(np.sqrt((x * x).sum(1)), 1.0, atol=1e-6)
    if f > 1:
        assert np.abs(x.mean(0)).max() < 0.05 and (x < 0).any()


def test_seg_lists_cover_the_block_loop():
    ptr, col, w = WR.seg_lists()
    assert np.diff(ptr).tolist() == list(WR.SEG_LENGTHS) and {0, 1, 2, 63, 64, 65, 128, 130, 300} == set(WR.SEG_LENGTHS)
    assert (w == 0).any() and w.min() < 0 < w.max() and col.max() < WR.N_NODES
    first = col[ptr[0]:ptr[1]]
    assert len(np.unique(first)) < len(first)                 # repeated ids within a row


STEP_SHAPES = sorted({(f, d) for f, d, _ in WR.STEP_CASES})


@pytest.mark.parametrize("f,d", STEP_SHAPES, ids=[f"f{f}-d{d}" for f, d in STEP_SHAPES])
def test_step_reference_meets_its_conditions(f, d):
    WR.check_step_conditions(f, d)


def test_step_cases_are_narrow_shapes():
    lib = _lib.load()
    for f, d, chain in WR.STEP_CASES:
        assert lib.ggad_mb_supported(d, f) == 1 and d <= lib.ggad_max_embed_dim() and chain in (0, 2)
    assert WR.STEP_CASES[0] == (65, 64, 0) and 4 * 65 * 64 * 4 > 64 * 1024 >= 4 * 64 * 64 * 4


def test_narrow_shape_predicate():
    lib = _lib.load()
    for d, f in [(64, 148), (32, 296), (9, 1024), (1, 1024), (64, 1), (16, 592)]:
        assert lib.ggad_mb_supported(d, f) == 1, (d, f)
    for d, f in [(64, 149), (32, 297), (1, 1025), (65, 17), (0, 17), (64, 0), (16, 593)]:
        assert lib.ggad_mb_supported(d, f) == 0, (d, f)
    for d in range(1, 65):
        for f in (1, 17, 9472 // d, 9472 // d + 1):
            assert lib.ggad_mb_supported(d, f) == int(f * d <= 9472 and f <= 1024), (d, f)


@pytest.mark.parametrize("chain", [0, 2])
@pytest.mark.parametrize("f,d,bound", [(149, 64, 148), (297, 32, 296), (745, 64, 148), (1025, 1, 1024)])
def test_unsupported_narrow_shape_is_refused_at_construction(f, d, bound, chain):
    """A ValueError before any allocation or launch (no device is needed to get it); it names the bound and the chain that takes
    the shape."""
    from ggad_amd.minibatch import MiniBatchEngine
    with pytest.raises(ValueError, match=f"features <= {bound} ") as exc:
        MiniBatchEngine(f, d, "cuda:0", chain=chain)
    assert ("chain=3 (the wide chain) takes this shape" in str(exc.value)) == (f <= 1024)
