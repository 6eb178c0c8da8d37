"""Host side of the PC-GNN device path: the float64 restatement the GPU tests measure against reproduces the imported reference
(tests/golden/minibatch_pcgnn.npz), and `check_relation` refuses what the kernels cannot take."""
import numpy as np
import pytest
import torch

import pcgnn_fp64
from conftest import load_golden
from ggad_amd.pcgnn_device import check_relation


@pytest.fixture(scope="module")
def golden():
    return load_golden("minibatch_pcgnn.npz")


def _evaluate(g, dtype):
    rels = [(g[f"rowptr{k}"], g[f"col{k}"]) for k in range(3)]
    return pcgnn_fp64.evaluate(rels, g["feat"], g["nodes"], g["labels"], {k: g["init." + k] for k in pcgnn_fp64.PARAMS}, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_with_ascending_unique_set_matches_the_reference_vectors(golden, dtype):
    """combined, affinity, both losses, the five gradients and prob_gnn of the imported reference classes, which walk U in python's
    set order, to 1e-6 absolute from the restatement that keeps U ascending (measured: 1.8e-7 in float64, 4.8e-7 in float32)."""
    r = _evaluate(golden, dtype)
    worst = 0.0
    for key in ["combined", "affinity", "loss", "prob_gnn"] + ["grad." + k for k in pcgnn_fp64.PARAMS]:
        want = golden[key].T if key == "combined" else golden[key]
        assert r[key].shape == want.shape, key
        err = float(np.abs(r[key] - want).max())
        worst = max(worst, err)
        assert err <= 1e-6, (key, err)
    print(f"\n[pcgnn restatement {dtype}] largest difference to the reference vectors: {worst:.2e}")


def test_check_relation_accepts_the_fixture_relations(golden):
    for k in range(3):
        rowptr, col = golden[f"rowptr{k}"], golden[f"col{k}"]
        check_relation(rowptr, col)
        assert int(np.diff(rowptr).min()) >= 2


def _broken(golden, kind):
    rowptr, col = golden["rowptr0"].astype(np.int64).copy(), golden["col0"].astype(np.int64).copy()
    row = 7
    a, b = int(rowptr[row]), int(rowptr[row + 1])
    assert b - a >= 2
    if kind == "empty":
        col = np.concatenate([col[:a], col[b:]])
        rowptr[row + 1:] -= b - a
    elif kind == "swapped":
        col[a], col[a + 1] = col[a + 1], col[a]
    elif kind == "duplicate":
        col[a + 1] = col[a]
    return rowptr, col, row


@pytest.mark.parametrize("kind", ["empty", "swapped", "duplicate"])
def test_check_relation_names_the_first_offending_row(golden, kind):
    rowptr, col, row = _broken(golden, kind)
    with pytest.raises(ValueError, match=rf"row {row}\b"):
        check_relation(rowptr, col)
    with pytest.raises(ValueError, match=rf"row {row}\b"):
        check_relation(rowptr.astype(np.int32), col.astype(np.int32))


def test_check_relation_refuses_columns_that_are_no_node(golden):
    rowptr, col = golden["rowptr1"].copy(), golden["col1"].copy()
    col[-1] = len(rowptr) - 1
    with pytest.raises(ValueError):
        check_relation(rowptr, col)
