"""Keeping the best epoch on the device (csrc/select.hip, ggad_amd/select.py, `run.py --select / --save / --score`), the parts that
need no GPU:

  1. the numpy restatement (tests/select_ref.py) against hand-worked edge cases: a NaN value, a non-zero status, a tie (the earlier
     epoch stays), an invalid first epoch, AUROC and AP disagreeing on the best epoch, a curve shorter than the run;
  2. the new `run.py` flags parse and default to off; `--score` with `--select` is rejected;
  3. the three new symbols are bound in `_lib.SIGNATURES`; the argument checks of the two entry points return GGAD_E_INVALID before
     any launch;
  4. a checkpoint written from a CPU-constructed `Model` carries the reference's key names and loads with `strict=True`; another
     `n_in` / `embedding_dim` is refused with both values named;
  5. `write_ranked` lives in `metrics` and is still importable from `model_handler`."""
import ctypes
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import select_ref as R
from conftest import ROOT

NAN = float("nan")

# the parameter names of the reference's `Model` (its constructor order)
REFERENCE_KEYS = ["gcn1.bias", "gcn1.fc.weight", "gcn1.act.weight", "gcn2.bias", "gcn2.fc.weight", "gcn2.act.weight",
                  "gcn3.bias", "gcn3.fc.weight", "gcn3.act.weight", "fc1.weight", "fc2.weight", "fc3.weight", "fc4.weight",
                  "fc6.weight", "fc5.weight", "disc.f_k.weight", "disc.f_k.bias"]


def _run_py():
    spec = importlib.util.spec_from_file_location("ggad_run_script_select", os.path.join(ROOT, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


# ------------------------------------------------------------------------------------------------ 1. the restatement
def test_a_nan_value_is_never_taken():
    r = R.run([(0.5, 0.5, 0.0), (NAN, NAN, 0.0)], 0)
    assert r["taken"] == [True, False] and r["state4"].tolist()[:3] == [0.5, 0.0, 2.0] and r["state4"][3] == 0.0
    r = R.run([(NAN, NAN, 0.0), (0.25, 0.5, 0.0)], 1)          # a NaN first: best_epoch stays -1, so the next valid epoch is taken
    assert r["taken"] == [False, True] and r["state4"].tolist() == [0.5, 1.0, 2.0, 1.0]


def test_a_non_zero_status_is_never_taken():
    for status in (1.0, 2.0, 3.0, 4.0):
        r = R.run([(0.5, 0.5, 0.0), (0.9, 0.9, status)], 0)
        assert r["taken"] == [True, False] and r["state4"].tolist() == [0.5, 0.0, 2.0, 0.0]
        assert r["curve"][1].tolist() == [0.9, 0.9, status]       # (the curve records it all the same)


def test_a_tie_keeps_the_earlier_epoch():
    r = R.run([(0.75, 0.5, 0.0), (0.75, 0.5, 0.0), (0.75, 0.5, 0.0)], 0)
    assert r["taken"] == [True, False, False] and r["state4"].tolist() == [0.75, 0.0, 3.0, 0.0]
    one_ulp = np.nextafter(0.75, 1.0)
    r = R.run([(0.75, 0.5, 0.0), (one_ulp, 0.5, 0.0)], 0)        # strict > in double: one ulp more does displace
    assert r["taken"] == [True, True] and r["state4"].tolist() == [one_ulp, 1.0, 2.0, 1.0]


def test_an_invalid_first_epoch_leaves_no_best():
    r = R.run([(NAN, 0.0, 1.0)], 0)
    assert r["taken"] == [False] and R.same(r["state4"], [NAN, -1.0, 1.0, 0.0])
    r = R.run([(NAN, 0.0, 1.0), (0.0, 0.0, 0.0)], 0)              # a valid 0.0 afterwards is taken: there is no best yet
    assert r["taken"] == [False, True] and r["state4"].tolist() == [0.0, 1.0, 2.0, 1.0]


def test_auroc_and_ap_disagree_on_the_best_epoch():
    a, p = R.run(R.DISAGREE, 0), R.run(R.DISAGREE, 1)
    assert a["state4"].tolist() == [0.75, 3.0, 7.0, 0.0] and p["state4"].tolist() == [0.5, 2.0, 7.0, 0.0]
    assert R.same(a["curve"], p["curve"]) and R.same(a["curve"], np.array(R.DISAGREE))


def test_the_shared_sequence_and_its_snapshots():
    params = [[np.full(3, e, dtype=np.float32), np.full((2, 2), 10 + e, dtype=np.float32)] for e in range(len(R.SEQUENCE))]
    for which in (0, 1):
        r = R.run(R.SEQUENCE, which, params)
        assert r["taken"] == R.TAKEN[which]
        assert r["state4"].tolist() == [(0.875, 0.625)[which], 7.0, 9.0, 0.0]
        assert r["snapshot"][0].tolist() == [7.0] * 3 and r["snapshot"][1].tolist() == [[17.0, 17.0]] * 2
        r = R.run(R.SEQUENCE[:7], which, params)
        best = (3, 2)[which]
        assert r["snapshot"][0].tolist() == [float(best)] * 3 and r["snapshot"][1].tolist() == [[10.0 + best] * 2] * 2


def test_a_curve_shorter_than_the_run_is_not_overrun():
    r = R.run(R.SEQUENCE, 0, curve_cap=4)
    assert r["curve"].shape == (4, 3) and R.same(r["curve"], np.array(R.SEQUENCE[:4])) and r["state4"][2] == 9.0


def test_copy_follows_the_flag_bit_for_bit():
    src = [np.array([NAN, -0.0, 1.5], dtype=np.float32)]
    dst = [np.array([7.0, 8.0, 9.0], dtype=np.float32)]
    R.copy(np.array([0.5, 0.0, 1.0, 0.0]), src, dst)
    assert dst[0].tolist() == [7.0, 8.0, 9.0]
    R.copy(np.array([0.5, 0.0, 1.0, 1.0]), src, dst)
    assert dst[0].view(np.uint32).tolist() == src[0].view(np.uint32).tolist()


# ------------------------------------------------------------------------------------------------ 2. the command line
def test_the_new_flags_default_to_off():
    from ggad_amd.fullgraph_script import select_options
    a = _run_py().parse([])
    assert select_options(a) == (None, None, None, 0, "")
    # ... and leave no attribute behind: the namespace of a command line without them is the one run.py had before they existed
    assert not {"select", "save", "score", "top_k", "top_k_out"} & set(vars(a))
    assert select_options(types.SimpleNamespace()) == (None, None, None, 0, "")      # (a caller's hand-made namespace: off too)


def test_the_new_flags_parse():
    from ggad_amd.fullgraph_script import select_options
    run = _run_py()
    assert select_options(run.parse(["--select", "ap", "--save", "w.pt", "--synthetic"])) == ("ap", "w.pt", None, 0, "")
    assert select_options(run.parse(["--score", "w.pt", "--top_k", "50", "--top_k_out", "r.npz"])) == (None, None, "w.pt", 50, "r.npz")
    assert select_options(run.parse(["--select", "auroc"])) == ("auroc", None, None, 0, "")
    assert select_options(run.parse(["--score", "w.pt"])) == (None, None, "w.pt", 0, "")


@pytest.mark.parametrize("argv", [["--score", "w.pt", "--select", "auroc"], ["--score", "w.pt", "--save", "x.pt"], ["--select", "f1"],
                                  ["--top_k", "5"], ["--score", "w.pt", "--top_k_out", "r.npz"]])
def test_contradictory_flags_are_rejected(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        _run_py().parse(argv)
    assert exc.value.code == 2
    capsys.readouterr()


def test_fit_takes_the_validation_list_as_a_trailing_keyword_with_a_default():
    import inspect
    run = _run_py()
    for fn in (run.fit, run._fit):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "idx_val" and p["idx_val"].default is None
        assert list(p)[:10] == ["args", "dev", "full", "feats", "model", "normal_label_idx", "abnormal_label_idx", "idx_test", "ano_label", "history"]


# ------------------------------------------------------------------------------------------------ 3. the C ABI
def test_the_new_symbols_are_bound_and_the_abi_version_stays():
    from ggad_amd import _lib
    for name in ("ggad_select_max_tensors", "ggad_select_decide_f64", "ggad_select_copy_f32"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.ggad_abi_version() == _lib.ABI_VERSION == 11
    assert lib.ggad_select_max_tensors() == 16


def test_argument_checks_return_invalid_before_any_launch():
    from ggad_amd import _lib
    lib = _lib.load()
    fake = 4096                                                   # a non-null, aligned address that is never dereferenced on the host
    for which in (-1, 2, 3):
        assert lib.ggad_select_decide_f64(fake, which, fake, None, 0, None) == _lib.GGAD_E_INVALID
    assert lib.ggad_select_decide_f64(None, 0, fake, None, 0, None) == _lib.GGAD_E_INVALID
    assert lib.ggad_select_decide_f64(fake, 0, None, None, 0, None) == _lib.GGAD_E_INVALID
    assert lib.ggad_select_decide_f64(fake, 0, fake, fake, -1, None) == _lib.GGAD_E_INVALID
    arr = (ctypes.c_void_p * 17)(*([fake] * 17))
    num = (ctypes.c_int64 * 17)(*([4] * 17))
    for n in (0, 17, -1):
        assert lib.ggad_select_copy_f32(n, arr, arr, num, fake, None) == _lib.GGAD_E_INVALID
    assert lib.ggad_select_copy_f32(1, arr, arr, num, None, None) == _lib.GGAD_E_INVALID
    odd = (ctypes.c_void_p * 1)(fake + 2)                          # not 4-byte aligned
    assert lib.ggad_select_copy_f32(1, odd, arr, num, fake, None) == _lib.GGAD_E_INVALID
    neg = (ctypes.c_int64 * 1)(-1)
    assert lib.ggad_select_copy_f32(1, arr, arr, neg, fake, None) == _lib.GGAD_E_INVALID


def test_best_keeper_refuses_an_unknown_metric_without_a_gpu():
    from ggad_amd.select import BestKeeper
    with pytest.raises(ValueError, match="neither 'auroc' nor 'ap'"):
        BestKeeper([torch.zeros(3)], 4, "f1", labels_u8=np.zeros(2, dtype=np.uint8), rows=[0, 1])
    with pytest.raises(ValueError, match="one GPU"):
        BestKeeper([torch.zeros(3)], 4, "auroc", labels_u8=np.zeros(2, dtype=np.uint8), rows=[0, 1])


# ------------------------------------------------------------------------------------------------ 4. checkpoints
def test_checkpoint_of_a_cpu_model_round_trips_with_the_reference_key_names(tmp_path):
    from ggad_amd.fullgraph_script import load_checkpoint, save_checkpoint
    from ggad_amd.model import Model
    torch.manual_seed(3)
    model = Model(12, 16, "prelu", 1, "avg")
    args = types.SimpleNamespace(dataset="photo", embedding_dim=16, seed=3, select="auroc")
    path = str(tmp_path / "w.pt")
    meta = save_checkpoint(path, model.state_dict(), args, 12, 500, epoch=4, value=0.875)
    assert meta == {"dataset": "photo", "n_in": 12, "embedding_dim": 16, "nodes": 500, "seed": 3, "epoch": 4, "select": "auroc", "value": 0.875}
    ck = load_checkpoint(path, 12, 16)
    assert ck["meta"] == meta
    assert sorted(ck["state_dict"].keys()) == sorted(REFERENCE_KEYS) and len(list(model.parameters())) == 17
    torch.manual_seed(4)
    other = Model(12, 16, "prelu", 1, "avg")
    assert not torch.equal(other.fc1.weight, model.fc1.weight)
    other.load_state_dict(ck["state_dict"], strict=True)
    for (k, a), (k2, b) in zip(sorted(model.state_dict().items()), sorted(other.state_dict().items())):
        assert k == k2 and torch.equal(a, b)
    # without --select: the last epoch's weights, no metric
    args = types.SimpleNamespace(dataset="photo", embedding_dim=16, seed=3)
    meta = save_checkpoint(path, model.state_dict(), args, 12, 500, epoch=9)
    assert meta["select"] is None and meta["value"] is None and load_checkpoint(path, 12, 16)["meta"] == meta


def test_checkpoint_of_another_shape_is_refused_naming_both_values(tmp_path):
    from ggad_amd.fullgraph_script import load_checkpoint, save_checkpoint
    from ggad_amd.model import Model
    model = Model(12, 16, "prelu", 1, "avg")
    path = str(tmp_path / "w.pt")
    save_checkpoint(path, model.state_dict(), types.SimpleNamespace(dataset="photo", embedding_dim=16, seed=0), 12, 500, epoch=0)
    with pytest.raises(ValueError, match=r"n_in = 12, embedding_dim = 16; .* n_in = 13, embedding_dim = 16"):
        load_checkpoint(path, 13, 16)
    with pytest.raises(ValueError, match=r"n_in = 12, embedding_dim = 16; .* n_in = 12, embedding_dim = 32"):
        load_checkpoint(path, 12, 32)
    torch.save({"weights": 1}, path)
    with pytest.raises(ValueError, match="not a checkpoint written by --save"):
        load_checkpoint(path, 12, 16)


def test_model_score_adds_no_parameter():
    from ggad_amd.model import Model
    model = Model(12, 16, "prelu", 1, "avg")
    assert callable(model.score) and sorted(model.state_dict().keys()) == sorted(REFERENCE_KEYS)


# ------------------------------------------------------------------------------------------------ 5. write_ranked moved
def test_write_ranked_lives_in_metrics_and_is_re_exported(tmp_path):
    from ggad_amd import metrics, model_handler
    assert model_handler.write_ranked is metrics.write_ranked
    r = metrics.Ranked(pos=torch.tensor([2, 0], dtype=torch.int32), ids=torch.tensor([12, 10]), scores=torch.tensor([0.9, 0.8]),
                       cum_pos=torch.tensor([1, 1], dtype=torch.int32), m=2, n_pos=1, tied_left_out=0)
    path = str(tmp_path / "r.npz")
    metrics.write_ranked(path, r, np.array([0, 0, 1], dtype=np.uint8))
    z = np.load(path)
    assert z["node"].tolist() == [12, 10] and z["label"].tolist() == [1, 0] and z["cum_positives"].tolist() == [1, 1]
    assert int(z["n_pos"]) == 1 and int(z["tied_left_out"]) == 0 and z["score"].dtype == np.float32
