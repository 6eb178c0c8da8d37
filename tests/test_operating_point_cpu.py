"""The operating point without a GPU: the binding, the refusals, the criterion parser, the command-line rules of `run.py --threshold`
and tests/operating_point_ref.py against a brute-force loop over every threshold.

  1. the three entry points are bound, there are five criteria and the ABI version is still 11;
  2. `ggad_rank_operating_workspace_elems` refuses what `ggad_rank_wide_workspace_elems` refuses and needs room beyond it;
  3. out-of-bounds calls return GGAD_E_INVALID before anything could launch;
  4. `metrics.parse_criterion`; `operating_point` / `pr_curve` argument checks; config key `thres_select`;
  5. `run.py`: `--threshold` is parsed by the same parser, `--score` with it is an error, and a command line without it leaves no
     attribute behind;
  6. the reference (`choose` over the positives' distinct scores) equals `brute_force` (every distinct score, python integers and
     Fractions) at n = 200, for every criterion, on random, quantised and saturated inputs: the candidate-set argument, checked."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import operating_point_ref as OP


def test_the_binding_holds_the_three_entry_points():
    from ggad_amd import _lib
    for name in ("ggad_rank_operating_criteria", "ggad_rank_operating_workspace_elems", "ggad_rank_operating_f32"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ggad_rank_operating_f32"][1]) == 13            # twelve arguments and the stream
    lib = _lib.load()
    assert int(lib.ggad_rank_operating_criteria()) == 5 == len(OP.CRITERIA)
    assert _lib.ABI_VERSION == 11 and int(lib.ggad_abi_version()) == 11
    from ggad_amd import metrics
    assert metrics.CRITERIA == OP.CRITERIA


def test_workspace_elems_refuses_what_the_wide_call_refuses():
    from ggad_amd import _lib
    lib = _lib.load()
    cap = 1 << 20
    wide = lambda n, p: int(lib.ggad_rank_wide_workspace_elems(n, p))          # noqa: E731
    ours = lambda n, p: int(lib.ggad_rank_operating_workspace_elems(n, p))     # noqa: E731
    for n, p in ((-1, 5), (2 ** 31, 5), (100, 0), (100, -1), (100, cap + 1), (2 ** 31, cap + 1)):
        assert wide(n, p) == 0 and ours(n, p) == 0, (n, p)
    for n in (0, 1, 63, 1024, 8193, 20000, 1736598, 2 ** 31 - 1):
        for p in (1, 600, 8192, 8193, 16385, cap):
            assert ours(n, p) > wide(n, p) > 0, (n, p)                         # the tiles' candidates lie behind the wide layout
            assert ours(n, p) - wide(n, p) <= 8 * 128 + 3


def test_out_of_bounds_calls_are_refused_before_any_launch():
    from ggad_amd import _lib
    lib = _lib.load()
    cap = int(lib.ggad_rank_wide_max_pos())
    f = lib.ggad_rank_operating_f32
    ok = dict(score=16, label=16, n=10, pos_cap=5, thres=0.5, crit=0, param=0.0, out=16, ct=None, ctp=None, cfp=None, ws=16)

    def rc(**kw):
        a = dict(ok, **kw)
        return f(a["score"], a["label"], a["n"], a["pos_cap"], a["thres"], a["crit"], a["param"], a["out"], a["ct"], a["ctp"], a["cfp"],
                 a["ws"], None)
    for bad in (dict(pos_cap=0), dict(pos_cap=cap + 1), dict(n=-1), dict(n=2 ** 31), dict(score=None), dict(label=None), dict(out=None),
                dict(ws=None), dict(ws=24), dict(crit=-1), dict(crit=5), dict(crit=3, param=-0.1), dict(crit=3, param=1.5),
                dict(crit=4, param=float("nan")), dict(crit=4, param=2.0), dict(ct=16), dict(ct=16, ctp=16), dict(ctp=16, cfp=16),
                dict(cfp=16)):
        assert rc(**bad) == -1, bad


def test_parse_criterion():
    from ggad_amd.metrics import parse_criterion
    assert parse_criterion("f1") == ("f1", None)
    assert parse_criterion("f1_macro") == ("f1_macro", None)
    assert parse_criterion(" gmean ") == ("gmean", None)
    assert parse_criterion("precision:0.9") == ("precision", 0.9)
    assert parse_criterion("fpr:0.01") == ("fpr", 0.01)
    assert parse_criterion("fpr:0") == ("fpr", 0.0) and parse_criterion("precision:1") == ("precision", 1.0)
    for bad in ("", "F1", "auc", "f1:0.5", "gmean:", "precision", "precision:", "precision:x", "precision:1.1", "fpr:-0.1", "fpr:nan",
                "recall:0.5", "f1 macro"):
        with pytest.raises(ValueError, match="threshold criterion"):
            parse_criterion(bad)


def test_argument_checks_need_no_gpu():
    from ggad_amd.metrics import operating_point, pr_curve
    s, y = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="unknown criterion"):
        operating_point(s, y, "auc")
    for crit, param in (("precision", None), ("precision", 1.5), ("fpr", -0.1), ("fpr", None)):
        with pytest.raises(ValueError, match="param"):
            operating_point(s, y, crit, param)
    for args in ((s.double(), y), (s, y.long()), (s.view(2, 2), y.view(2, 2)), (s, y[:3]), (s, y)):      # (the last: CPU tensors)
        with pytest.raises(ValueError, match="operating_point takes"):
            operating_point(*args)
        with pytest.raises(ValueError, match="operating_point takes"):
            pr_curve(*args)


def test_config_key_thres_select():
    import yaml
    from ggad_amd.model_handler import ModelHandler
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["thres_select"] == ""                                           # the key is there, off
    with pytest.raises(ValueError, match="threshold criterion"):
        ModelHandler(dict(model="GCN", thres_select="f2"))
    with pytest.raises(ValueError, match="thres_select"):
        ModelHandler(dict(model="SAGE", thres_select="f1"))
    assert ModelHandler.thres_path("/x/y.pkl") == "/x/y.pkl.thres.json"


def test_run_py_command_line_rules(capsys):
    import run
    base = ["--dataset", "reddit", "--synthetic"]
    plain = run.parse(base)
    assert not hasattr(plain, "threshold")                                     # not given: no attribute, the namespace of before
    a = run.parse(base + ["--threshold", "fpr:0.01", "--save", "w.pt"])
    assert a.threshold == "fpr:0.01"
    for argv, text in ((["--threshold", "f2"], "threshold criterion"), (["--threshold", "precision"], "takes a bound"),
                       (["--threshold", "gmean", "--score", "w.pt"], "--threshold chooses one at training time")):
        with pytest.raises(SystemExit):
            run.parse(base + argv)
        assert text in capsys.readouterr().err
    from ggad_amd import fullgraph_script as FS
    import argparse
    p = FS.add_select_options(argparse.ArgumentParser())
    assert "--threshold" not in p.format_help()                                # the option is run.py's own
    with_it = vars(run.parse(base + ["--threshold", "f1"]))
    assert set(with_it) - set(vars(plain)) == {"threshold"}


def _small_inputs():
    rng = np.random.default_rng(11)
    out = []
    for p in (1, 7, 60, 199):
        y = np.zeros(200, dtype=np.uint8)
        y[rng.choice(200, p, replace=False)] = 1
        x = rng.standard_normal(200) + (y == 1)
        out.append((f"normal_p{p}", x.astype(np.float32), y))
        out.append((f"quantised_p{p}", (np.floor(x * 4) / 4).astype(np.float32), y))
        out.append((f"saturated_p{p}", (1.0 / (1.0 + np.exp(-8.0 * x))).astype(np.float32), y))
        out.append((f"independent_p{p}", rng.random(200).astype(np.float32), y))
    s, y = OP.tie_by_hand()
    out.append(("tie_by_hand", s, y))
    z = np.array([0.0, -0.0, 0.0, -0.0, 0.5, -0.5], dtype=np.float32)
    out.append(("signed_zero", z, np.array([1, 0, 0, 1, 1, 0], dtype=np.uint8)))
    return out


@pytest.mark.parametrize("name,s,y", _small_inputs(), ids=[c[0] for c in _small_inputs()])
def test_reference_against_a_loop_over_every_threshold(name, s, y):
    cached = OP.candidates(s, y)
    assert len(cached[0]) == len(np.unique(OP.fold(s)[y == 1]))
    for crit, param in OP.COMBOS + (("precision", 0.0), ("precision", 1.0), ("fpr", 1.0), ("fpr", 0.25)):
        got = OP.choose(s, y, crit, param, cached)
        want = OP.brute_force(s, y, crit, param)
        if want is None:
            assert got["status"] == 5 and got["thres"] == np.inf and (got["tp"], got["fp"]) == (0, 0), (crit, param)
            assert got["fn"] == int(y.sum()) and got["tn"] == int((y == 0).sum()) and got["value"] == 0.0
            continue
        assert got["status"] == 0
        assert (got["thres"], got["tp"], got["fp"]) == want, (crit, param)
        pred = OP.fold(s) >= got["thres"]
        assert (int((pred & (y == 1)).sum()), int((pred & (y == 0)).sum())) == (got["tp"], got["fp"])


def test_tie_rule_by_hand_in_the_reference():
    s, y = OP.tie_by_hand()
    got = OP.choose(s, y, "f1")
    assert (got["thres"], got["tp"], got["fp"], got["value"]) == (np.float32(0.9), 1, 0, 0.5)
    s, y = OP.tie_by_hand_padded()
    got = OP.choose(s, y, "f1")
    assert (got["thres"], got["tp"], got["fp"], got["value"]) == (np.float32(0.9), 8192, 16382, 0.5)
    cand, tp, fp, P, Nn = OP.candidates(s, y)
    f1 = 2.0 * tp / (tp + fp + P)
    assert P == 8194 and (f1 <= 0.5).all() and int((f1 == 0.5).sum()) == 2
    s, y = OP.tie_across_sorted_tiles()
    got = OP.choose(s, y, "gmean")
    assert (got["thres"], got["tp"], got["fp"]) == (np.float32(0.9), 1, 0)
