"""DeLong's variance and the paired test without a GPU: the binding, the refusals, the command-line rules and tests/delong_ref.py against
the definition.

  1. the four entry points (two calls, two workspace sizes) are bound and exported, and the ABI version is still 11;
  2. both `*_workspace_elems` refuse what `ggad_rank_wide_workspace_elems` refuses and need room beyond it;
  3. out-of-bounds calls return GGAD_E_INVALID before anything could launch;
  4. the argument checks of `metrics.auc_ci` / `compare_auc`, config key `auc_ci`, and the command-line rules of `src/main.py` and
     `run.py`, whose namespace without the options is the one of before;
  5. the reference (`single`, `pair`: exact integer sums of placements from `searchsorted`) equals `brute` (the O(mn) definition in
     Fractions) at n = 200 on random, quantised, saturated and independent inputs with 1, 7, 60 and 199 positives, and on signed zeros;
  6. `single` equals the midrank form of DeLong's variance (scipy's `rankdata`, `var(ddof=1)`) to 1e-12 relative at (11,193, 8,193)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import delong_ref as DL

NAMES = ("ggad_rank_delong_workspace_elems", "ggad_rank_delong_pair_workspace_elems", "ggad_rank_delong_f32", "ggad_rank_delong_pair_f32")


def test_the_binding_holds_the_entry_points():
    import ctypes
    from ggad_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert len(_lib.SIGNATURES["ggad_rank_delong_f32"][1]) == 9                # eight arguments and the stream
    assert len(_lib.SIGNATURES["ggad_rank_delong_pair_f32"][1]) == 10
    assert _lib.ABI_VERSION == 11 and int(lib.ggad_abi_version()) == 11
    from ggad_amd import metrics
    from ggad_amd.eval_cache import ResidentSweep
    assert callable(metrics.auc_ci) and callable(metrics.compare_auc) and callable(ResidentSweep.auc_ci) and callable(ResidentSweep.compare)


def test_workspace_elems_refuse_what_the_wide_call_refuses():
    from ggad_amd import _lib
    lib = _lib.load()
    cap = 1 << 20
    wide = lambda n, p: int(lib.ggad_rank_wide_workspace_elems(n, p))          # noqa: E731
    one = lambda n, p: int(lib.ggad_rank_delong_workspace_elems(n, p))         # noqa: E731
    two = lambda n, p: int(lib.ggad_rank_delong_pair_workspace_elems(n, p))    # noqa: E731
    for n, p in ((-1, 5), (2 ** 31, 5), (100, 0), (100, -1), (100, cap + 1), (2 ** 31, cap + 1)):
        assert wide(n, p) == 0 and one(n, p) == 0 and two(n, p) == 0, (n, p)
    for n in (0, 1, 63, 1024, 8193, 20000, 1736598, 2 ** 31 - 1):
        for p in (1, 600, 8192, 8193, 16385, cap):
            assert two(n, p) > 2 * one(n, p) > 2 * wide(n, p) > 0, (n, p)      # two halves, each a single layout and Lt, then the cross partials
            assert one(n, p) - wide(n, p) <= 8 * 128 + 3                       # four 64-bit words per tile
            assert one(n, p) % 4 == 0 and two(n, p) % 4 == 0


def test_out_of_bounds_calls_are_refused_before_any_launch():
    from ggad_amd import _lib
    lib = _lib.load()
    cap = int(lib.ggad_rank_wide_max_pos())
    ok = dict(a=16, b=16, label=16, n=10, pos_cap=5, out=16, sums=16, ws=16)

    def rc(pair, **kw):
        v = dict(ok, **kw)
        if pair:
            return lib.ggad_rank_delong_pair_f32(v["a"], v["b"], v["label"], v["n"], v["pos_cap"], 0.5, v["out"], v["sums"], v["ws"], None)
        return lib.ggad_rank_delong_f32(v["a"], v["label"], v["n"], v["pos_cap"], 0.5, v["out"], v["sums"], v["ws"], None)
    for bad in (dict(pos_cap=0), dict(pos_cap=cap + 1), dict(n=-1), dict(n=2 ** 31), dict(a=None), dict(label=None), dict(out=None),
                dict(sums=None), dict(ws=None), dict(ws=24)):
        assert rc(False, **bad) == -1 and rc(True, **bad) == -1, bad
    assert rc(True, b=None) == -1


def test_argument_checks_need_no_gpu():
    from ggad_amd.metrics import auc_ci, compare_auc
    s, y = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    for args in ((s.double(), y), (s, y.long()), (s.view(2, 2), y.view(2, 2)), (s, y[:3]), (s, y)):      # (the last: CPU tensors)
        with pytest.raises(ValueError, match="auc_ci takes"):
            auc_ci(*args)
        with pytest.raises(ValueError, match="compare_auc takes"):
            compare_auc(args[0], s, args[1])
        with pytest.raises(ValueError, match="compare_auc takes"):
            compare_auc(s, args[0], args[1])
    for level in (0.0, 1.0, -0.5, 95):
        with pytest.raises(ValueError, match="level"):
            auc_ci(s, y, level)


def test_config_key_auc_ci():
    import yaml
    from ggad_amd.model_handler import ModelHandler
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["auc_ci"] == 0                                                  # the key is there, off
    with pytest.raises(ValueError, match="auc_ci.*model: 'GCN'"):
        ModelHandler(dict(model="SAGE", auc_ci=0.95))
    for level in (1.0, 95, -0.1):
        with pytest.raises(ValueError, match="auc_ci.*confidence level"):
            ModelHandler(dict(model="GCN", auc_ci=level))


def test_main_py_command_line_rules():
    src = os.path.join(ROOT, "src")

    def run(*argv):
        return subprocess.run([sys.executable, "main.py", *argv], cwd=src, capture_output=True, text=True)
    p = run("--compare", "b.pkl")
    assert p.returncode == 2 and "--compare" in p.stderr and "needs --score" in p.stderr
    p = run("--score", "a.pkl", "--score_ids", "ids.npy", "--compare", "b.pkl")
    assert p.returncode == 2 and "no labels" in p.stderr
    p = run("--handler", "dominant", "--auc_ci")
    assert p.returncode == 2 and "--handler ggad only" in p.stderr
    p = run("--auc_ci", "1.5")
    assert p.returncode == 2 and "confidence level" in p.stderr
    p = run("--help")
    assert p.returncode == 0 and "--auc_ci [LEVEL]" in p.stdout and "--compare CKPT_B" in p.stdout


def test_run_py_command_line_rules(capsys):
    import argparse
    import run
    from ggad_amd import fullgraph_script as FS
    base = ["--dataset", "reddit", "--synthetic"]
    plain = run.parse(base)
    assert not hasattr(plain, "auc_ci") and not hasattr(plain, "compare")      # not given: no attribute, the namespace of before
    assert FS.compare_options(plain) == (None, None)
    a = run.parse(base + ["--auc_ci"])
    assert a.auc_ci == 0.95 and set(vars(a)) - set(vars(plain)) == {"auc_ci"}
    a = run.parse(base + ["--score", "a.pt", "--auc_ci", "0.9", "--compare", "b.pt"])
    assert FS.compare_options(a) == (0.9, "b.pt") and set(vars(a)) - set(vars(plain)) == {"score", "auc_ci", "compare"}
    for argv, text in ((["--compare", "b.pt"], "it needs --score"), (["--auc_ci", "0"], "confidence level"),
                       (["--auc_ci", "1"], "confidence level"), (["--save", "w.pt", "--compare", "b.pt"], "it needs --score")):
        with pytest.raises(SystemExit) as exc:
            run.parse(base + argv)
        assert exc.value.code == 2 and text in capsys.readouterr().err
    for add in (FS.add_select_options, FS.add_threshold_options):
        assert "--compare" not in add(argparse.ArgumentParser()).format_help()  # the options are run.py's own
    assert "--auc_ci [LEVEL]" in FS.add_compare_options(argparse.ArgumentParser()).format_help()


def _small_inputs():
    """The sixteen shapes of tests/test_operating_point_cpu.py, restated, and signed zeros."""
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
    z = np.array([0.0, -0.0, 0.0, -0.0, 0.5, -0.5], dtype=np.float32)
    out.append(("signed_zero", z, np.array([1, 0, 0, 1, 1, 0], dtype=np.uint8)))
    return out


SMALL = _small_inputs()


@pytest.mark.parametrize("name,s,y", SMALL, ids=[c[0] for c in SMALL])
def test_reference_against_the_definition(name, s, y):
    got = DL.single(s, y)
    theta, var = DL.brute(s, y)
    assert got["auc"] == theta
    assert got["status"] == (6 if name.endswith(("_p1", "_p199")) else 0)
    if got["status"] == 6:
        assert var is None and got["var"] is None and got["sums"][:2] == [got["S1"], 0]
        return
    assert got["var"] == var and got["N10"] >= 0 and got["N01"] >= 0
    # the pair against a second list of the same labels: the model's own quantisation (other tie runs)
    sb = (np.floor(s.astype(np.float64) * 2) / 2).astype(np.float32)
    pr = DL.pair(s, sb, y)
    other = DL.single(sb, y)
    assert pr["var_a"] == var and pr["var_b"] == other["var"] and pr["diff"] == got["auc"] - other["auc"]
    assert pr["cov"] == DL.brute_cov(s, sb, y)
    assert pr["var_diff"] == pr["var_a"] + pr["var_b"] - 2 * pr["cov"]           # (exact in Fractions: the identity behind ND10, ND01)
    assert pr["status"] == (7 if pr["var_diff"] == 0 else 0)
    same = DL.pair(s, s, y)
    assert same["status"] == 7 and same["ND10"] == same["ND01"] == 0 and same["cov"] == var


def test_reference_status_codes_and_limbs():
    s = np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32)
    y = np.array([0, 1, 0, 1], dtype=np.uint8)
    assert DL.single(s, np.zeros(4, np.uint8))["status"] == 1 and DL.single(s, np.ones(4, np.uint8))["status"] == 1
    assert DL.single(s, y, pos_cap=1)["status"] == 2
    assert DL.single(np.array([0.1, np.nan, 0.3, 0.4], dtype=np.float32), y)["status"] == 3
    assert DL.single(s, np.array([0, 2, 0, 1], dtype=np.uint8))["status"] == 4
    assert DL.single(s, np.array([0, 2, 0, 1], dtype=np.uint8))["sums"] == [0] * 12
    assert DL.pair(s, np.array([0.1, np.nan, 0.3, 0.4], dtype=np.float32), y)["status"] == 3
    assert DL.limbs([5, (1 << 64) + 7, (1 << 127) + (1 << 63)], 8) == [5, 0, 7, 1, -(1 << 63), -(1 << 63), 0, 0]
    a = np.array([(1 << 32), (1 << 32) - 1, 12345], dtype=np.int64)
    assert DL.dot(a, a) == sum(int(v) ** 2 for v in a) and DL.dot(a, a) >= 1 << 64


def test_reference_against_the_midrank_form():
    """DeLong's algorithm as usually written (Sun & Xu): V10_i = (midrank in all - midrank among the positives) / n, V01_j =
    1 - (midrank in all - midrank among the negatives) / m, var = var(V10, ddof=1) / m + var(V01, ddof=1) / n, in float64."""
    from scipy.stats import rankdata
    rng = np.random.default_rng(5)
    n_all, m = 11193, 8193
    y = np.zeros(n_all, dtype=np.uint8)
    y[rng.choice(n_all, m, replace=False)] = 1
    for s in ((rng.standard_normal(n_all) + y).astype(np.float32), (np.floor((rng.standard_normal(n_all) + y) * 16) / 16).astype(np.float32)):
        x, z = DL.fold(s)[y == 1].astype(np.float64), DL.fold(s)[y == 0].astype(np.float64)
        n = len(z)
        tz = rankdata(np.concatenate([x, z]))
        v10 = (tz[:m] - rankdata(x)) / n
        v01 = 1.0 - (tz[m:] - rankdata(z)) / m
        want = v10.var(ddof=1) / m + v01.var(ddof=1) / n
        got = DL.single(s, y)
        assert got["status"] == 0
        assert abs(float(got["var"]) - want) <= 1e-12 * want, (float(got["var"]), want)
        assert abs(float(got["auc"]) - v10.mean()) <= 1e-12
