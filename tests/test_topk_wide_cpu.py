"""Top-k above 16,384 ranks (csrc/topk.hip, `metrics.top_k(wide=True)`, config key `top_k_wide`), the parts that need no GPU:

  1. the wide cases of tests/topk_wide_ref.py of at most 5,000 elements against a brute-force python sort by (-score, position), and
     the shape of the case list;
  2. the library's caps and `ggad_topk_wide_workspace_elems` (0 on refused arguments, growing in n and in k); out-of-range arguments
     are refused before any launch;
  3. `check_k(16385)` raises as before and passes with `wide=True`;
  4. the `ModelHandler` config errors: `top_k_wide` without `top_k`, and today's message for a large `top_k` without the key;
  5. `run.py`'s parser: the namespace without the flag is unchanged, the flag without `--top_k` is an error; `main.py --score_ids`
     without `--score` is a parser error; `src/dgraph.yml` carries the key, off."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import topk_wide_ref as TW

NARROW, WIDE = 16384, 1 << 22


@pytest.fixture(scope="module")
def wide_cases():
    return TW.cases_wide(NARROW, WIDE)


def _brute(s, y, k):
    idx = sorted(range(len(s)), key=lambda i: (-float(s[i]), i))[:k]
    cum, run = [], 0
    for i in idx:
        run += int(y[i] == 1)
        cum.append(run)
    last = float(s[idx[-1]])
    left = sum(1 for v in s if float(v) == last) - sum(1 for i in idx if float(s[i]) == last)
    return idx, cum, left


# ------------------------------------------------------------------ 1: the cases
def test_the_small_wide_cases_against_a_brute_force_sort(wide_cases):
    small = [c for c in wide_cases if len(c[1]) <= 5000]
    assert [c[0] for c in small] == ["m2047", "m2048", "m2049", "runs3"]
    for name, s, y, k in small:
        r = TW.reference(s, y, k)
        idx, cum, left = _brute(s, y, k)
        assert r["m"] == k == len(idx), name
        assert r["pos"].tolist() == idx and r["cum_pos"].tolist() == cum, name
        assert np.array_equal(r["score"].view(np.int32), s[idx].view(np.int32)), name
        assert (r["n_pos"], r["tied_left_out"]) == (int(y.sum()), left), name


def test_the_wide_case_list_hits_what_it_is_meant_to(wide_cases):
    by = {c[0]: c for c in wide_cases}
    assert len(by) == len(wide_cases) == 16
    runs = lambda name: -(-min(by[name][3], len(by[name][1])) // TW.RUN)       # noqa: E731
    assert [runs(n) for n in ("m2047", "m2048", "m2049", "runs3", "runs5", "runs9_first_wide_k")] == [1, 1, 2, 3, 5, 9]
    assert by["runs9_first_wide_k"][3] == NARROW + 1 == by["k_is_n"][3] == len(by["k_is_n"][1])
    assert len(by["runs9_first_wide_k"][1]) == 19385
    assert (len(by["k_above_n"][1]), by["k_above_n"][3]) == (20000, 50000)
    _, s, y, k = by["all_tied"]
    r = TW.reference(s, y, k)
    assert (len(s), k, r["tied_left_out"]) == (40000, 25000, 15000) and r["pos"].tolist() == list(range(25000))
    _, s, y, k = by["ties_across_runs_and_cut"]
    r = TW.reference(s, y, k)
    assert (len(s), k, r["tied_left_out"]) == (70000, 30000, 6500)
    tied = r["pos"][1500:11500]
    assert (r["score"][1500:11500] == np.float32(0.75)).all() and r["score"][1499] > 0.75 > r["score"][11500]
    assert (np.diff(tied) > 0).all() and sorted(set((tied // 1015).tolist())) == list(range(69))   # every range of the scan holds some
    _, s, y, k = by["zeros_and_infinities"]
    r = TW.reference(s, y, k)
    assert (len(s), k) == (50000, 30000) and r["score"][-1] == 0 and r["tied_left_out"] > 0 and np.isinf(r["score"][0])
    _, s, y, k = by["saturated"]
    assert (len(s), k) == (270000, 100000)
    assert by["no_labels"][2] is None
    assert int(by["label_two"][2].max()) == 2 and np.isnan(by["nan_score"][1]).sum() == 1
    assert sorted(TW.STATUS_ONLY.items()) == [("label_two", 4), ("nan_score", 3)]
    _, s, y, k = by["at_cap"]
    assert (len(s), k, int(y.sum())) == (WIDE + 3000, WIDE, 2000)


# ------------------------------------------------------------------ 2: caps, workspace, refusals
def test_the_binding_holds_the_three_wide_entry_points():
    from ggad_amd import _lib
    for name in ("ggad_topk_wide_max_k", "ggad_topk_wide_workspace_elems", "ggad_topk_wide_f32"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["ggad_topk_wide_f32"] == _lib.SIGNATURES["ggad_topk_f32"]           # same arguments
    assert _lib.SIGNATURES["ggad_topk_wide_workspace_elems"] == _lib.SIGNATURES["ggad_topk_workspace_elems"]
    lib = _lib.load()
    assert lib.ggad_abi_version() == _lib.ABI_VERSION == 11
    assert int(lib.ggad_topk_max_k()) == NARROW and int(lib.ggad_topk_wide_max_k()) == WIDE
    ws = lib.ggad_topk_wide_workspace_elems
    for n, k in ((-1, 5), (2 ** 31, 5), (100, 0), (100, WIDE + 1), (100, -1)):
        assert ws(n, k) == 0
    assert ws(0, 1) > 0 and ws(2 ** 31 - 1, WIDE) > 0
    assert ws(1000, 100) < ws(1000000, 100) < ws(1000000, 20000) < ws(1000000, 200000)
    # beside the select stage's words: two buffers of m 64-bit words and one count per 1,024 ranks
    for n, k in ((1000000, 20000), (5000000, WIDE), (3000, 20000), (0, 7)):
        m = max(1, min(n, k))
        assert ws(n, k) == lib.ggad_topk_workspace_elems(n, min(k, NARROW)) + 2 * (k - min(k, NARROW)) + 4 * m + -(-m // 1024)
    assert ws(2 ** 31 - 1, WIDE) * 4 < 100 * 2 ** 20                                           # under 100 MB at the cap
    assert lib.ggad_topk_wide_f32(8, None, 10, 0, 8, 8, None, 8, 8, None) == -1
    assert lib.ggad_topk_wide_f32(8, None, 10, WIDE + 1, 8, 8, None, 8, 8, None) == -1
    assert lib.ggad_topk_wide_f32(None, None, 10, 5, 8, 8, None, 8, 8, None) == -1
    assert lib.ggad_topk_wide_f32(8, None, 10, 5, 8, 8, None, 8, 4, None) == -1                # a workspace off the 8-byte grid


# ------------------------------------------------------------------ 3: check_k
def test_check_k_raises_as_before_and_passes_wide():
    from ggad_amd.metrics import check_k, top_k
    with pytest.raises(ValueError) as exc:
        check_k(NARROW + 1, "top_k")
    assert str(exc.value) == "top_k: k = 16385 is outside 1..ggad_topk_max_k() = 16384 (the pairs one workgroup sorts in LDS)"
    check_k(NARROW, "top_k")
    check_k(NARROW + 1, "top_k", wide=True)
    check_k(WIDE, "top_k", None, True)
    for k in (0, -2, WIDE + 1, 2.5):
        with pytest.raises(ValueError, match=r"ggad_topk_wide_max_k\(\) = 4194304"):
            check_k(k, "top_k", wide=True)
    with pytest.raises(ValueError, match="float32"):
        top_k(torch.zeros(4, dtype=torch.float64), 2, wide=True)
    with pytest.raises(ValueError, match="GPU"):
        top_k(torch.zeros(4), 2, wide=True)


# ------------------------------------------------------------------ 4: the config keys
BASE = dict(data_name="synthetic", data_dir="", seed=72, model="GCN")


def test_top_k_wide_without_top_k_is_a_config_error_naming_both_keys():
    from ggad_amd.model_handler import ModelHandler
    for extra in (dict(), dict(top_k=0)):
        with pytest.raises(ValueError, match="`top_k_wide`.*`top_k: K`"):
            ModelHandler(dict(BASE, top_k_wide=True, **extra))
    with pytest.raises(ValueError, match="data_name"):                       # the key off: the constructor goes on to the loader
        ModelHandler(dict(BASE, top_k_wide=False))


def test_a_large_top_k_without_the_key_is_todays_error_and_legal_with_it():
    from ggad_amd.model_handler import ModelHandler
    for extra in (dict(), dict(top_k_wide=False)):
        with pytest.raises(ValueError) as exc:
            ModelHandler(dict(BASE, top_k=NARROW + 1, **extra))
        assert str(exc.value) == ("config key `top_k`: k = 16385 is outside 1..ggad_topk_max_k() = 16384 (the pairs one workgroup sorts "
                                  "in LDS)")
    for k in (NARROW + 1, WIDE):
        with pytest.raises(ValueError, match="data_name"):
            ModelHandler(dict(BASE, top_k=k, top_k_wide=True))
    with pytest.raises(ValueError, match=r"ggad_topk_wide_max_k\(\)"):
        ModelHandler(dict(BASE, top_k=WIDE + 1, top_k_wide=True))
    with pytest.raises(ValueError, match="top_k.*model: 'GCN'"):
        ModelHandler(dict(BASE, model="SAGE", top_k=20000, top_k_wide=True))


# ------------------------------------------------------------------ 5: run.py's parser, the yml
def _run_py():
    spec = importlib.util.spec_from_file_location("ggad_run_script_topk_wide", os.path.join(ROOT, "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    return run


def test_run_py_parser_without_and_with_the_flag(capsys):
    from ggad_amd.fullgraph_script import select_options, top_k_wide_option
    run = _run_py()
    for argv in ([], ["--score", "w.pt", "--top_k", "50"]):
        a = run.parse(argv)
        assert "top_k_wide" not in vars(a) and top_k_wide_option(a) is False
    a = run.parse(["--score", "w.pt", "--top_k", "20000", "--top_k_wide"])
    assert a.top_k_wide is True and top_k_wide_option(a) is True
    assert select_options(a) == (None, None, "w.pt", 20000, "")                # still five values
    for argv in (["--top_k_wide"], ["--score", "w.pt", "--top_k_wide"], ["--top_k", "20000", "--top_k_wide"]):
        with pytest.raises(SystemExit) as exc:
            run.parse(argv)
        assert exc.value.code == 2
    capsys.readouterr()


def test_main_py_refuses_score_ids_without_score():
    import subprocess
    import sys
    src = os.path.join(ROOT, "src")
    p = subprocess.run([sys.executable, "main.py", "--score_ids", "ids.npy"], cwd=src, capture_output=True, text=True)
    assert p.returncode == 2 and "--score_ids" in p.stderr and "needs --score" in p.stderr
    p = subprocess.run([sys.executable, "main.py", "--help"], cwd=src, capture_output=True, text=True)
    assert p.returncode == 0 and "--top_k_wide" in p.stdout and "--score_ids FILE.npy" in p.stdout


def test_dgraph_yml_carries_the_key_off():
    import yaml
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["top_k_wide"] is False and cfg["top_k"] == 0
