"""`bench.py --dump-outputs DIR`: the last timed step's outputs as float32 .npy files, identical inputs for identical arguments."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("losses", "weight", "enc.weight", "enc.fc.weight", "exp_avg", "exp_avg_sq")


def _bench_module():
    spec = importlib.util.spec_from_file_location("ggad_bench_cli", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_float32_arrays_and_steps_must_be_positive(tmp_path, monkeypatch):
    bench = _bench_module()
    D, F = 4, 3
    params = torch.arange(D + D * F + D * D, dtype=torch.float32)
    engine = types.SimpleNamespace(weight=params[:D].view(1, D), enc_weight=params[D:D + D * F].view(D, F),
                                   enc_fc_weight=params[D + D * F:].view(D, D), exp_avg=torch.full((params.numel(),), 0.5),
                                   exp_avg_sq=torch.full((params.numel(),), 0.25))
    bench.dump_outputs(str(tmp_path / "out"), engine, np.array([1.0, 0.5, 0.25, 0.125]))
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in NAMES}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["enc.weight"].shape == (D, F) and got["enc.fc.weight"].shape == (D, D) and got["weight"].shape == (1, D)
    np.testing.assert_array_equal(np.concatenate([got[n].ravel() for n in ("weight", "enc.weight", "enc.fc.weight")]), params.numpy())
    np.testing.assert_array_equal(got["losses"], [1.0, 0.5, 0.25, 0.125])
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert a.full is False and a.no_extras is False and (a.steps, a.warmup) == (20, 5)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-extras"])
    a = bench.parse()
    assert a.full is True and a.no_extras is True


@pytest.mark.gpu
def test_bench_dump_outputs_same_arguments_same_outputs(tmp_path):
    """Two runs with the same arguments dump the same last step (the inputs are seeded); the loss row is the line's last_loss,
    and the whole dump stays far below 64 MB."""
    runs = []
    for tag in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "10", "--nodes", "200000",
               "--entries", "4000000", "--chunk", "20", "--no-extras", "--dump-outputs", str(tmp_path / tag)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 40 and line["ms_per_step"] > 0
        got = {n: np.load(tmp_path / tag / (n + ".npy")) for n in NAMES}
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
        assert sum(os.path.getsize(tmp_path / tag / (n + ".npy")) for n in NAMES) < 64 << 20
        assert got["losses"].shape == (4,) and float(got["losses"][0]) == pytest.approx(line["last_loss"], rel=1e-6)
        runs.append(got)
    for n in NAMES:
        np.testing.assert_allclose(runs[0][n], runs[1][n], rtol=1e-5, atol=1e-6, err_msg=n)


@pytest.mark.gpu
def test_bench_plain_run_measures_the_timed_region_only(tmp_path):
    """A plain run prints the headline without the roofline, the value repeats, the extra legs or the CPU baselines; `--full
    --no-extras` adds the roofline with its per-kernel entries from an instrumented repeat of the one-chunk window.  The timed
    steps are the same either way: both runs dump the same last step."""
    lines, dumps = {}, {}
    for tag, extra in (("plain", []), ("full", ["--full", "--no-extras"])):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--nodes", "200000",
               "--entries", "4000000", "--chunk", "20", "--dump-outputs", str(tmp_path / tag)] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines[tag] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        dumps[tag] = {n: np.load(tmp_path / tag / (n + ".npy")) for n in NAMES}
    plain, full = lines["plain"], lines["full"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["full"] is False
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["value_repeats"] is None and plain["multi_gpu"] is None
    assert not {"steady_state", "e2e_with_sampler", "dgraph_sparse_regime", "fullgraph"} & set(plain)
    assert full["full"] is True and full["value_repeats"] is None and full["cpu_baseline"] is None
    roof = full["roofline"]
    assert roof["launches"] == 1 and roof["achieved"] > 0 and "repeat" in roof["by_kernel_measured_in"]
    assert len(roof["by_kernel"]) >= 2 and all(k["avg_launch_ms"] > 0 for k in roof["by_kernel"])
    for n in NAMES:
        np.testing.assert_allclose(dumps["plain"][n], dumps["full"][n], rtol=1e-5, atol=1e-6, err_msg=n)
