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
