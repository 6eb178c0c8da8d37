"""The capture helper of the full-graph scripts (`ggad_amd.fullgraph_script.CapturedEpoch` / `capture`) on the smallest thing that can
go wrong: one `torch.nn.Linear(4, 4)` under a `FlatAdam`, an epoch of zero_grad / forward on a fixed (8, 4) input plus an (8, 4) noise
buffer / backward / step, 7 epochs.  The loops run once, in a child process under a time limit (this file run as a program prints
what they gave as one JSON line); the tests compare the results.  The mini-batch handlers' form -- `at=1` and a `key` per epoch,
a changed key captured again -- runs on the same model."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

EPOCHS, AT = 7, 2
KEYS = ["a"] * 4 + ["b"] * 3            # the key of every epoch: it changes once, at epoch 4


def _setup():
    import torch
    from ggad_amd.fullgraph import FlatAdam
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lin = torch.nn.Linear(4, 4).to(dev)
    opt = FlatAdam(lin.parameters(), lr=1e-2)
    x = torch.randn(8, 4).to(dev)
    noise = torch.zeros(8, 4, device=dev)
    log = []

    def epoch_fn():
        log.append("epoch_fn (capturing)" if torch.cuda.is_current_stream_capturing() else "epoch_fn")
        opt.zero_grad()
        loss = (lin(x + noise) ** 2).mean()
        loss.backward()
        opt.step()
        return loss.detach()
    return lin, opt, noise, epoch_fn, log


def _result(lin, losses, **more):
    return dict(losses=losses, weight=lin.weight.detach().cpu().flatten().tolist(), bias=lin.bias.detach().cpu().tolist(), **more)


def _helper_loop(enabled=True, gate=None, draws=None):
    """7 epochs through `CapturedEpoch`; `draws`: the host-noise pattern, a fresh CPU draw copied into the buffer before every epoch --
    by the loop while the epochs are eager, by `before_replay` afterwards."""
    from ggad_amd.fullgraph_script import CapturedEpoch
    lin, opt, noise, epoch_fn, log = _setup()
    events, gate_calls = [], []

    def before_capture():
        log.append("before_capture")
        if draws is not None:
            noise.fill_(1e3)            # (what the buffer holds at the capture is never read: the capture executes nothing)
        opt.zero_grad()

    def gate_fn():
        gate_calls.append(epoch)
        return gate()

    cap = CapturedEpoch(epoch_fn, enabled=enabled, at=AT, before_capture=before_capture, after_capture=lambda: log.append("after_capture"),
                        gate=None if gate is None else gate_fn)
    losses = []
    for epoch in range(EPOCHS):
        del log[:]

        def before_replay():
            log.append("before_replay")
            if draws is not None:
                noise.copy_(draws[epoch])
        if draws is not None and epoch < AT:
            noise.copy_(draws[epoch])
        losses.append(cap.step(epoch, before_replay).item())
        events.append(list(log))
    return _result(lin, losses, events=events, captured=cap.captured, gate_calls=gate_calls)


def _keyed_loop(enabled=True, keys=None):
    """7 epochs through `CapturedEpoch(at=1)`, `step` given `keys[epoch]` (None: the keyless form)."""
    from ggad_amd.fullgraph_script import CapturedEpoch
    lin, opt, noise, epoch_fn, log = _setup()
    cap = CapturedEpoch(epoch_fn, enabled=enabled, at=1, before_capture=opt.zero_grad)
    losses, events = [], []
    for epoch in range(EPOCHS):
        del log[:]
        losses.append(cap.step(epoch, lambda: log.append("before_replay"), key=None if keys is None else keys[epoch]).item())
        events.append(list(log))
    return _result(lin, losses, events=events, captured=cap.captured)


def _eager_loop(draws=None):
    lin, opt, noise, epoch_fn, _ = _setup()
    losses = []
    for epoch in range(EPOCHS):
        if draws is not None:
            noise.copy_(draws[epoch])
        losses.append(epoch_fn().item())
    return _result(lin, losses)


def _function_loop():
    from ggad_amd.fullgraph_script import capture
    lin, opt, noise, epoch_fn, _ = _setup()
    losses = [epoch_fn().item() for _ in range(AT)]
    graph, static = capture(epoch_fn, before=opt.zero_grad)
    for _ in range(AT, EPOCHS):
        graph.replay()
        losses.append(static.item())
    return _result(lin, losses)


def _measure():
    import torch
    torch.cuda.set_device(0)
    draws = torch.randn(EPOCHS, 8, 4, generator=torch.Generator().manual_seed(1))
    return dict(eager=_helper_loop(enabled=False), captured=_helper_loop(), gate_closed=_helper_loop(gate=lambda: False),
                gate_open=_helper_loop(gate=lambda: True), noise_eager=_eager_loop(draws), noise_captured=_helper_loop(draws=draws),
                function=_function_loop(), plain_eager=_eager_loop(), keyed=_keyed_loop(keys=KEYS),
                keyed_eager=_keyed_loop(enabled=False, keys=KEYS), keyless_at_1=_keyed_loop())


@pytest.fixture(scope="module")
def res():
    from conftest import ROOT
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__)], cwd=ROOT, capture_output=True, text=True,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1])


def _same(a, b):
    return a["losses"] == b["losses"] and a["weight"] == b["weight"] and a["bias"] == b["bias"]


def test_captured_equals_eager_bit_for_bit(res):
    assert res["captured"]["captured"] is True and res["eager"]["captured"] is False
    assert len(res["captured"]["losses"]) == EPOCHS and len(set(res["captured"]["losses"])) == EPOCHS          # (it trains: no two alike)
    assert _same(res["captured"], res["eager"])
    assert _same(res["eager"], res["plain_eager"])                  # the helper switched off is the plain loop


def test_callbacks_run_once_around_the_capture_and_before_every_replay(res):
    ev = res["captured"]["events"]
    assert ev[:AT] == [["epoch_fn"]] * AT
    assert ev[AT] == ["before_capture", "epoch_fn (capturing)", "after_capture", "before_replay"]
    assert ev[AT + 1:] == [["before_replay"]] * (EPOCHS - AT - 1)               # a replay never calls the epoch function
    assert res["eager"]["events"] == [["epoch_fn"]] * EPOCHS


def test_closed_gate_means_no_capture(res):
    g = res["gate_closed"]
    assert g["captured"] is False and g["gate_calls"] == [AT]
    assert g["events"] == [["epoch_fn"]] * EPOCHS
    assert _same(g, res["eager"])
    o = res["gate_open"]
    assert o["captured"] is True and o["gate_calls"] == [AT] and _same(o, res["eager"])


def test_replay_reads_the_buffer_that_before_replay_filled(res):
    assert res["noise_captured"]["captured"] is True
    assert _same(res["noise_captured"], res["noise_eager"])
    assert res["noise_eager"]["losses"] != res["eager"]["losses"]               # (the draws matter)


def test_function_form_equals_the_helper(res):
    assert _same(res["function"], res["captured"])


def test_a_key_that_differs_from_the_captured_one_is_captured_again(res):
    """Two captures, at epoch 1 (`at`) and at epoch 4 (the key changes); every other epoch from 1 on replays; bit for bit the
    `enabled=False` run."""
    ev = res["keyed"]["events"]
    assert ev[0] == ["epoch_fn"]
    assert ev[1] == ev[4] == ["epoch_fn (capturing)", "before_replay"]
    assert ev[2] == ev[3] == ev[5] == ev[6] == ["before_replay"]
    assert res["keyed"]["captured"] is True and res["keyed_eager"]["captured"] is False
    assert res["keyed_eager"]["events"] == [["epoch_fn"]] * EPOCHS
    assert _same(res["keyed"], res["keyed_eager"]) and _same(res["keyed_eager"], res["plain_eager"])


def test_without_a_key_the_same_epochs_are_captured_once(res):
    ev = res["keyless_at_1"]["events"]
    assert ev[0] == ["epoch_fn"] and ev[1] == ["epoch_fn (capturing)", "before_replay"]
    assert ev[2:] == [["before_replay"]] * (EPOCHS - 2)
    assert _same(res["keyless_at_1"], res["plain_eager"])


if __name__ == "__main__":
    print(json.dumps(_measure()))
