"""What the mini-batch handlers share (`ggad_amd/handler_loop.py`), without a GPU: the best-checkpoint rule on a two-parameter
`nn.Linear`, and the batch schedule of the labelled-batch loop driven with a stub step -- python lists under `random.shuffle` against
int64 arrays under `PyCompatRandom`, on the shapes of `test_distributed_cpu.test_world_one_is_the_reference_schedule`."""
import argparse
import operator
import os
import random

import numpy as np
import torch

from ggad_amd.handler_loop import BestCheckpoint, train_labelled
from ggad_amd.sampler import PyCompatRandom


def _linear(value):
    lin = torch.nn.Linear(1, 1)
    with torch.no_grad():
        lin.weight.fill_(value)
        lin.bias.fill_(-value)
    return lin


def test_best_checkpoint_saves_on_a_strictly_better_auc_and_restores_the_last_save(tmp_path, capsys):
    best = BestCheckpoint(str(tmp_path) + "/run/", "dgraphfin", "SAGE")
    assert best.ep_best == -1 and best.path_saver == os.path.join(best.dir_saver, "dgraphfin_SAGE.pkl")
    assert best.dir_saver.startswith(str(tmp_path) + "/run/") and len(best.dir_saver) == len(str(tmp_path) + "/run/") + 19     # %Y-%m-%d %H-%M-%S
    saved, ep = [], []
    for epoch, auc in enumerate((0.0, 0.6, 0.6, 0.7, 0.5)):
        best.offer(epoch, 0.1 * epoch, auc, _linear(float(epoch)))
        saved.append("  Saving model ...\n" == capsys.readouterr().out)
        ep.append(best.ep_best)
        if epoch == 0:
            assert not os.path.exists(best.dir_saver)          # 0.0 does not beat the initial 0: nothing on disk yet
    assert saved == [False, True, False, True, False]
    assert ep == [-1, 1, 1, 3, 3] and best.auc_best == 0.7 and best.f1_mac_best == 0.1 * 3
    model = _linear(9.0)
    best.restore(model)
    assert capsys.readouterr().out == "Restore model from epoch 3\nModel path: {}\n".format(best.path_saver)
    assert model.weight.item() == 3.0 and model.bias.item() == -3.0


def test_best_checkpoint_that_does_not_write_follows_the_rule_in_silence(tmp_path, capsys):
    best = BestCheckpoint(str(tmp_path) + "/rank1/", "dgraphfin", "GCN", write=False)
    for epoch, auc in enumerate((0.0, 0.6, 0.6, 0.7, 0.5)):
        best.offer(epoch, 0.0, auc, _linear(float(epoch)))
    model = _linear(9.0)
    best.restore(model)
    assert best.ep_best == 3 and model.weight.item() == 9.0
    assert capsys.readouterr().out == "" and not os.path.exists(best.dir_saver) and os.listdir(tmp_path) == []


def test_best_checkpoint_without_a_successful_offer_restores_nothing(tmp_path, capsys):
    best = BestCheckpoint(str(tmp_path) + "/none/", "dgraphfin", "SAGE")
    best.offer(0, 0.0, 0.0, _linear(1.0))
    model = _linear(9.0)
    best.restore(model)
    assert best.ep_best == -1 and model.weight.item() == 9.0
    assert capsys.readouterr().out == "" and os.listdir(tmp_path) == []


def _drive(tmp_path, train, pool, labels, **order):
    """2 epochs x 5 batches of 30 + 10 through `train_labelled` with a step that only records; returns the batches."""
    args = argparse.Namespace(num_batches=5, n_pseudo=10, batch_size=30, num_epochs=2, valid_epochs=1, thres=0.5, model="SAGE",
                              data_name="synthetic", save_dir=str(tmp_path) + "/")
    dataset = {"labels": labels, "idx_test": [1, 2, 3], "y_test": [0, 1, 0]}
    batches, log, lines, sweeps = [], [], [], []

    def step(batch_nodes, batch_label):
        assert np.array_equal(batch_label, labels[np.asarray(batch_nodes)])
        batches.append([int(v) for v in batch_nodes])
        return (torch.tensor(float(len(batches))),)

    def sweep(cases, y, model, batch_size, thres):
        sweeps.append((list(cases), list(y), batch_size, thres))
        return 0.0, 0.0, 0.0, 0.0, 0.0                           # an AUC that never beats the initial 0: nothing is saved

    res = train_labelled(args, dataset, None, train, pool, step=step, report=lambda *a: lines.append(a), sweep=sweep, log=log, **order)
    assert res == (0.0, 0.0, 0.0, 0.0, 0.0) and sweeps == [([1, 2, 3], [0, 1, 0], 30, 0.5)] * 3       # two validations, the test sweep
    assert log == [float(i) for i in range(1, 11)]
    assert [(e, m) for e, m, _ in lines] == [(0, [3.0]), (1, [8.0])]                              # the mean loss of each epoch
    assert os.listdir(tmp_path) == []
    return batches


def test_labelled_loop_draws_the_same_schedule_from_lists_and_from_arrays(tmp_path, capsys):
    labels = np.zeros(3000, dtype=np.int64)
    pool = np.arange(100, 400)
    labels[pool] = 1
    train = np.arange(400, 2400)
    random.seed(72)
    from_lists = _drive(tmp_path, train.tolist(), pool.tolist(), labels, shuffle=random.shuffle, join=operator.add)
    state_lists = random.getstate()
    random.seed(72)
    rng = PyCompatRandom.from_python_state(random.getstate())
    from_arrays = _drive(tmp_path, train.copy(), pool.copy(), labels, shuffle=rng.shuffle, join=lambda a, b: np.concatenate([a, b]))
    random.setstate(rng.to_python_state())                       # the stream handed back, as the device path does
    assert random.getstate() == state_lists
    assert len(from_lists) == 10 and all(len(b) == 40 for b in from_lists) and from_lists == from_arrays
    # the reference's schedule, restated (src/model_handler.py:314,333-347)
    random.seed(72)
    tr, pl = train.tolist(), pool.tolist()
    for epoch in range(2):
        random.shuffle(tr)
        for b in range(5):
            random.shuffle(pl)
            assert from_lists[epoch * 5 + b] == tr[b * 30:(b + 1) * 30] + pl[:10]
    assert capsys.readouterr().out == "Valid at epoch 0\nValid at epoch 1\n" * 2
