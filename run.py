#!/usr/bin/env python3
"""Full-graph GGAD on one MI355X:  python run.py --dataset reddit [--synthetic]

Same command line and per-dataset overrides as the reference's `run.py` (`:18-66`: lr 1e-3; epochs photo 100 /
elliptic 150 / reddit 300 / t_finance 500 / Amazon 800; noise N(0.02, 0.01) for reddit and photo, else 0), same
seeding, same prints, same evaluation cadence (AUROC / AP on idx_test every 10 epochs with sklearn).  The
arithmetic of the epoch -- two GCN layers, outlier generation, scorer MLP, BCE + local-affinity margin +
reconstruction loss, backward, Adam -- runs in the HIP kernels of libggad_hip.so (sparse CSR / edge-parallel
instead of the reference's dense N x N tensors).  Extra flags: `--synthetic` (no dataset ships with this repo:
builds a graph of the dataset's published size from the seed), `--device`, `--device_noise` (opt-in: the N(mean, var)
noise is drawn on the device from torch's own CPU stream, `ggad_amd/rng.py`; the draw opens the captured epoch).
`--select auroc|ap` (opt-in): every epoch ends with a noise-free scoring forward, the validation AUROC / AP on idx_val and a
conditional snapshot of the weights, all on the device and inside the captured epoch (`ggad_amd/select.py`); the trajectory and
the CPU generator are untouched.  `--save PATH` writes the weights (the best epoch's with `--select`, else the last epoch's),
`--score PATH [--top_k K] [--top_k_out F.npz]` scores the graph from such a file without training and ranks its test nodes;
`--top_k_wide` ranks through csrc/topk.hip, K above 16,384 up to 4,194,304 (the whole test split of T-Finance or Elliptic).
`--auc_ci [LEVEL]` (after training or with `--score`) prints the test AUROC with DeLong's standard error and interval; `--score A.pt
--compare B.pt` tests the AUROCs of two checkpoints against each other on idx_test (`metrics.auc_ci` / `compare_auc`).
`--ap_ci [LEVEL] [--boot_reps B] [--boot_seed S]` (at the same places) prints the test average precision and AUROC with the percentile
intervals of a stratified bootstrap made on the device (`metrics.ap_ci`).  `--score A.pt --compare B.pt --compare_ap [LEVEL]` also tests
the two average precisions against each other by a paired bootstrap (`metrics.compare_ap`; `--boot_reps`, `--boot_seed`).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ggad_amd.fullgraph import FlatAdam, ggad_loss  # noqa: E402
from ggad_amd.fullgraph_script import (SIZES, CapturedEpoch, add_bootstrap_options, add_compare_options, add_select_options,  # noqa: E402,F401
                                       add_threshold_options, bootstrap_options, check_bootstrap_options, check_compare_options,
                                       check_select_options, check_threshold_options, choose_threshold, compare_ap_option,
                                       compare_options, init_process, load_checkpoint, load_graph, make_parser, parse_with_defaults,
                                       prepare, print_ap_ci, print_auc_ci, print_captured, print_compare, print_compare_ap, print_eval,
                                       print_median, print_threshold_test, save_checkpoint, score_from_checkpoint, select_options,
                                       threshold_option)
from ggad_amd.metrics import average_precision, roc_auc  # noqa: E402
from ggad_amd.model import Model  # noqa: E402

EPOCHS = {"photo": 100, "elliptic": 150, "reddit": 300, "t_finance": 500, "Amazon": 800}


def parse(argv=None):
    p = make_parser("reddit", sampling=False,
                    no_graph_help="launch every kernel of every epoch from Python instead of replaying a captured hipGraph of the "
                                  "training epoch (same kernels, same order, same results)",
                    device_noise_help="draw the N(mean, var) noise on the device from torch's own CPU stream (ggad_amd.rng): the draw "
                                      "becomes the first node of the captured epoch; values agree with the host's to float32 rounding")
    p.add_argument("--mean", type=float, default=0.0)
    p.add_argument("--var", type=float, default=0.0)
    add_select_options(p)
    add_threshold_options(p)
    add_compare_options(p)
    add_bootstrap_options(p)
    a = check_threshold_options(p, check_select_options(p, parse_with_defaults(p, argv, {}, EPOCHS, fallback=(1e-3, 100))))
    a = check_bootstrap_options(p, check_compare_options(p, a))
    a.mean, a.var = (0.02, 0.01) if a.dataset in ["reddit", "photo"] else (0.0, 0.0)      # run.py:61-66 (CLI values overwritten)
    return a


def load(args):
    g = load_graph(args)
    return g.adj, g.feat, g.ano_label, g.idx_test, g.normal_idx, g.abn_idx


def main(argv=None):
    """Train (returns None) or, with `--score`, score from a checkpoint (returns the (N,) float32 scores of all nodes)."""
    args = parse(argv)
    print("Dataset: ", args.dataset)
    dev = init_process(args, "run.py", why="the GGAD hot path has no CPU fallback")
    g = load_graph(args)
    print(g.adj.sum())
    full, feats, ft_size = prepare(args, g.adj, g.feat, dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    if select_options(args)[2]:
        try:
            scores = score_from_checkpoint(args, model, lambda: model.score(feats, full), ft_size, g.idx_test, g.ano_label, dev)[0]
            level, other = compare_options(args)
            if level:
                print_auc_ci(level, scores, g.idx_test, g.ano_label, dev)
            if bootstrap_options(args)[0]:
                print_ap_ci(bootstrap_options(args), scores, g.idx_test, g.ano_label, dev)
            if other:                                    # the same model and graph under the second checkpoint's weights
                model.load_state_dict(load_checkpoint(other, ft_size, args.embedding_dim)["state_dict"], strict=True)
                model.eval()
                scores_b = model.score(feats, full)
                print_compare(scores, scores_b, g.idx_test, g.ano_label, dev)
                if compare_ap_option(args):
                    print_compare_ap((compare_ap_option(args),) + bootstrap_options(args)[1:], scores, scores_b, g.idx_test, g.ano_label, dev)
        except ValueError as exc:
            sys.exit("run.py --score: {}".format(exc))
        return scores.cpu().numpy()
    fit(args, dev, full, feats, model, g.normal_idx, g.abn_idx, g.idx_test, g.ano_label, idx_val=g.idx_val)


def fit(args, dev, full, feats, model, normal_label_idx, abnormal_label_idx, idx_test, ano_label, history=None, idx_val=None):
    """`_fit`, on the host's noise (the default) or -- `args.device_noise`, or GGAD_DEVICE_NOISE=1 where `args` does not say -- with the
    CPU generator continued on the device (ggad_amd.rng): snapshotted before the first epoch, handed back when the loop ends, also
    on an exception."""
    device_noise = getattr(args, "device_noise", None)
    if device_noise is None:
        device_noise = os.environ.get("GGAD_DEVICE_NOISE", "0") == "1"
    if not device_noise:
        return _fit(args, dev, full, feats, model, normal_label_idx, abnormal_label_idx, idx_test, ano_label, history, idx_val=idx_val)
    from ggad_amd.rng import DeviceMT
    mt = DeviceMT.from_host(dev)
    model.device_noise = mt
    if history is not None:
        history["noise"] = "device"
    try:
        return _fit(args, dev, full, feats, model, normal_label_idx, abnormal_label_idx, idx_test, ano_label, history, mt, idx_val=idx_val)
    finally:
        model.device_noise = model.noise_override = None
        mt.to_host()


def _fit(args, dev, full, feats, model, normal_label_idx, abnormal_label_idx, idx_test, ano_label, history=None, device_mt=None,
         idx_val=None):
    """The training loop of the reference's script (`run.py:137-240`): Adam, `num_epoch` epochs, an evaluation forward (which draws
    noise too, quirk 5) every 10th epoch.  `history` (a dict, tests / the end-of-training parity report): filled with the four loss
    terms of every epoch, the AUROC / AP of every evaluation, and -- one extra evaluation after the last epoch, which the reference
    does not run -- the final scores of all nodes.

    `args.select` ("auroc" / "ap"; needs `idx_val`): every epoch ends, after the optimiser step and inside the captured epoch, with
    `Model.score` (no noise draw) and `BestKeeper.step` -- validation AUROC / AP on `idx_val` as exact counts, the decision and the
    conditional snapshot of the weights, launches only.  Nothing of the training reads what they write, so losses, weights and the CPU
    generator are those of a run without it.  After the loop (and after everything a run without it does) the best epoch is printed,
    its weights are loaded into `model` and evaluated on `idx_test`; `history` gains `val_curve` ((epochs, 3): AUROC, AP, status),
    `best_epoch`, `best_value`, `best_scores` (all N logits under the best weights), `best_auc` / `best_ap` (on `idx_test`) and
    `last_params` (the last epoch's weights, which `model` no longer holds).  `args.save`: the weights `model` ends with are written."""
    nb_nodes = feats.shape[1]
    select, save = select_options(args)[:2]
    keeper = None
    if select:
        if idx_val is None:
            raise ValueError("--select validates on idx_val: pass fit(..., idx_val=...)")
        from ggad_amd.select import BestKeeper
        rows = np.asarray(idx_val, dtype=np.int64)
        keeper = BestKeeper(list(model.parameters()), args.num_epoch, select, labels_u8=np.asarray(ano_label).reshape(-1)[rows], rows=rows)
    optimiser = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    ls = full.loss_structs(normal_label_idx, abnormal_label_idx)
    idx_test_dev = torch.as_tensor(np.asarray(idx_test, dtype=np.int64), device=dev)
    y_test_dev = torch.as_tensor(np.asarray(ano_label)[np.asarray(idx_test, dtype=np.int64)].astype(np.int64), device=dev)
    total_time = 0.0
    epoch_times = []
    # One training epoch = ~125 small launches driven by Python autograd; on the small graphs the host is the bottleneck
    # (Reddit: 1.3 ms of kernels per 2.3 ms epoch).  After two eager epochs (allocations, plan caches, Adam state) the epoch
    # is captured once and replayed; the N(mean, var) noise is still drawn from the CPU generator every epoch, exactly as
    # the reference does (model.py:143), and copied into the static buffer the captured epoch reads.
    noise_buf, pending_noise = None, None
    n_abn = len(abnormal_label_idx)

    one = torch.ones((), dtype=torch.float32, device=dev)
    device_buf = torch.zeros(1, n_abn, args.embedding_dim, device=dev) if device_mt is not None else None

    def train_epoch():
        if device_mt is not None:                # the first launches of the epoch: this epoch's draw, on the device
            model.noise_override = device_mt.randn_(device_buf, args.var, args.mean)
        optimiser.zero_grad()
        emb, emb_combine, logits, emb_con, emb_abnormal = model(feats, full, abnormal_label_idx, normal_label_idx, True, args)
        if device_mt is not None:
            model.noise_override = None          # (the evaluation forward draws for itself: model.device_noise)
        out = ggad_loss(emb, logits, emb_con, emb_abnormal, full, ls, 0.7)
        out[0].backward(gradient=one)            # (d loss / d loss = 1 from a kept tensor: autograd would fill a new one every epoch)
        optimiser.step()
        if keeper is not None:                   # the last launches of the epoch: score, validate, keep the weights if they are the best
            keeper.step(model.score(feats, full))
        return tuple(t.detach() for t in out)

    def before_capture():
        nonlocal noise_buf
        if device_mt is None:
            noise_buf = model.noise_override = torch.zeros(1, n_abn, args.embedding_dim, device=dev)
        optimiser.zero_grad()

    def after_capture():
        model.noise_override = None
        if device_mt is not None:
            print_captured()

    def host_draw():
        nonlocal pending_noise
        noise = pending_noise
        if noise is None:
            noise = torch.randn(1, n_abn, args.embedding_dim) * args.var + args.mean  # same draw as Model.forward
        pending_noise = None
        noise_buf.copy_(noise)

    # (where launch gaps matter: an eager epoch under 20 ms -- T-Finance size, 5.3 ms of kernels, still gains 2.5 %)
    cap = CapturedEpoch(train_epoch, enabled=not args.no_graph, before_capture=before_capture, after_capture=after_capture,
                        gate=lambda: epoch_times[1] < float(os.environ.get("GGAD_CAPTURE_BELOW_S", "20e-3")))
    for epoch in range(args.num_epoch):
        start_time = time.time()
        model.train()
        # (under device noise the draw is the first node of the captured epoch: nothing to do on the host)
        loss, loss_margin, loss_bce, loss_rec = cap.step(epoch, host_draw if device_mt is None else None)
        # the next epoch's draw while the GPU runs this one -- unless an evaluation (which draws too) comes in between
        if cap.captured and device_mt is None and epoch % 10 != 0 and epoch + 1 < args.num_epoch:
            pending_noise = torch.randn(1, n_abn, args.embedding_dim) * args.var + args.mean
        torch.cuda.synchronize()
        epoch_times.append(time.time() - start_time)
        total_time += epoch_times[-1]
        if history is not None:
            history.setdefault("losses", []).append([loss.item(), loss_margin.item(), loss_bce.item(), loss_rec.item()])
        if not args.quiet:
            print("Total time is", total_time)
        if epoch % 2 == 0 and not args.quiet:
            print("Epoch:", "%04d" % epoch, "train_loss_margin=", "{:.5f}".format(loss_margin.item()))
            print("Epoch:", "%04d" % epoch, "train_loss_bce=", "{:.5f}".format(loss_bce.item()))
            print("Epoch:", "%04d" % epoch, "rec_loss=", "{:.5f}".format(loss_rec.item()))
            print("Epoch:", "%04d" % epoch, "train_loss=", "{:.5f}".format(loss.item()))
            print("=====================================================================")
        if epoch % 10 == 0:
            model.eval()
            with torch.no_grad():
                _, _, logits_eval, _, _ = model(feats, full, abnormal_label_idx, normal_label_idx, False, args)
            scores = logits_eval[0, idx_test_dev, 0]                          # stays in HBM: device sort + fp64 prefix sums
            auc, ap = print_eval(args.dataset, scores, y_test_dev)            # run.py:236-238
            if history is not None:
                history.setdefault("eval", []).append([epoch, auc, ap])
    if history is not None:
        model.eval()
        with torch.no_grad():
            _, _, logits_eval, _, _ = model(feats, full, abnormal_label_idx, normal_label_idx, False, args)
        scores = logits_eval[0, idx_test_dev, 0]
        history["final_logits"] = logits_eval[0, :, 0].cpu().numpy()
        history["final_auc"], history["final_ap"] = roc_auc(scores, y_test_dev), average_precision(scores, y_test_dev)
        history["captured"] = cap.captured
    print("nodes/s (training window, run.py:146->214): {:.1f}".format(nb_nodes * args.num_epoch / total_time))
    print_median(epoch_times, nb_nodes, "one-off plan building / module load")
    best_epoch, best_value = args.num_epoch - 1, None
    if keeper is not None:
        curve, best_epoch, best_value = keeper.curve(), keeper.best_epoch, keeper.best_value
        if history is not None:
            history["val_curve"], history["best_epoch"], history["best_value"] = curve, best_epoch, best_value
            history["last_params"] = [p.detach().cpu().clone() for p in model.parameters()]
        if best_epoch < 0:
            raise RuntimeError("--select {}: no epoch had a defined validation metric (statuses {}): is one class missing from idx_val?"
                               .format(select, sorted(set(curve[:, 2].tolist()))))
        print("[select] best epoch {:04d} by validation {}: validation AUC:{:.4f} AP: {}".format(
            best_epoch, select, curve[best_epoch, 0], curve[best_epoch, 1]))
        keeper.load_into(model)
        model.eval()
        best_scores = model.score(feats, full)
        auc, ap = print_eval(args.dataset, best_scores.index_select(0, idx_test_dev), y_test_dev, prefix="[select] best epoch: ")
        if history is not None:
            history["best_scores"], history["best_auc"], history["best_ap"] = best_scores.cpu().numpy(), auc, ap
    point = None
    if threshold_option(args):                   # `model` holds the weights that --save writes: the kept epoch's, else the last epoch's
        if idx_val is None:
            raise ValueError("--threshold chooses on idx_val: pass fit(..., idx_val=...)")
        model.eval()
        with torch.no_grad():
            all_scores = model.score(feats, full).detach()
        point = choose_threshold(threshold_option(args), all_scores, idx_val, ano_label, dev)
        print_threshold_test(all_scores.index_select(0, idx_test_dev), y_test_dev, point.thres)
        if history is not None:
            history["threshold"], history["threshold_scores"] = point, all_scores.cpu().numpy()
    if compare_options(args)[0] or bootstrap_options(args)[0]:    # --auc_ci, --ap_ci: idx_test under the weights `model` ends with,
        model.eval()                                              # scored once for both
        with torch.no_grad():
            end_scores = model.score(feats, full).detach()
        if compare_options(args)[0]:
            ci = print_auc_ci(compare_options(args)[0], end_scores, idx_test, ano_label, dev)
            if history is not None:
                history["auc_ci"] = ci
        if bootstrap_options(args)[0]:
            ci = print_ap_ci(bootstrap_options(args), end_scores, idx_test, ano_label, dev)
            if history is not None:
                history["ap_ci"] = ci
    if save:
        state = keeper.state_dict(model) if keeper is not None else model.state_dict()
        save_checkpoint(save, state, args, feats.shape[2], nb_nodes, best_epoch, best_value, threshold=point)
        print("weights of epoch {:04d} written to {}".format(best_epoch, save))


if __name__ == "__main__":
    main()
