"""Full-graph AnomalyDAE at the published sizes (`fullgraph_bench.SIZES`: Reddit 10,984 nodes, Amazon 11,944 / 4.4 M entries,
Photo 7,535 / 745 features, T-Finance 39,357 / 21.2 M entries, Elliptic 46,564): one whole training step of `anomalyDAE.py` --
`Model.forward` on normal_idx and idx_test, backward, FlatAdam at the script's lr -- through the HIP kernels against the sparse
float64 oracle (`oracle/ggad_oracle.py`: `adae_forward`, `adae_recon`, torch autograd, `adam_f64` with weight_decay 0), run by
torch in float64 on the device, plus bit-determinism of everything.  The oracle is pinned to the dense formulation and to the
reference's captures in tests/test_anomalydae_cpu.py.

Each size is asserted to reach the kernels' long-loop branches it has: a GAT target with 64 or more stored in-entries (all but
Elliptic, whose largest in-degree is 4), more than 64 column blocks per loss row (N > 16,384: T-Finance, Elliptic) and more than
1,024 loss rows (all but Photo, whose 1,022 normal rows are just below).

Tolerances (|HIP - float64|, relative to the largest magnitude of the float64 tensor, as test_fullgraph_fullsize_gpu.py):
  * z, x_hat: 2e-5 -- fp32 GEMMs over K = F or 300 and the GAT's softmax sums over up to 7,368 in-entries (sqrt(7,368) x 6e-8
    = 5e-6 of rounding walk);
  * loss and test scores: 2e-5 -- the score's own sums carry 90 roundings (tests/test_anomalydae_branches_gpu.py), on top of
    the z and x_hat deviations above carried through sigmoid and the norms (slopes at most 1);
  * gradients: 1e-4, the suite's full-size gradient tolerance, plus 1e-6 absolute (100 eps, the level below which
    tests/step_reference.py treats a gradient as unresolved).  The floor matters where the float64 gradient is itself below
    it: at Photo size z_i . z_j exceeds 17 for most pairs at initialisation (745 features in [0, 1]), fp32's sigmoid returns
    exactly 1.0 there and s (1 - s) = 0 where float64 has e^-x, so everything upstream of z (dense_stru, gat_layer) gets a
    float64 gradient of 3e-7 at most that no fp32 evaluation resolves; and d att_dst is 0 in exact arithmetic wherever every
    target's incoming pre-activations share one leaky-ReLU slope (Amazon, Elliptic: float64 leaves 1e-19);
  * weights after one Adam step: 3e-3 lr where the gradient is above 1e-6 of its tensor's scale and above 1e-6 (100 eps),
    elsewhere at most one opposite step (2.1 lr) -- tests/step_reference.py explains the mask: a fresh Adam step is lr g / (|g| +
    eps), +-lr unless |g| is within a few hundred eps of 0.  3e-3 lr is step_reference's 3e-6 at lr 1e-3, scaled to the lr.
"""
import random

import numpy as np
import pytest
import torch

from ggad_amd.fullgraph_bench import SIZES, make_dataset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HAS_HUB = {"reddit", "Amazon", "photo", "t_finance"}
MANY_BLOCKS = {"t_finance", "elliptic"}
MANY_ROWS = {"reddit", "Amazon", "t_finance", "elliptic"}


def _step(ds, full, lr):
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.model_anomalydae import Model
    torch.manual_seed(0)
    model = Model(ds["f"], 300, "prelu", 1, "avg").to(DEV)
    init = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = FlatAdam(model.parameters(), lr=lr, weight_decay=0.0)
    feats = torch.from_numpy(ds["features"])[None].to(DEV)
    model.train()
    opt.zero_grad()
    loss, score = model(feats, full, ds["normal_idx"], ds["idx_test"])
    loss.backward()
    with torch.no_grad():
        xhat, z = model.model_enc(feats[0], full)
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    opt.step()
    torch.cuda.synchronize()
    return dict(loss=loss.detach().reshape(1).clone(), score=score.clone(), z=z.clone(), xhat=xhat.clone(), grads=grads,
                weights={k: p.detach().clone() for k, p in model.named_parameters()}, init=init)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", ["reddit", "Amazon", "photo", "t_finance", "elliptic"])
def test_training_step_at_full_size_against_the_oracle(name):
    import scipy.sparse as sp
    from anomalyDAE import LR
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.utils import normalize_adj
    from oracle import ggad_oracle as O
    random.seed(0)
    np.random.seed(0)
    ds = make_dataset(name, 0)
    n, f = ds["n"], ds["f"]
    assert (n, f) == (SIZES[name][0], SIZES[name][2])
    full = FullGraphAdj(normalize_adj(ds["adj"]) + sp.eye(n), ds["adj"] + sp.eye(n), DEV)
    a = full.A.host
    nrm, tst = ds["normal_idx"], ds["idx_test"]
    assert (np.bincount(a.indices, minlength=n).max() >= 64) == (name in HAS_HUB)
    assert (-(-n // 256) > 64) == (name in MANY_BLOCKS)
    assert (len(nrm) > 1024) == (name in MANY_ROWS)
    lr = LR[name]
    got = _step(ds, full, lr)

    # ---- the float64 oracle on the device: same initial weights, A_hat as the kernels hold it (fp32 values)
    P = {k: got["init"][k].double().requires_grad_(True) for k in O.ADAE_PARAM_ORDER}
    assert sorted(got["init"]) == sorted(O.ADAE_PARAM_ORDER + ["disc.f_k.weight", "disc.f_k.bias"])
    A = (a.indptr, a.indices, a.data.astype(np.float32))
    x = torch.from_numpy(ds["features"]).to(DEV).double()
    xhat, z = O.adae_forward(P, x, A)
    loss, _, _, _ = O.adae_recon(z, xhat, x, A, nrm)
    loss.backward()
    with torch.no_grad():
        score = O.adae_recon(z, xhat, x, A, tst)[1]
    print(f"[{name}] N={n} F={f} |R|={len(nrm)} test={len(tst)} loss {loss.item():.6f}")

    def close(a_, b_, what, tol, floor=0.0):
        b_ = b_.detach()
        scale = float(b_.abs().max()) + 1e-30
        err = float((a_.double() - b_).abs().max())
        print(f"  {what}: max |HIP - f64| = {err:.2e}, / scale = {err / scale:.2e} (scale {scale:.3e})")
        assert err < tol * scale + floor, (name, what, err, scale)
    close(got["loss"], loss.reshape(1), "loss", 2e-5)
    close(got["score"], score, "test scores", 2e-5)
    close(got["z"], z, "z", 2e-5)
    close(got["xhat"], xhat, "x_hat", 2e-5)
    assert sorted(got["grads"]) == sorted(O.ADAE_PARAM_ORDER)                   # the discriminator gets no gradient
    for k in O.ADAE_PARAM_ORDER:
        close(got["grads"][k], P[k].grad, "grad " + k, 1e-4, floor=1e-6)
    worst = 0.0
    for k in O.ADAE_PARAM_ORDER:
        g = P[k].grad.cpu().numpy()
        p_ref = O.adam_f64(P[k].detach().cpu().numpy(), 0.0, 0.0, g, 1, lr, 0.0)[0]
        sure = (np.abs(g) > 1e-6 * (np.abs(g).max() + 1e-30)) & (np.abs(g) > 1e-6)
        d = np.abs(got["weights"][k].cpu().numpy() - p_ref)
        if sure.any():
            worst = max(worst, float(d[sure].max()))
            assert d[sure].max() < 3e-3 * lr, (name, k, float(d[sure].max()))
        assert d.max() < 2.1 * lr, (name, k, float(d.max()))                    # at most one opposite Adam step
    print(f"  weights after the Adam step: max |HIP - f64| = {worst:.2e} (lr {lr:g})")
    for k in ("disc.f_k.weight", "disc.f_k.bias"):
        assert torch.equal(got["weights"][k], got["init"][k]), k               # no gradient: not touched

    # ---- bit-determinism: the same step from the same state gives the same bits everywhere
    again = _step(ds, full, lr)
    for k in ("loss", "score", "z", "xhat"):
        assert _bits_equal(got[k], again[k]), k
    for k in got["grads"]:
        assert _bits_equal(got["grads"][k], again["grads"][k]), k
    for k in got["weights"]:
        assert _bits_equal(got["weights"][k], again["weights"][k]), k
