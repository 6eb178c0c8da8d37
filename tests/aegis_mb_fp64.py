"""Torch restatement of the mini-batch AEGIS discriminator step (`csrc/aegis_mb.hip`; reference `src/graphsage_aegis.py:167-173,
298-323` as `oracle/ggad_oracle.py::aegis_forward / aegis_mlp / aegis_loss` restate it) from the two aggregates of a batch and the
seven tensors, at a chosen dtype: the yardstick (float64) and the measure of float32's own error of the device tests."""
import numpy as np
import torch
import torch.nn.functional as F

PARAMS = ("enc.weight", "enc.discriminator2.lins.0.weight", "enc.discriminator2.lins.0.bias",
          "enc.discriminator2.norms.0.module.weight", "enc.discriminator2.norms.0.module.bias",
          "enc.discriminator2.lins.1.weight", "enc.discriminator2.lins.1.bias")
GRADS = tuple("grad." + k for k in PARAMS)
STATS = ("mean", "var", "mean_gen", "var_gen")
KEYS = ("p", "p_gen", "loss_dis", "loss_g") + GRADS + STATS + ("running_mean", "running_var")
MOMENTUM, EPS = 0.1, 1e-5


def make_params(f, seed):
    """Xavier-uniform encoder weight, torch.nn.Linear's uniform draws for the two linears, a batch norm away from its initial (1, 0)."""
    rng = np.random.default_rng(seed)
    a = np.sqrt(6.0 / (64 + f))
    k = 1.0 / np.sqrt(64.0)
    return [rng.uniform(-a, a, (64, f)).astype(np.float32), rng.uniform(-k, k, (64, 64)).astype(np.float32),
            rng.uniform(-k, k, 64).astype(np.float32), rng.uniform(0.5, 1.5, 64).astype(np.float32),
            rng.uniform(-0.2, 0.2, 64).astype(np.float32), rng.uniform(-k, k, (1, 64)).astype(np.float32),
            rng.uniform(-k, k, 1).astype(np.float32)]


def make_inputs(b, f, seed):
    """x_feat small positives (a 1-hop aggregate of row-normalised features), x_noise signed normals."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 0.1, (b, f)).astype(np.float32), rng.standard_normal((b, f)).astype(np.float32))


def _call(h, gamma, beta, w1, b1):
    mean, var = h.mean(0), h.var(0, unbiased=False)
    s = torch.sigmoid((h - mean) / torch.sqrt(var + EPS) * gamma + beta)
    return torch.sigmoid(s.mm(w1.t()) + b1)[:, 0], mean, h.var(0, unbiased=True)


def evaluate(x_feat, x_noise, params, dtype, running=None):
    """Every quantity of KEYS as float64 numpy.  `running` = (running_mean, running_var) before the step (default 0, 1)."""
    w, w0, b0, gamma, beta, w1, b1 = (torch.tensor(np.asarray(p), dtype=dtype).requires_grad_() for p in params)
    xf, xn = torch.tensor(np.asarray(x_feat), dtype=dtype), torch.tensor(np.asarray(x_noise), dtype=dtype)
    b = xf.shape[0]
    e = F.relu(torch.cat([xf, xn], 0).mm(w.t()))
    h = e.mm(w0.t()) + b0
    p, mean, var = _call(h, gamma, beta, w1, b1)
    p_gen, mean_gen, var_gen = _call(h[b:], gamma, beta, w1, b1)
    label = torch.cat([torch.zeros(b, dtype=dtype), torch.ones(b, dtype=dtype)])
    loss_dis = F.binary_cross_entropy(p, label)
    loss_g = F.binary_cross_entropy(p_gen, torch.zeros_like(p_gen))
    (loss_dis + loss_g).backward()
    rm = torch.zeros(64, dtype=dtype) if running is None else torch.tensor(np.asarray(running[0]), dtype=dtype)
    rv = torch.ones(64, dtype=dtype) if running is None else torch.tensor(np.asarray(running[1]), dtype=dtype)
    with torch.no_grad():
        for m, v in ((mean, var), (mean_gen, var_gen)):             # call 1, then call 2: torch's update, unbiased variance
            rm = MOMENTUM * m + (1 - MOMENTUM) * rm
            rv = MOMENTUM * v + (1 - MOMENTUM) * rv
    out = {"p": p, "p_gen": p_gen, "loss_dis": loss_dis.reshape(1), "loss_g": loss_g.reshape(1), "mean": mean, "var": var,
           "mean_gen": mean_gen, "var_gen": var_gen, "running_mean": rm, "running_var": rv}
    for k, t in zip(GRADS, (w, w0, b0, gamma, beta, w1, b1)):
        out[k] = t.grad
    return {k: v.detach().double().numpy().copy() for k, v in out.items()}
