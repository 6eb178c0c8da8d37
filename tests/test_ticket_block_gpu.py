"""`fullgraph.ticket_block` under `fullgraph_script.capture`: the block that `FullGraphAdj.__init__` allocated is the one the captured
launches hold (no allocation, no fill node inside the capture), replays equal the eager epoch bit for bit, and the block is zero
afterwards.  The epoch: one `GcnLayerFn` (k_prelu_bwd_one in its backward) and one AEGIS batch-norm head (k_bn_stats,
k_bn_bwd_sums) forward and backward, on N = 600 nodes at H = 64."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, F, H = 600, 32, 64


def test_captured_epoch_holds_the_block_built_with_the_graph():
    from ggad_amd import fullgraph as FG
    from ggad_amd.fullgraph_script import capture
    from ggad_amd.model_aegis import ACT_RELU, BnActFn
    rng = np.random.default_rng(0)
    r, c = rng.integers(0, N, 4 * N), rng.integers(0, N, 4 * N)
    a = (sp.eye(N, format="csr") + sp.csr_matrix((rng.random(4 * N), (r, c)), shape=(N, N))).tocsr()
    fa = FG.FullGraphAdj(a, a, DEV)
    assert DEV in FG._TICKET_BLOCKS                                    # built with the graph, before any epoch
    block = FG.ticket_block(DEV)
    ptrs = [block.data_ptr()]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, F, generator=g).to(DEV)
    gy = torch.randn(N, H, generator=g).to(DEV)
    w = (torch.randn(H, F, generator=g) * 0.2).to(DEV).requires_grad_(True)
    b = (torch.randn(H, generator=g) * 0.1).to(DEV).requires_grad_(True)
    slope = torch.tensor([0.25], device=DEV, requires_grad=True)
    bn = torch.nn.BatchNorm1d(H).to(DEV)
    params = [w, b, slope, bn.weight, bn.bias]

    def epoch_fn():
        hid = FG.GcnLayerFn.apply(x, w, b, slope, fa)
        y = BnActFn.apply(hid, bn.weight, bn.bias, bn, ACT_RELU)
        grads = torch.autograd.grad(y, params, gy)
        ptrs.append(FG.ticket_block(DEV).data_ptr())
        return [y.detach()] + [t.detach() for t in grads]

    eager = [t.clone() for t in epoch_fn()]
    torch.cuda.synchronize()
    assert not block.any()
    graph, static = capture(epoch_fn)
    ptrs.append(FG.ticket_block(DEV).data_ptr())
    assert len(ptrs) == 4 and len(set(ptrs)) == 1                      # before, in the eager epoch, inside the capture, after it
    for _ in range(3):
        for t in static:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for s, e in zip(static, eager):
            assert s.dtype == e.dtype and torch.equal(s.view(torch.int32), e.view(torch.int32))
    assert not block.any()
    assert int(bn.num_batches_tracked) == 4                            # the eager epoch and three replays (the capture runs nothing)
