"""HIP-graph replay of ops.bn_leaky_relu_bf16 (amk_bnact_bf16_*): forward, input-gradient-only backward and double backward
captured once at (4, 16, 31, 31), the replay bitwise equal to the eager run -- the bf16 counterpart of
tests/test_discr_norm_gpu.py::test_graph_replay_bitwise.  Workspaces come from torch and launches go on the current stream,
so nothing in the op stands in the way of a capture.  The file name sorts behind every other test file, as the other capture
test's does."""
import pytest
import torch
import torch.nn as nn

from amk import ops
from amk.models.discriminator import input_grad_only

pytestmark = pytest.mark.gpu
SLOPE = 0.2
BF16 = torch.bfloat16


def test_graph_replay_bitwise(device):
    shape = (4, 16, 31, 31)
    g = torch.Generator().manual_seed(7)
    x0 = (0.7 + 1.3 * torch.randn(shape, generator=g)).to(device=device, dtype=BF16)
    gz0 = torch.randn(shape, generator=g).to(device=device, dtype=BF16)
    ggx = torch.randn(shape, generator=g).to(device=device, dtype=BF16)
    bn = nn.BatchNorm2d(shape[1])
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(shape[1], generator=g))
        bn.bias.copy_(0.3 * torch.randn(shape[1], generator=g))
    bn = bn.to(device)
    x = x0.clone().requires_grad_()
    assert ops.bn_leaky_relu_bf16_ok(bn, x)

    def step():
        z = ops.bn_leaky_relu_bf16(x, bn, SLOPE)
        with input_grad_only():
            (gx,) = torch.autograd.grad(z, x, gz0, create_graph=True)
        loss = (z.float() * gz0.float()).sum() + (gx.float() * ggx.float()).sum()
        gxx, gw, gb = torch.autograd.grad(loss, (x, bn.weight, bn.bias))
        return [z.detach(), gx.detach(), gxx, gw, gb]

    eager = [t.clone() for t in step()]
    assert [t.dtype for t in eager] == [BF16, BF16, BF16, torch.float32, torch.float32]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, static):
        assert torch.equal(a, b)
