"""``Parti.sample(graph=True)`` under bf16 autocast: the captured step on a bf16 decode state computes what the eager loop
computes, bit for bit, and a second call in a FRESH autocast context replays the same capture -- it reads state-owned and
parameter memory only, never autocast's weight-cast cache, which is gone by then.  Named to sort behind every other test
file, as tests/test_zz_parti_decode_graph_gpu.py is."""
import pytest
import torch

from test_parti_decode_gpu import SAMPLE_STEPS, _sampler

pytestmark = pytest.mark.gpu


def test_graphed_sample_under_autocast_equals_eager_bitwise(device):
    m, text, gumbel, _, _, (B, V) = _sampler(device)
    eager_trace, graph_trace = [], []
    with torch.autocast("cuda", dtype=torch.bfloat16):
        eager = m.sample(text, gumbel=gumbel, trace=eager_trace)
        graphed = m.sample(text, gumbel=gumbel, trace=graph_trace, graph=True)
    assert m.decode_graph_captures == 1
    assert tuple(graphed.shape) == (B, SAMPLE_STEPS) and torch.equal(graphed, eager)
    assert len(graph_trace) == len(eager_trace) == SAMPLE_STEPS
    for step in range(SAMPLE_STEPS):
        assert graph_trace[step].dtype == torch.float32
        assert torch.equal(graph_trace[step], eager_trace[step]), step
    # a second call in a fresh autocast context, another context tensor and other noise: its own eager run, no new capture
    g = torch.Generator().manual_seed(77)
    text2 = text + 0.5 * torch.randn(text.shape, generator=g).to(device)
    gumbel2 = gumbel.flip(0).contiguous()
    eager_trace2, graph_trace2 = [], []
    with torch.autocast("cuda", dtype=torch.bfloat16):
        eager2 = m.sample(text2, gumbel=gumbel2, trace=eager_trace2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        graphed2 = m.sample(text2, gumbel=gumbel2, trace=graph_trace2, graph=True)
    assert m.decode_graph_captures == 1
    assert torch.equal(graphed2, eager2)
    for step in range(SAMPLE_STEPS):
        assert torch.equal(graph_trace2[step], eager_trace2[step]), step
    assert not torch.equal(eager2, eager)
    # outside autocast the same module decodes in f32 on a capture of its own: the key holds the state's dtype
    f32 = m.sample(text2, gumbel=gumbel2, graph=True)
    assert m.decode_graph_captures == 2 and torch.equal(f32, m.sample(text2, gumbel=gumbel2))
    m.drop_decode_graph()
