"""``Parti.sample(graph=True)``: the captured step replayed for every position computes what the eager loop computes,
bit for bit; the state and the static inputs are refreshed between calls; noise drawn inside the graph is fresh on every
replay.  Kept in a file of its own whose name sorts behind every other test file, so that a plain ``pytest tests`` runs the
captures last (DESIGN.md section 4i on captures)."""
import copy

import pytest
import torch

from test_parti_decode_gpu import SAMPLE_STEPS, _sampler

pytestmark = pytest.mark.gpu


def test_graphed_sample_equals_eager_bitwise(device):
    m, text, gumbel, ids_ref, _, (B, V) = _sampler(device)
    eager_trace, graph_trace = [], []
    eager = m.sample(text, gumbel=gumbel, trace=eager_trace)
    graphed = m.sample(text, gumbel=gumbel, trace=graph_trace, graph=True)
    assert torch.equal(graphed, eager) and torch.equal(eager.cpu(), ids_ref)
    assert len(graph_trace) == SAMPLE_STEPS
    for step in range(SAMPLE_STEPS):
        assert torch.equal(graph_trace[step], eager_trace[step]), step
    # a second call on the same module, other text and other noise: the captured graph is reused, the state reset and
    # the static inputs refreshed
    g = torch.Generator().manual_seed(77)
    text2 = text + 0.5 * torch.randn(text.shape, generator=g).to(device)
    gumbel2 = gumbel.flip(0).contiguous()
    captures = m.decode_graph_captures
    eager2, graphed2 = m.sample(text2, gumbel=gumbel2), m.sample(text2, gumbel=gumbel2, graph=True)
    assert m.decode_graph_captures == captures == 1
    assert torch.equal(graphed2, eager2)
    assert not torch.equal(eager2, eager)   # the second text and noise do lead elsewhere
    # a parameter that moved is captured anew, never replayed on its old address; dropping the graph frees it
    m.to_logits.bias.data = m.to_logits.bias.data.clone()
    assert torch.equal(m.sample(text2, gumbel=gumbel2, graph=True), eager2) and m.decode_graph_captures == 2
    copy.deepcopy(m)          # the captured graph is no attribute of the module
    m.drop_decode_graph()


def test_graphed_sample_draws_fresh_noise(device):
    m, text, _, _, _, (B, V) = _sampler(device)
    a = m.sample(text, graph=True)
    b = m.sample(text, graph=True)
    for ids in (a, b):
        assert tuple(ids.shape) == (B, SAMPLE_STEPS) and int(ids.min()) >= 0 and int(ids.max()) < V
    # 24 steps x 2 rows over 48 codes: equal ids mean the replays reuse one draw
    assert not torch.equal(a, b)
    assert len({tuple(a[:, s].tolist()) for s in range(1, SAMPLE_STEPS)}) > 1   # nor is one step's draw frozen
