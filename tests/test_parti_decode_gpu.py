"""KV-cached causal decoding of Parti and the seq2seq Transformer on the GPU: teacher-forced ``next_logits`` against the
fp64 restatement (tests/parti_ref.py) and the reference's own fixtures, and ``sample`` against an fp64 oracle that reruns
the whole causal forward on the growing prefix."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import parti_ref
from test_parti_golden import _w64, fixture
from test_parti_gpu import TOL_OUT, StubVQ, _load
from util import assert_close

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-3        # tools/gen_parti_golden.py's condition on a sampling fixture
SAMPLE_STEPS = 24
SAMPLE_SEED = 0       # chosen on the CPU so that both margins of _oracle_sample hold (asserted there, never skipped)


@pytest.mark.parametrize("name", ["parti_small", "parti_d64"])
def test_parti_next_logits_teacher_forced(device, name):
    from amk import ops
    from amk.models import Parti

    fx = fixture(name)
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    m = _load(Parti(dim, StubVQ(V, T), None, None, 77, h, d, depth), fx, device)
    ids = torch.from_numpy(fx["ids"])
    ref = parti_ref.parti_logits(torch.from_numpy(fx["text"]).double(), ids, _w64(fx, grad=False), h, d, depth)   # (B, T, V)
    ids_dev = ids.to(device)
    ops.KERNEL_EVENTS = {}
    try:
        state = m.begin_decode(torch.from_numpy(fx["text"]).to(device))
        rows = [m.next_logits(state, ids_dev[:, t - 1] if t else None) for t in range(T)]
        torch.cuda.synchronize()
        names = set(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    logits = torch.stack(rows, dim=1).cpu()
    for t in range(T):
        assert_close(logits[:, t], ref[:, t], TOL_OUT, f"{name} step {t} logits")
    loss = F.cross_entropy(logits.transpose(1, 2), ids)
    print(f"{name}: teacher-forced loss {float(loss):.7f} (reference {float(fx['loss'].item()):.7f}); kernels {sorted(names)}")
    assert_close(loss, fx["loss"], TOL_OUT, "loss")
    assert "attn_decode" in names and not any(n.startswith("attn_fwd") for n in names), names
    assert state.host_pos == T and int(state.pos.item()) == T
    with pytest.raises(RuntimeError, match="full"):
        m.next_logits(state, ids_dev[:, -1])


def test_transformer_next_logits_teacher_forced(device):
    from amk.models import Transformer

    fx = fixture("transformer_small")
    dim, V, h, d, enc_depth, dec_depth, n_classes, S, T, B = (int(v) for v in fx["dims"])
    m = _load(Transformer(dim, V, h, d, enc_depth, dec_depth, n_classes), fx, device)
    tgt = torch.from_numpy(fx["tgt"]).to(device)
    state = m.begin_decode(torch.from_numpy(fx["src"]).to(device), capacity=T)
    for t in range(T):
        assert_close(m.next_logits(state, tgt[:, t]), fx["logits"][:, t], TOL_OUT, f"step {t} logits")


@functools.lru_cache(maxsize=None)
def _oracle_sample():
    """(text, gumbel (steps, B, V), ids (B, steps), logits (steps, B, V)) of the fp64 oracle: parti_logits rerun on the
    growing prefix, generate's filter and argmax.  Asserts the two margins tools/gen_parti_golden.py searches for, at every
    step and row: winner against runner-up of filtered logits + noise, and the k-th against the (k + 1)-th logit."""
    fx = fixture("parti_small")
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    w = _w64(fx, grad=False)
    text = torch.from_numpy(fx["text"]).double()
    g = torch.Generator().manual_seed(SAMPLE_SEED)
    gumbel = -torch.empty(SAMPLE_STEPS, B, V).exponential_(generator=g).log()
    k = math.ceil((1 - 0.9) * V)
    ids = torch.zeros(B, 0, dtype=torch.long)
    rows, gap = [], float("inf")
    for step in range(SAMPLE_STEPS):
        padded = torch.cat((ids, torch.zeros(B, 1, dtype=torch.long)), dim=1)   # the last column is never read
        last = parti_ref.parti_logits(text, padded, w, h, d, depth)[:, -1, :]
        top = last.topk(k + 1, dim=-1).values
        filtered = torch.full_like(last, float("-inf")).scatter_(1, last.topk(k, dim=-1).indices, top[:, :k])
        two = (filtered + gumbel[step].double()).topk(2, dim=-1)
        gap = min(gap, float((two.values[:, 0] - two.values[:, 1]).min()), float((top[:, k - 1] - top[:, k]).min()))
        rows.append(last)
        ids = torch.cat((ids, two.indices[:, :1]), dim=1)
    print(f"sampling oracle: seed {SAMPLE_SEED}, smallest gap {gap:.3e}")
    assert gap >= MIN_GAP, f"seed {SAMPLE_SEED}: smallest gap {gap:.3e} < {MIN_GAP}: choose another seed"
    return fx, gumbel, ids, torch.stack(rows)


def _sampler(device):
    from amk.models import Parti

    fx, gumbel, ids, logits = _oracle_sample()
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    m = _load(Parti(dim, StubVQ(V, SAMPLE_STEPS), None, None, 77, h, d, depth), fx, device)
    return m, torch.from_numpy(fx["text"]).to(device), gumbel.to(device), ids, logits, (B, V)


def test_parti_sample_follows_the_oracle(device):
    m, text, gumbel, ids_ref, logits_ref, (B, V) = _sampler(device)
    trace = []
    ids = m.sample(text, gumbel=gumbel, trace=trace)
    assert tuple(ids.shape) == (B, SAMPLE_STEPS) and len(trace) == SAMPLE_STEPS
    for step in range(SAMPLE_STEPS):
        assert torch.equal(ids[:, step].cpu(), ids_ref[:, step]), step
        assert_close(trace[step], logits_ref[step], TOL_OUT, f"step {step} logits")
    own = m.sample(text)   # its own noise: ids of the same shape inside the codebook
    assert tuple(own.shape) == (B, SAMPLE_STEPS) and own.dtype == torch.long
    assert int(own.min()) >= 0 and int(own.max()) < V


def test_transformer_sample_is_bounded_by_max_len(device):
    from amk.models import Transformer

    fx = fixture("transformer_small")
    dim, V, h, d, enc_depth, dec_depth, n_classes, S, T, B = (int(v) for v in fx["dims"])
    m = _load(Transformer(dim, V, h, d, enc_depth, dec_depth, n_classes), fx, device)
    out = m.sample(torch.from_numpy(fx["src"]).to(device), max_len=4)
    assert out.device == torch.device(device) and out.dtype == torch.long
    assert out.shape[0] == B and 1 <= out.shape[1] <= 5 and bool((out[:, 0] == 1).all())
