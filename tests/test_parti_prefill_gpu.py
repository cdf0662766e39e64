"""Prompted KV-cached decoding of Parti and the seq2seq Transformer on the GPU: ``prefill`` -- the given tokens through the
decoder in one pass on the many-row kernel of csrc/attn_prefill.hip -- against the fp64 restatement (tests/parti_ref.py)
and the reference's own fixtures, the teacher-forced steps that follow it, a prefill in two parts, the kernels it runs,
its refusals, and ``sample(prefix_ids=...)`` against the fp64 sampling oracle of tests/test_parti_decode_gpu.py."""
import functools

import pytest
import torch

import parti_ref
from test_parti_decode_gpu import SAMPLE_STEPS, _sampler
from test_parti_golden import _w64, fixture
from test_parti_gpu import TOL_OUT, StubVQ, _load
from util import assert_close

pytestmark = pytest.mark.gpu

PARTI = ["parti_small", "parti_d64"]


def _prefix_lengths(T):
    return [1, 33, 64, 65, T - 1]


@functools.lru_cache(maxsize=None)
def _parti_ref(name):
    """fp64 logits (B, T, V) of the fixture's ids: computed once, shared, never written."""
    fx = fixture(name)
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    return parti_ref.parti_logits(torch.from_numpy(fx["text"]).double(), torch.from_numpy(fx["ids"]), _w64(fx, grad=False), h, d, depth)


def _parti(name, device):
    from amk.models import Parti

    fx = fixture(name)
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    m = _load(Parti(dim, StubVQ(V, T), None, None, 77, h, d, depth), fx, device)
    return m, torch.from_numpy(fx["text"]).to(device), torch.from_numpy(fx["ids"]).to(device), _parti_ref(name), T


def _transformer(device):
    from amk.models import Transformer

    fx = fixture("transformer_small")
    dim, V, h, d, enc_depth, dec_depth, n_classes, S, T, B = (int(v) for v in fx["dims"])
    m = _load(Transformer(dim, V, h, d, enc_depth, dec_depth, n_classes), fx, device)
    return m, torch.from_numpy(fx["src"]).to(device), torch.from_numpy(fx["tgt"]).to(device), torch.from_numpy(fx["logits"]), T


@pytest.mark.parametrize("name", PARTI)
def test_parti_prefill_then_teacher_forced_steps(device, name):
    from amk import ops

    m, text, ids, ref, T = _parti(name, device)
    for n in _prefix_lengths(T):
        state = m.begin_decode(text)
        ops.KERNEL_EVENTS = {}
        try:
            logits = m.prefill(state, ids[:, :n], all_logits=True)      # the start token and n tokens: rows 0 .. n
            torch.cuda.synchronize()
            names = set(ops.KERNEL_EVENTS)
        finally:
            ops.KERNEL_EVENTS = None
        assert tuple(logits.shape) == (ref.shape[0], n + 1, ref.shape[2]) and logits.dtype == torch.float32
        assert "attn_prefill" in names and not any(k.startswith(("attn_fwd", "attn_decode")) for k in names), names
        assert state.host_pos == n + 1 and int(state.pos.item()) == n + 1
        for t in range(n + 1):
            assert_close(logits[:, t], ref[:, t], TOL_OUT, f"{name} n {n}: prefill row {t}")
        for t in range(n + 1, T):                                       # the steps after the prompt read what it cached
            assert_close(m.next_logits(state, ids[:, t - 1]), ref[:, t], TOL_OUT, f"{name} n {n}: step {t}")
        last = m.prefill(m.begin_decode(text), ids[:, :n])              # the last row alone: the same row
        assert_close(last, ref[:, n], TOL_OUT, f"{name} n {n}: last row alone")


def test_transformer_prefill_then_teacher_forced_steps(device):
    from amk import ops

    m, src, tgt, ref, T = _transformer(device)
    for n in _prefix_lengths(T):
        state = m.begin_decode(src, capacity=T)
        ops.KERNEL_EVENTS = {}
        try:
            logits = m.prefill(state, tgt[:, :n], all_logits=True)      # rows 0 .. n - 1
            torch.cuda.synchronize()
            names = set(ops.KERNEL_EVENTS)
        finally:
            ops.KERNEL_EVENTS = None
        assert "attn_prefill" in names and not any(k.startswith(("attn_fwd", "attn_decode")) for k in names), names
        assert tuple(logits.shape) == (ref.shape[0], n, ref.shape[2]) and state.host_pos == n == int(state.pos.item())
        for t in range(n):
            assert_close(logits[:, t], ref[:, t], TOL_OUT, f"n {n}: prefill row {t}")
        for t in range(n, T):
            assert_close(m.next_logits(state, tgt[:, t]), ref[:, t], TOL_OUT, f"n {n}: step {t}")


@pytest.mark.parametrize("name", PARTI)
def test_parti_prefill_in_two_parts(device, name):
    m, text, ids, ref, T = _parti(name, device)
    a, b = 23, 42                                                       # the second part starts inside a row block
    whole = m.prefill(m.begin_decode(text), ids[:, :a + b], all_logits=True)
    state = m.begin_decode(text)
    first = m.prefill(state, ids[:, :a], all_logits=True)               # rows 0 .. a
    second = m.prefill(state, ids[:, a:a + b], all_logits=True)         # position a + 1: rows a + 1 .. a + b
    assert state.host_pos == a + b + 1 and int(state.pos.item()) == a + b + 1
    parts = torch.cat((first, second), dim=1)
    assert_close(parts, whole, TOL_OUT, "prefill(a) then prefill(b) against prefill(a + b)")
    for t in range(a + b + 1):
        assert_close(parts[:, t], ref[:, t], TOL_OUT, f"{name}: row {t}")


def test_transformer_prefill_in_two_parts(device):
    m, src, tgt, ref, T = _transformer(device)
    a, b = 23, 42
    whole = m.prefill(m.begin_decode(src, capacity=T), tgt[:, :a + b], all_logits=True)
    state = m.begin_decode(src, capacity=T)
    parts = torch.cat((m.prefill(state, tgt[:, :a], all_logits=True), m.prefill(state, tgt[:, a:a + b], all_logits=True)), dim=1)
    assert_close(parts, whole, TOL_OUT, "prefill(a) then prefill(b) against prefill(a + b)")
    assert_close(parts, ref[:, :a + b], TOL_OUT, "against the fixture")


def test_position_and_capacity_refusals(device):
    m, text, ids, ref, T = _parti("parti_small", device)
    state = m.begin_decode(text)
    with pytest.raises(RuntimeError, match="no room"):
        m.prefill(state, ids)                                           # T tokens behind the start token: T + 1 rows
    assert state.host_pos == 0 and int(state.pos.item()) == 0
    m.prefill(state, ids[:, :T - 1])                                    # exactly full
    assert state.host_pos == T
    with pytest.raises(RuntimeError, match="no room"):
        m.prefill(state, ids[:, :1])
    with pytest.raises(RuntimeError, match="full"):
        m.next_logits(state, ids[:, 0])
    with pytest.raises(ValueError, match="only position 0"):
        m.next_logits(state, None)
    with pytest.raises(ValueError, match="prefill takes tokens"):
        m.prefill(m.begin_decode(text), ids[:1, :4])                    # another batch
    with pytest.raises(ValueError, match="at least one token"):
        state.set_position(3)
        m.prefill(state, ids[:, :0])
    dec = m.transformer_decoder
    state = m.begin_decode(text)
    with pytest.raises(ValueError, match="prefill takes n >= 1 rows"):
        dec.prefill(torch.zeros(ids.shape[0], 4, device=device), state)
    with pytest.raises(RuntimeError, match="no room"):
        dec.prefill(torch.zeros(ids.shape[0], T + 1, m.dim, device=device), state)
    with torch.autocast("cuda", dtype=torch.bfloat16):                  # an f32 state does not run under autocast
        with pytest.raises(RuntimeError, match="outside autocast"):
            m.prefill(state, ids[:, :4])
    with pytest.raises(ValueError, match="prefix_ids must be"):
        m.sample(text, prefix_ids=ids)                                  # nothing left to sample
    tm, src, tgt, tref, TT = _transformer(device)
    state = tm.begin_decode(src, capacity=8)
    with pytest.raises(RuntimeError, match="no room"):
        tm.prefill(state, tgt[:, :9])
    with pytest.raises(ValueError, match="prefix must be"):
        tm.sample(src, max_len=8, prefix=tgt[:, :8])
    with pytest.raises(ValueError, match="prefix must be"):
        tm.sample(src, max_len=8, prefix=tgt[0, :3])                    # one-dimensional
    with pytest.raises(ValueError, match="prefix_ids must be"):
        m.sample(text, prefix_ids=ids[0, :3])


@pytest.mark.parametrize("k", [1, 7, 23])
def test_parti_sample_with_a_prefix_follows_the_oracle(device, k):
    m, text, gumbel, ids_ref, logits_ref, (B, V) = _sampler(device)
    trace = []
    ids = m.sample(text, prefix_ids=ids_ref[:, :k].to(device), gumbel=gumbel, trace=trace)
    assert tuple(ids.shape) == (B, SAMPLE_STEPS) and len(trace) == SAMPLE_STEPS
    assert torch.equal(ids.cpu(), ids_ref)                              # the given tokens kept, the rest the oracle's
    for step in range(SAMPLE_STEPS):                                    # gumbel and trace by absolute step
        assert_close(trace[step], logits_ref[step], TOL_OUT, f"k {k}: step {step} logits")


def test_parti_sample_with_a_prefix_replays_the_captured_step(device):
    m, text, gumbel, ids_ref, logits_ref, (B, V) = _sampler(device)
    try:
        for k in (7, 23, 1):                                            # one capture serves every prefix length
            trace = []
            ids = m.sample(text, prefix_ids=ids_ref[:, :k].to(device), gumbel=gumbel, trace=trace, graph=True)
            assert torch.equal(ids.cpu(), ids_ref), k
            assert len(trace) == SAMPLE_STEPS
            for step in range(SAMPLE_STEPS):
                assert_close(trace[step], logits_ref[step], TOL_OUT, f"graph k {k}: step {step} logits")
        assert m.decode_graph_captures == 1
        assert torch.equal(m.sample(text, gumbel=gumbel, graph=True).cpu(), ids_ref)   # and the sample without a prefix
        assert m.decode_graph_captures == 1
    finally:
        m.drop_decode_graph()


def test_transformer_sample_with_a_prefix(device):
    m, src, tgt, ref, T = _transformer(device)
    g = torch.Generator().manual_seed(5)
    gumbel = -torch.empty(12, ref.shape[0], ref.shape[2]).exponential_(generator=g).log().to(device)
    full = m.sample(src, max_len=12, gumbel=gumbel)
    assert full.shape[1] >= 2, "the first sequence drew the end token at once: choose another seed"
    for k in range(1, min(full.shape[1], 12)):                                 # its own tokens as the prefix: the same sample
        again = m.sample(src, max_len=12, gumbel=gumbel, prefix=full[:, 1:1 + k])
        assert torch.equal(again, full), k
