"""KV-cached decoding of Parti and the seq2seq Transformer under bf16 autocast on the GPU: a bf16 decode state (bf16
caches, the state's own bf16 weight copies, amk_attn_decode_bf16 and amk_gemm_rows_bf16) against the fp64 logits and
against the causal forward under the same autocast, ``sample`` against torch's sampler on its own traced logits, the
AMK_DECODE_BF16 switch, a state used outside autocast, and weight copies that follow the parameters.

Deviation from the fp64 logits, decode / causal forward under autocast (max and rms over all logits; the caps asserted are
1.5 and 1.25).  The test prints the ratios it measures; DESIGN.md section 4i records them."""
import functools
import math

import pytest
import torch

import parti_ref
from test_parti_golden import _w64, fixture
from test_parti_gpu import StubVQ, _load

pytestmark = pytest.mark.gpu

NAMES = ["parti_small", "parti_d64", "transformer_small"]
MAX_CAP, RMS_CAP = 1.5, 1.25
BF16 = torch.bfloat16


def _autocast():
    return torch.autocast("cuda", dtype=BF16)


class _Case:
    """One fixture: the model on the device, its teacher-forced inputs, the fp64 logits (B, T, V)."""

    def __init__(self, name, device):
        from amk.models import Parti, Transformer

        fx = fixture(name)
        self.name, self.parti = name, name.startswith("parti")
        if self.parti:
            dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
            self.m = _load(Parti(dim, StubVQ(V, T), None, None, 77, h, d, depth), fx, device)
            self.ctx = torch.from_numpy(fx["text"]).to(device)
            self.ids = torch.from_numpy(fx["ids"]).to(device)
            self.ref = _parti_ref(name)
        else:
            dim, V0, h, d, enc_depth, dec_depth, V, S, T, B = (int(v) for v in fx["dims"])
            self.m = _load(Transformer(dim, V0, h, d, enc_depth, dec_depth, V), fx, device)
            self.ctx = torch.from_numpy(fx["src"]).to(device)
            self.ids = torch.from_numpy(fx["tgt"]).to(device)
            self.ref = torch.from_numpy(fx["logits"]).double()
        self.T, self.B, self.V = T, B, V

    def begin(self, out=None):
        if self.parti:
            return self.m.begin_decode(self.ctx, out=out)
        return self.m.begin_decode(self.ctx, capacity=self.T, out=out)

    def prev(self, t, ids=None):
        """The token fed at position t."""
        ids = self.ids if ids is None else ids
        if self.parti:
            return ids[:, t - 1] if t else None
        return ids[:, t]

    def teacher_forced(self, state):
        return torch.stack([self.m.next_logits(state, self.prev(t)) for t in range(self.T)], dim=1)

    def forward_logits(self):
        """The causal forward's logits (B, T, V) as the caller's autocast context runs them: the parent's own path."""
        from amk import ops

        m = self.m
        if not self.parti:
            return m(self.ctx, self.ids)
        text = m.context_norm(self.ctx)
        x = m.pos_enc(m.token_emb(self.ids[:, :-1]))
        x = m.init_norm(torch.cat((m.start_token.expand(self.B, 1, -1), x), dim=1))
        out = m.transformer_decoder(dec_in=x, context=text, causal_mask=ops.causal_mask(self.T, self.T, x.device))
        return m.to_logits(m.final_norm(out))


@functools.lru_cache(maxsize=None)
def _parti_ref(name):
    fx = fixture(name)
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    return parti_ref.parti_logits(torch.from_numpy(fx["text"]).double(), torch.from_numpy(fx["ids"]), _w64(fx, grad=False), h, d, depth)


def _dev(got, ref):
    e = got.detach().double().cpu() - ref
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


@pytest.mark.parametrize("name", NAMES)
def test_next_logits_teacher_forced_under_autocast(device, name):
    from amk import ops

    c = _Case(name, device)
    with _autocast():
        state = c.begin()                        # (the Transformer's encoder runs here, on the attention forward)
        ops.KERNEL_EVENTS = {}
        try:
            logits = c.teacher_forced(state)
            torch.cuda.synchronize()
            names = set(ops.KERNEL_EVENTS)
        finally:
            ops.KERNEL_EVENTS = None
    with _autocast():
        fwd = c.forward_logits()
    assert state.dtype == BF16 and all(t.dtype == BF16 for t in state.self_kv + state.cross_kv)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (c.B, c.T, c.V)
    assert bool(torch.isfinite(logits).all())
    dmax, drms = _dev(logits, c.ref)
    fmax, frms = _dev(fwd.float(), c.ref)
    print(f"{name}: decode max {dmax:.3e} rms {drms:.3e}; causal forward under autocast max {fmax:.3e} rms {frms:.3e}; "
          f"ratio max {dmax / fmax:.3f} rms {drms / frms:.3f}; kernels {sorted(names)}")
    assert dmax <= MAX_CAP * fmax, (dmax, fmax)
    assert drms <= RMS_CAP * frms, (drms, frms)
    assert "attn_decode" in names and not any(n.startswith("attn_fwd") for n in names), names
    assert any(n.startswith("gemm_rows_bf16") for n in names), names
    assert state.host_pos == c.T and int(state.pos.item()) == c.T


@pytest.mark.parametrize("name", NAMES)
def test_a_state_built_under_autocast_serves_outside_it(device, name):
    c = _Case(name, device)
    with _autocast():
        inside = c.teacher_forced(c.begin())
        state = c.begin()
    outside = c.teacher_forced(state)            # no autocast here: the bf16 state carries everything the step reads
    assert outside.dtype == torch.float32
    assert torch.equal(inside, outside)


@pytest.mark.parametrize("name", NAMES)
def test_switch_off_refuses_under_autocast(device, name, monkeypatch):
    from amk import ops

    c = _Case(name, device)
    monkeypatch.setattr(ops, "DECODE_BF16", False)
    with _autocast():
        with pytest.raises(RuntimeError, match="a bf16 cache is not implemented"):
            state = c.begin()
            assert state.dtype == torch.float32
            c.m.next_logits(state, c.prev(0))
    state = c.begin()                            # outside autocast the f32 decode runs as ever
    assert state.dtype == torch.float32 and c.m.next_logits(state, c.prev(0)).dtype == torch.float32


@pytest.mark.parametrize("name", NAMES)
def test_weight_copies_follow_the_parameters(device, name):
    c = _Case(name, device)
    m = c.m
    head = m.to_logits if c.parti else m.linear
    layer = (m.transformer_decoder if c.parti else m.decoder).layers[0]
    with _autocast():
        state = c.begin()
        before = c.m.next_logits(state, c.prev(0)).clone()
        ptrs = [w.data_ptr() for d in state.weights + [state.head] for w in d.values()]
        with torch.no_grad():
            head.weight.mul_(0.5)
            layer.feed_forward.ff[3].weight.mul_(-1.0)
            layer.self_attn.kv[0].weight.add_(0.25)
        assert c.begin(out=state) is state
        after = c.m.next_logits(state, c.prev(0))
    assert ptrs == [w.data_ptr() for d in state.weights + [state.head] for w in d.values()]
    bits = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    assert torch.equal(bits(state.head["head"]), bits(head.weight.detach().to(BF16)))
    assert torch.equal(bits(state.weights[0]["ff2"]), bits(layer.feed_forward.ff[3].weight.detach().to(BF16)))
    hd = layer.self_attn.q[0].weight.shape[0]
    assert torch.equal(bits(state.weights[0]["qkv"][hd:]), bits(layer.self_attn.kv[0].weight.detach().to(BF16)))
    assert torch.equal(bits(state.weights[0]["qkv"][:hd]), bits(layer.self_attn.q[0].weight.detach().to(BF16)))
    assert not torch.equal(before, after)
    with _autocast():                            # and equal to a state built fresh from the changed parameters
        fresh = c.m.next_logits(c.begin(), c.prev(0))
    assert torch.equal(after, fresh)


@pytest.mark.parametrize("name", ["parti_small", "parti_d64"])
def test_parti_sample_under_autocast(device, name):
    c = _Case(name, device)
    m, steps = c.m, c.T
    g = torch.Generator().manual_seed(11)
    gumbel = -torch.empty(steps, c.B, c.V).exponential_(generator=g).log().to(device)
    trace = []
    with _autocast():
        ids = m.sample(c.ctx, gumbel=gumbel, trace=trace)
    assert tuple(ids.shape) == (c.B, steps) and len(trace) == steps
    k = math.ceil((1 - 0.9) * c.V)
    for step in range(steps):
        lg = trace[step]
        assert lg.dtype == torch.float32
        top = lg.topk(k + 1, dim=-1)
        assert bool((top.values[:, k - 1] > top.values[:, k]).all()), f"step {step}: a tie at the k-th logit"
        filtered = torch.full_like(lg, float("-inf")).scatter_(1, top.indices[:, :k], top.values[:, :k])
        assert torch.equal(ids[:, step], (filtered + gumbel[step]).argmax(dim=-1)), step
    with _autocast():                            # the sampled ids fed back reproduce the traced logits, bit for bit
        state = c.begin()
        for step in range(steps):
            assert torch.equal(m.next_logits(state, c.prev(step, ids)), trace[step]), step
        own = m.sample(c.ctx)                    # its own noise
    assert tuple(own.shape) == (c.B, steps) and int(own.min()) >= 0 and int(own.max()) < c.V


def test_transformer_sample_under_autocast(device):
    c = _Case("transformer_small", device)
    m = c.m
    g = torch.Generator().manual_seed(5)
    gumbel = -torch.empty(c.T, c.B, c.V).exponential_(generator=g).log().to(device)
    with _autocast():
        out = m.sample(c.ctx, max_len=c.T, gumbel=gumbel)
        assert out.dtype == torch.long and out.shape[0] == c.B and 1 <= out.shape[1] <= c.T + 1
        assert bool((out[:, 0] == 1).all())
        state = m.begin_decode(c.ctx, capacity=c.T)
        n = out.shape[1]
        for t in range(min(n, c.T)):             # every token is the argmax of next_logits + noise; the loop ends on 2
            token = (m.next_logits(state, out[:, t]) + gumbel[t]).argmax(dim=-1)
            if t + 1 < n:
                assert torch.equal(token, out[:, t + 1]), t
            else:
                assert int(token[0]) == 2, t
