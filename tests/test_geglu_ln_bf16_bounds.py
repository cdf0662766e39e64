"""The per-element bounds of tests/geglu_ln_bf16_ref.py, checked without a GPU: the CPU emulation of
csrc/geglu_ln_bf16.hip stays under half of every bound, planted defects fall outside, and ops.geglu_ffn on CPU tensors is
the plain PyTorch chain."""
import pytest
import torch
import torch.nn.functional as F

import geglu_ln_bf16_ref as ref

SHAPES = [(5, 8), (7, 264), (33, 4096)]
CAP = 0.5

_CACHE = {}


def _case(family, M, H):
    key = (family, M, H)
    if key not in _CACHE:
        inp = ref.make_inputs(family, M, H)
        _CACHE[key] = (inp, ref.reference(*inp))
    return _CACHE[key]


@pytest.mark.parametrize("M,H", SHAPES)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_emulation_stays_under_half_of_every_bound(family, M, H):
    inp, R = _case(family, M, H)
    q = ref.ratios(ref.emulate(*inp), R, record=False)
    print(family, M, H, {k: round(v, 4) for k, v in q.items()})
    for name in ref.TENSORS:
        assert torch.isfinite(R["bound_" + name]).all(), name
        assert q[name] <= CAP, (name, q[name])


def test_flat_rows_give_beta_exactly_in_the_emulation():
    (ab, dy, gamma, beta), _ = _case("flat_rows", 7, 264)
    got = ref.emulate(ab, dy, gamma, beta)
    rows = ref.zero_rows("flat_rows", 7)
    assert rows
    for r in rows:
        assert torch.equal(got["y"][r], beta.to(torch.bfloat16))


@pytest.mark.parametrize("mut,family,tensors", [
    ("swapped_halves", "diffuse", ("y", "d_ab")),
    ("tanh_bf16_twice", "diffuse", ("y",)),
    ("uncentred_variance", "large", ("y", "rstd")),
    ("gamma_after_means", "diffuse", ("d_ab",)),
    ("dgamma_drops_last_row", "diffuse", ("dgamma",)),
])
def test_planted_defects_fall_outside_the_bound(mut, family, tensors):
    inp, R = _case(family, 33, 264)
    q = ref.ratios(ref.emulate(*inp, mut=mut), R, record=False)
    clean = ref.ratios(ref.emulate(*inp), R, record=False)
    print(mut, {k: round(v, 3) for k, v in q.items()})
    for name in tensors:
        assert clean[name] <= CAP
        assert q[name] > 1.0, (mut, name, q[name])


def test_num_partials_keeps_the_partial_traffic_small():
    assert ref.num_partials(8192, 4096) == 512
    assert ref.num_partials(1, 8) == 1 and ref.num_partials(5, 8) == 2 and ref.num_partials(5, 4096) == 5
    # (parts, 2, H) f32 written and read again, against ab + dy read and d_ab written in bf16
    assert 2 * 512 * 2 * 4096 * 4 <= 0.11 * (8192 * 4096 * 2 * 5)


def _chain(x, w1, gamma, beta, w2, eps=1e-5):
    val, gate = F.linear(x, w1).chunk(2, dim=-1)
    return F.linear(F.layer_norm(gate * F.gelu(val), (w2.shape[1],), gamma, beta, eps), w2)


def test_geglu_ffn_on_cpu_tensors_is_the_plain_chain():
    from amk import ops

    torch.manual_seed(0)
    dim, inner = 24, 40
    x = torch.randn(3, 5, dim, requires_grad=True)
    w1 = (torch.randn(2 * inner, dim) / dim ** 0.5).requires_grad_(True)
    w2 = (torch.randn(dim, inner) / inner ** 0.5).requires_grad_(True)
    gamma = (0.5 + torch.rand(inner)).requires_grad_(True)
    beta = torch.randn(inner)
    dout = torch.randn(3, 5, dim)
    want = _chain(x, w1, gamma, beta, w2)
    gw = torch.autograd.grad(want, (x, w1, gamma, w2), dout)
    got = ops.geglu_ffn(x, w1, gamma, beta, w2)
    gg = torch.autograd.grad(got, (x, w1, gamma, w2), dout)
    assert not ops.geglu_ffn_ok(x, w1, gamma, beta, w2)
    assert got.dtype == torch.float32 and (got - want).abs().max() <= 1e-6
    for a, b in zip(gg, gw):
        assert (a - b).abs().max() <= 1e-6


def test_feed_forward_on_cpu_is_unchanged():
    from amk.models import transformer

    torch.manual_seed(0)
    ff = transformer.FeedForward(24, mult=3)
    assert list(ff.state_dict()) == ["ff.0.weight", "ff.2.gamma", "ff.2.beta", "ff.3.weight"]
    x = torch.randn(2, 7, 24)
    assert torch.equal(ff(x), ff.ff(x))
    assert torch.equal(ff(x), _chain(x, ff.ff[0].weight, ff.ff[2].gamma, ff.ff[2].beta, ff.ff[3].weight))
