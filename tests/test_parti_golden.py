"""Parti, Transformer and PositionalEncoding on the CPU: the project's restatement (tests/parti_ref.py, run in fp64)
against the fixtures the reference's own modules wrote (tools/gen_parti_golden.py); the drop-in classes' state_dict keys
and shapes against the same fixtures; the alias package's exports; ops.causal_mask."""
import os

import numpy as np
import pytest
import torch

import parti_ref
from util import GOLDEN, load_golden, weights_of

RTOL = 1e-6   # relative to the largest element of each tensor (the fixtures store fp64 results rounded to f32: 6e-8)


def fixture(name):
    """<name>.npz, with <name>_grads.npz merged in where the gradients live in a file of their own."""
    fx = load_golden(name)
    if os.path.exists(os.path.join(GOLDEN, name + "_grads.npz")):
        fx.update(load_golden(name + "_grads"))
    return fx


def _close(a, b, what):
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    print(f"{what}: rel err {err:.3e}")
    assert err <= RTOL, f"{what}: rel err {err:.3e} > {RTOL:.0e}"


def _w64(fx, grad=True):
    """The fixture's weights in fp64 and, as "pos_enc.pe", the rows of the pe table it was computed with."""
    w = {k: v.double().requires_grad_(grad) for k, v in weights_of(fx).items() if v.dtype.is_floating_point}
    w["pos_enc.pe"] = torch.from_numpy(fx["pe_rows"]).double()
    return w


@pytest.mark.parametrize("name", ["parti_small", "parti_d64"])
def test_restatement_matches_the_parti_fixture(name):
    fx = fixture(name)
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    w = _w64(fx)
    text, ids = torch.from_numpy(fx["text"]).double(), torch.from_numpy(fx["ids"])
    assert ids.shape == (B, T) and text.shape == (B, L, dim)
    loss = parti_ref.parti_loss(text, ids, w, h, d, depth)
    _close(loss.detach(), fx["loss"], "loss")
    names = sorted(k[2:] for k in fx if k.startswith("g:"))
    assert set(w) - set(names) == {k for k in w if k.endswith(".beta")} | {"pos_enc.pe"}   # every parameter gets one
    grads = torch.autograd.grad(loss, [w[n] for n in names])
    for n, g in zip(names, grads):
        _close(g, fx["g:" + n], f"grad {n}")


def test_restatement_matches_the_transformer_fixture():
    fx = fixture("transformer_small")
    dim, V, h, d, enc_depth, dec_depth, n_classes, S, T, B = (int(v) for v in fx["dims"])
    w = _w64(fx)
    src, tgt = torch.from_numpy(fx["src"]), torch.from_numpy(fx["tgt"])
    logits = parti_ref.transformer_logits(src, tgt, w, h, d, enc_depth, dec_depth)
    assert logits.shape == (B, T, n_classes)
    _close(logits.detach(), fx["logits"], "logits")
    names = sorted(k[2:] for k in fx if k.startswith("g:"))
    grads = torch.autograd.grad((logits * torch.from_numpy(fx["cot"]).double()).sum(), [w[n] for n in names])
    for n, g in zip(names, grads):
        _close(g, fx["g:" + n], f"grad {n}")
    # a parameter without a stored gradient got none in the reference: the norms' beta buffers are not parameters
    assert set(w) - set(names) == {k for k in w if k.endswith(".beta")} | {"pos_enc.pe"}


def test_restatement_replays_the_generate_fixture():
    fx = fixture("parti_generate_small")
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    assert float(fx["min_gap"].item()) >= 1e-3   # the fixture's own condition (tools/gen_parti_golden.py)
    w = _w64(fx, grad=False)
    text = torch.from_numpy(fx["text"]).double()
    gumbel, ids_ref = torch.from_numpy(fx["gumbel"]).double(), torch.from_numpy(fx["ids"])
    assert gumbel.shape == (T, B, V) and ids_ref.shape == (B, T)
    ids = torch.zeros(B, 0, dtype=torch.long)
    for step in range(T):
        last, token = parti_ref.parti_generate_step(text, ids, w, h, d, depth, gumbel[step])
        _close(last, fx["logits"][step], f"step {step} logits")
        assert torch.equal(token, ids_ref[:, step]), step
        ids = torch.cat((ids, token.unsqueeze(1)), dim=1)


class _StubVQ(torch.nn.Module):
    def __init__(self, codebook_size, num_patches):
        super().__init__()
        import types
        self.codebook = types.SimpleNamespace(codebook_size=codebook_size)
        self.num_patches = num_patches


def _same_keys_and_shapes(module, fx, dim):
    sd = module.state_dict()
    want = {k: tuple(v.shape) for k, v in weights_of(fx).items()}
    want["pos_enc.pe"] = (5000, dim)   # the buffer the fixtures leave out
    assert {k: tuple(v.shape) for k, v in sd.items()} == want


@pytest.mark.parametrize("name", ["parti_small", "parti_d64", "parti_generate_small"])
def test_parti_has_the_reference_state_dict(name):
    from amk.models import Parti

    fx = fixture(name)
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    m = Parti(dim, _StubVQ(V, T), None, None, 77, h, d, depth)   # the reference's positional argument order
    _same_keys_and_shapes(m, fx, dim)
    assert not any(k.startswith("text_encoder") for k in m.state_dict())
    with pytest.raises(TypeError, match="CLIP"):
        m(["a photo"], torch.zeros(B, 3, 8, 8))
    with pytest.raises(TypeError, match="CLIP"):
        m.generate(["a photo"])


def test_transformer_has_the_reference_state_dict():
    from amk.models import Transformer

    fx = fixture("transformer_small")
    dim, V, h, d, enc_depth, dec_depth, n_classes, S, T, B = (int(v) for v in fx["dims"])
    m = Transformer(dim, V, h, d, enc_depth, dec_depth, n_classes)
    _same_keys_and_shapes(m, fx, dim)


def test_alias_package_exports_the_fourteen_names():
    import models
    from models import Parti, PositionalEncoding, Transformer  # noqa: F401

    reference_exports = ["SoftmaxAttention", "AgentAttention", "SwitchHeadAttention", "MoELayer", "Codebook", "ViTVQGAN",
                         "VQGAN", "ViT", "ViTMoE", "MUSE", "MaskGitTransformer", "Parti", "Transformer", "build_model"]
    for n in reference_exports:
        assert hasattr(models, n) and n in models.__all__, n
    from amk.models.positional_encoding import AbsolutePositionalEmbedding
    assert models.AbsolutePositionalEmbedding is AbsolutePositionalEmbedding


def test_positional_encoding_equals_the_reference_values():
    from amk.models import AbsolutePositionalEmbedding, PositionalEncoding

    fx = fixture("parti_small")
    pe_rows, text = torch.from_numpy(fx["pe_rows"]), torch.from_numpy(fx["text"])
    m = PositionalEncoding(text.shape[-1]).eval()
    assert tuple(m.pe.shape) == (5000, text.shape[-1]) and list(m.state_dict()) == ["pe"]
    assert m.dropout.p == 0.1
    # The table is built with f32 exp, sin and cos, whose last bits differ between CPUs' math libraries.  Row p is
    # sin / cos of p * div_term with div_term = exp(..) <= 1: an exp and a product that are each off by up to 2 ulps
    # (2^-23 relative) move the argument by up to p * 2^-21, and sin / cos (slope <= 1) add 2 ulps of their own.
    n = pe_rows.shape[0]
    bound = (n - 1) * 2.0 ** -21 + 2.0 ** -22
    for what, table in (("pe", m.pe[:n]), ("restated pe", parti_ref.positional_table(n, text.shape[-1]))):
        err = float((table.double() - pe_rows.double()).abs().max())
        print(f"{what}: abs err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, err, bound)
    with torch.no_grad():
        m.pe[:n] = pe_rows   # then the forward is an add: exact
    assert torch.equal(m(text), torch.from_numpy(fx["pe_out"]))
    a = AbsolutePositionalEmbedding(16, 32)
    out = a(torch.arange(10).unsqueeze(0))
    assert tuple(out.shape) == (1, 10, 16) and list(a.state_dict()) == ["emb.weight"]
    assert torch.allclose(out.norm(dim=-1), torch.ones(1, 10), atol=1e-6)


@pytest.mark.parametrize("I,J", [(1, 1), (65, 65), (200, 333)])
def test_causal_mask_is_the_reference_mask(I, J):
    from amk import ops

    m = ops.causal_mask(I, J, "cpu")
    assert m.dtype == torch.bool and torch.equal(m, torch.ones((I, J), dtype=torch.bool).triu(J - I + 1))
    assert ops.causal_mask(I, J, "cpu") is m   # cached per (I, J, device)
    assert torch.equal(m, parti_ref.causal_mask(I, J))
