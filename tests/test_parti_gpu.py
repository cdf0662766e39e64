"""Parti and the seq2seq Transformer on the GPU against the fixtures of the reference's own modules
(tools/gen_parti_golden.py): loss / logits and every parameter gradient, the token-by-token generate loop replayed with the
reference's noise, and Transformer.generate's bounded loop."""
import types

import pytest
import torch

from test_parti_golden import fixture
from util import assert_close, weights_of

pytestmark = pytest.mark.gpu

# the model-level tolerances of test_attention_head_dims_gpu.py::test_vit_dim_head_96
TOL_OUT = 5e-5
TOL_GRAD = 2e-4


class StubVQ(torch.nn.Module):
    """The frozen tokenizer's place: fixed ids for encode_imgs, ids handed back by decode_indices."""

    def __init__(self, codebook_size, num_patches, ids=None):
        super().__init__()
        self.codebook = types.SimpleNamespace(codebook_size=codebook_size)
        self.num_patches = num_patches
        self.ids = ids

    def encode_imgs(self, imgs):
        return self.ids.to(imgs.device)

    def decode_indices(self, ids):
        return ids


def _load(module, fx, device):
    missing, unexpected = module.load_state_dict(weights_of(fx), strict=False)
    assert missing == ["pos_enc.pe"] and not unexpected, (missing, unexpected)   # the buffer the fixtures leave out
    rows = torch.from_numpy(fx["pe_rows"])
    with torch.no_grad():   # the rows the reference ran with: the table's last bits depend on the CPU's math library
        assert float((module.pos_enc.pe[: rows.shape[0]] - rows).abs().max()) <= (rows.shape[0] - 1) * 2.0 ** -21 + 2.0 ** -22
        module.pos_enc.pe[: rows.shape[0]] = rows
    return module.to(device).eval()   # eval: PositionalEncoding has dropout 0.1


def _check_grads(module, fx):
    params = dict(module.named_parameters())
    names = sorted(k[2:] for k in fx if k.startswith("g:"))
    assert set(names) == {n for n in params if not n.startswith("vq.")}
    for n in names:
        g, ref = params[n].grad, torch.from_numpy(fx["g:" + n])
        assert g is not None, n
        err = float((g.detach().cpu().double() - ref.double()).abs().max())
        bound = TOL_GRAD * float(ref.abs().max())
        print(f"grad {n}: abs err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, f"grad {n}: abs err {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name", ["parti_small", "parti_d64"])
def test_parti_training_step_vs_reference(device, name):
    from amk import ops
    from amk.models import Parti

    fx = fixture(name)
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    m = _load(Parti(dim, StubVQ(V, T, torch.from_numpy(fx["ids"])), None, None, 77, h, d, depth), fx, device)
    text = torch.from_numpy(fx["text"]).to(device)
    ops.KERNEL_EVENTS = {}
    try:
        loss = m(text, torch.zeros(B, 3, 8, 8, device=device))
        loss.backward()
        torch.cuda.synchronize()
        names = set(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    print(f"{name}: loss {float(loss.detach()):.7f} (reference {float(fx['loss'].item()):.7f}); kernels {sorted(names)}")
    assert_close(loss.detach(), fx["loss"], TOL_OUT, "loss")
    _check_grads(m, fx)
    # the causal self-attention and the cross-attention ran on the library's attention kernels, both ways
    assert any(n.startswith("attn_fwd") for n in names) and any(n.startswith("attn_bwd") for n in names), names
    assert all(p.grad is None for p in m.vq.parameters())


def test_transformer_vs_reference(device):
    from amk.models import Transformer

    fx = fixture("transformer_small")
    dim, V, h, d, enc_depth, dec_depth, n_classes, S, T, B = (int(v) for v in fx["dims"])
    m = _load(Transformer(dim, V, h, d, enc_depth, dec_depth, n_classes), fx, device)
    src, tgt = torch.from_numpy(fx["src"]).to(device), torch.from_numpy(fx["tgt"]).to(device)
    context_mask, causal_mask = m.get_decoder_mask(src, tgt)
    assert context_mask.device == src.device and causal_mask.device == tgt.device   # (the reference builds them on the CPU)
    logits = m(src, tgt)
    assert_close(logits, fx["logits"], TOL_OUT, "logits")
    (logits * torch.from_numpy(fx["cot"]).to(device)).sum().backward()
    _check_grads(m, fx)


def test_parti_generate_replays_the_reference(device):
    from amk.models import Parti

    fx = fixture("parti_generate_small")
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    m = _load(Parti(dim, StubVQ(V, T), None, None, 77, h, d, depth), fx, device)
    trace = []
    ids = m.generate(torch.from_numpy(fx["text"]).to(device), gumbel=torch.from_numpy(fx["gumbel"]).to(device), trace=trace)
    assert tuple(ids.shape) == (B, T) and len(trace) == T
    ids_ref = torch.from_numpy(fx["ids"])
    for step in range(T):
        assert torch.equal(ids[:, step].cpu(), ids_ref[:, step]), step
        assert_close(trace[step], fx["logits"][step], TOL_OUT, f"step {step} logits")
    # without explicit noise the sampler draws its own: ids of the same shape inside the codebook
    own = m.generate(torch.from_numpy(fx["text"]).to(device))
    assert tuple(own.shape) == (B, T) and int(own.min()) >= 0 and int(own.max()) < V


def test_transformer_generate_is_bounded_by_max_len(device):
    from amk.models import Transformer

    fx = fixture("transformer_small")
    dim, V, h, d, enc_depth, dec_depth, n_classes, S, T, B = (int(v) for v in fx["dims"])
    m = _load(Transformer(dim, V, h, d, enc_depth, dec_depth, n_classes), fx, device)
    out = m.generate(torch.from_numpy(fx["src"]).to(device), max_len=4)
    assert out.device == torch.device(device) and out.dtype == torch.long
    assert out.shape[0] == B and 1 <= out.shape[1] <= 5 and bool((out[:, 0] == 1).all())
