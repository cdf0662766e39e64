"""Write tests/golden/parti_small.npz, parti_d64.npz, transformer_small.npz and parti_generate_small.npz: Parti and the
seq2seq Transformer, computed by the REFERENCE's own models/parti.py and models/transformer.py on the CPU.

    AMK_REFERENCE=<reference checkout> python tools/gen_parti_golden.py

The reference modules are loaded by path through a namespace stub for their ``models`` package.  models/parti.py imports
``transformers`` (imported first, for real) and ``torchvision`` (not installed: an empty stub module is registered, the
file only imports it).  Its TextEncoder downloads a CLIP tower, so ``parti.TextEncoder`` is replaced in that namespace by
a stub that returns the tensor it is given; ``vq`` is a stub nn.Module with ``codebook.codebook_size``, ``num_patches``,
``encode_imgs`` returning fixed ids and ``decode_indices`` returning its input.  Every model runs in eval mode
(PositionalEncoding has dropout 0.1).  The ``pos_enc.pe`` buffer (5000 x dim) is left out of the stored weights; its first
PE_ROWS rows are stored as ``pe_rows``: the reference builds the table with f32 exp / sin / cos, whose last bits differ
between CPUs' math libraries, and 1 ulp of exp is 100 ulps of sin's argument at position 100 -- a restatement or a model
that is to be compared to these files at 1e-6 has to take the very rows they were computed with.

parti_small and transformer_small keep their gradients in a second file, <name>_grads.npz (weights and gradients of the
two-layer models together would pass 1 MiB).
parti_small / parti_d64: weights, text embeddings, ids, the loss and the gradient of every parameter that gets one.
transformer_small: weights, source / target ids, the logits, a cotangent and the gradients of (logits * cot).sum().
Those three run the reference module in fp64 on the f32 weights (``module.double()``: the weights, and the pe table the
reference builds in f32, exactly) and store the results rounded to f32, so what a test compares against carries 6e-8 of
rounding and none of an f32 run's own error.
parti_generate_small: Parti.generate as the reference runs it, with the Gumbel noise it drew (re-drawn from the same seed:
F.gumbel_softmax is the loop's only consumer of the global generator), every step's unfiltered last-row logits and the
chosen ids.  Seeds are searched until, at every step and row of the reference's own run, the winning ``logits + gumbel``
among the kept tokens leads the second by at least MIN_GAP and the 5th largest logit (the filter's boundary, k =
ceil(0.1 * 48) = 5) leads the 6th by at least MIN_GAP: a condition on the fixture that keeps f32 rounding from flipping a
token, not a tolerance.  The smallest gap is stored.
"""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.fixture_recipe import randomize_, seeded  # noqa: E402
from oracle.gen_golden import REF  # noqa: E402  (the reference checkout; AMK_REFERENCE overrides)
from tools.gen_agent_golden_dh import save  # noqa: E402

MIN_GAP = 1e-3
PE_ROWS = 160   # rows of the pe table stored with every fixture: more than any sequence here


def load_reference():
    import transformers  # noqa: F401  (before the torchvision stub: transformers probes for the real package)

    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tv.transforms = types.ModuleType("torchvision.transforms")
        sys.modules["torchvision"] = tv
        sys.modules["torchvision.transforms"] = tv.transforms
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg
    parti = importlib.import_module("models.parti")
    transformer = importlib.import_module("models.transformer")

    class TextEncoderStub(nn.Module):   # the CLIP tower's place: hands the given hidden states on
        def __init__(self, dim, enc_type, enc_name, max_length):
            super().__init__()

        def forward(self, text_hidden):
            return text_hidden

    parti.TextEncoder = TextEncoderStub
    return parti, transformer


class StubVQ(nn.Module):
    def __init__(self, codebook_size, num_patches, ids=None):
        super().__init__()
        self.codebook = types.SimpleNamespace(codebook_size=codebook_size)
        self.num_patches = num_patches
        self.ids = ids

    def encode_imgs(self, imgs):
        return self.ids

    def decode_indices(self, ids):
        return ids


def weights(module):
    return {"w:" + k: v.detach().numpy().copy() for k, v in module.state_dict().items() if not k.endswith("pos_enc.pe")}


def f32(t):
    """An fp64 result as it is stored: rounded to f32 (6e-8 relative: the files stay half the size)."""
    return t.detach().to(torch.float32).numpy().copy()


def save_split(name, arrays, split):
    """One file, or (split) the gradients in <name>_grads.npz: every committed file stays well under 1 MiB."""
    if not split:
        return save(name, arrays)
    grads = {k: v for k, v in arrays.items() if k.startswith("g:")}
    return save(name, {k: v for k, v in arrays.items() if k not in grads}) + save(name + "_grads", grads)


def seeded_ids(shape, high, seed):
    return torch.randint(0, high, shape, generator=torch.Generator().manual_seed(seed))


def gen_parti(parti, name, dim, heads, d_head, depth, V, L, T, B, seed):
    ids = seeded_ids((B, T), V, seed + 1)
    torch.manual_seed(0)
    m = parti.Parti(dim, StubVQ(V, T, ids), None, None, 77, heads, d_head, depth)
    randomize_(m, seed)
    m.eval()
    text = seeded((B, L, dim), seed + 2)
    arrays = dict(weights(m), text=text.numpy(), ids=ids.numpy(), dims=np.array([dim, heads, d_head, depth, V, L, T, B]),
                  pe_rows=m.pos_enc.pe[:PE_ROWS].numpy().copy())
    if name == "parti_small":
        arrays["pe_out"] = m.pos_enc(text).detach().numpy()   # eval mode: text + pe[:L]
    m.double()   # the f32 weights and the f32-built pe table, exactly, in fp64 arithmetic
    loss = m(text.double(), torch.zeros(B, 3, 8, 8))
    loss.backward()
    arrays["loss"] = f32(loss)
    for n, p in m.named_parameters():
        if p.grad is not None:
            arrays["g:" + n] = f32(p.grad)
    print(f"{name}.npz: {save_split(name, arrays, depth > 1)} bytes, loss {float(loss.detach()):.6f}")


def gen_transformer(transformer):
    dim, V, heads, d_head, S, T, B, seed = 64, 50, 2, 32, 5, 70, 2, 311
    torch.manual_seed(0)
    m = transformer.Transformer(dim, vocab_size=V, n_heads=heads, d_head=d_head, enc_depth=1, dec_depth=1, n_classes=V)
    randomize_(m, seed)
    m.eval()
    src, tgt = seeded_ids((B, S), V, seed + 1), seeded_ids((B, T), V, seed + 2)
    cot = seeded((B, T, V), seed + 3)
    arrays = dict(weights(m), src=src.numpy(), tgt=tgt.numpy(), cot=cot.numpy(), dims=np.array([dim, V, heads, d_head, 1, 1, V, S, T, B]),
                  pe_rows=m.pos_enc.pe[:PE_ROWS].numpy().copy())
    m.double()
    logits = m(src, tgt)
    (logits * cot.double()).sum().backward()
    arrays["logits"] = f32(logits)
    for n, p in m.named_parameters():
        if p.grad is not None:
            arrays["g:" + n] = f32(p.grad)
    print(f"transformer_small.npz: {save_split('transformer_small', arrays, True)} bytes")


def gen_generate(parti):
    dim, heads, d_head, depth, V, L, T, B = 64, 2, 32, 2, 48, 7, 12, 2
    k = math.ceil((1 - 0.9) * V)
    torch.manual_seed(0)
    m = parti.Parti(dim, StubVQ(V, T), None, None, 77, heads, d_head, depth)
    randomize_(m, 421)
    m.eval()
    text = seeded((B, L, dim), 422)
    last_rows = []
    hook = m.to_logits.register_forward_hook(lambda mod, inp, out: last_rows.append(out[:, -1, :].detach().clone()))
    for seed in range(1, 200):
        last_rows.clear()
        torch.manual_seed(seed)
        with torch.no_grad():
            ids = m.generate(text)
        torch.manual_seed(seed)
        noise = torch.stack([-torch.empty(B, V).exponential_().log() for _ in range(T)])
        logits = torch.stack(last_rows)                                   # (T, B, V)
        top = logits.topk(k + 1, dim=-1).values
        filtered = torch.full_like(logits, float("-inf")).scatter_(2, logits.topk(k, dim=-1).indices, top[..., :k])
        two = (filtered + noise).topk(2, dim=-1)
        assert torch.equal(two.indices[..., 0].t(), ids), "the re-drawn noise does not replay the reference's choice"
        gap = min(float((two.values[..., 0] - two.values[..., 1]).min()), float((top[..., k - 1] - top[..., k]).min()))
        print(f"seed {seed}: smallest gap {gap:.3e}", flush=True)
        if gap >= MIN_GAP:
            break
    else:
        raise SystemExit("no seed reaches the gap")
    hook.remove()
    assert gap >= MIN_GAP
    arrays = dict(weights(m), text=text.numpy(), gumbel=noise.numpy(), logits=logits.numpy(), ids=ids.numpy(),
                  pe_rows=m.pos_enc.pe[:PE_ROWS].numpy().copy(),
                  min_gap=np.array(gap), seed=np.array(seed), dims=np.array([dim, heads, d_head, depth, V, L, T, B]))
    print(f"parti_generate_small.npz: {save('parti_generate_small', arrays)} bytes, seed {seed}, smallest gap {gap:.3e}")


def main():
    parti, transformer = load_reference()
    torch.set_num_threads(1)   # a fixed reduction order for the reference's CPU kernels
    gen_parti(parti, "parti_small", 64, 2, 32, 2, 48, 7, 80, 2, 401)
    gen_parti(parti, "parti_d64", 64, 1, 64, 1, 48, 7, 130, 2, 411)
    gen_transformer(transformer)
    gen_generate(parti)


if __name__ == "__main__":
    main()
