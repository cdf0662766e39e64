"""CPU restatement of Parti and the seq2seq Transformer (reference: models/parti.py:84-155, models/transformer.py:138-228)
on plain weight dicts, in whatever dtype the weights have (the tests run it in fp64): the two training forwards and one
step of Parti.generate.  Attention, the GEGLU feed-forward and the gamma / beta LayerNorm are oracle/ref_cpu.py's."""
import math

import torch
import torch.nn.functional as F

from oracle import ref_cpu
from oracle.ref_cpu import _gamma_ln, _geglu_ffn, _ln, _sub, softmax_attention


def positional_table(n, dim, dtype=torch.float32):
    """The first n rows of PositionalEncoding's buffer (models/positional_encoding.py:27-32), built in f32 as the
    reference builds it.  Its last bits depend on the CPU's math library (see tools/gen_parti_golden.py)."""
    position = torch.arange(n).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, dim, 2) * (-math.log(10000.0) / dim))
    pe = torch.zeros(n, dim)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.to(dtype)


def _pe(w, n, dim, dtype):
    """The table's first n rows: those in `w` ("pos_enc.pe", any number of rows: a fixture's own) or freshly built."""
    if "pos_enc.pe" in w:
        assert w["pos_enc.pe"].shape[0] >= n
        return w["pos_enc.pe"][:n].to(dtype)
    return positional_table(n, dim, dtype)


def causal_mask(i, j):
    return torch.ones(i, j, dtype=torch.bool).triu(j - i + 1)


def encoder(x, w, prefix, depth, h, d, context_mask=None):
    """transformer.Encoder (models/transformer.py:49-84)."""
    for i in range(depth):
        lw = _sub(w, f"{prefix}.layers.{i}")
        x = softmax_attention(_gamma_ln(x, lw, "norm1"), _sub(lw, "self_attn"), h, d, context_mask=context_mask) + x
        x = _geglu_ffn(_gamma_ln(x, lw, "norm2"), _sub(lw, "feed_forward")) + x
    return x


def decoder(x, context, w, prefix, depth, h, d, context_mask=None, causal=None):
    """transformer.Decoder (models/transformer.py:87-135)."""
    for i in range(depth):
        lw = _sub(w, f"{prefix}.layers.{i}")
        x = softmax_attention(_gamma_ln(x, lw, "norm1"), _sub(lw, "self_attn"), h, d, causal_mask=causal) + x
        x = softmax_attention(_gamma_ln(x, lw, "norm2"), _sub(lw, "cross_attn"), h, d, context=context,
                              context_mask=context_mask) + x
        x = _geglu_ffn(_gamma_ln(x, lw, "norm3"), _sub(lw, "feed_forward")) + x
    return x


def parti_logits(text, ids, w, h, d, depth):
    """Parti.forward up to the logits (models/parti.py:93-120), eval mode."""
    dtype = text.dtype
    ctx = _ln(text, w, "context_norm")
    b, t = ids.shape
    x = w["token_emb.weight"][ids[:, :-1]] + _pe(w, t - 1, text.shape[-1], dtype)
    x = torch.cat((w["start_token"].expand(b, 1, -1), x), dim=1)
    x = _ln(x, w, "init_norm")
    x = decoder(x, ctx, w, "transformer_decoder", depth, h, d, causal=causal_mask(t, t))
    x = _ln(x, w, "final_norm")
    return x @ w["to_logits.weight"].t() + w["to_logits.bias"]


def parti_loss(text, ids, w, h, d, depth):
    return F.cross_entropy(parti_logits(text, ids, w, h, d, depth).transpose(1, 2), ids)


def parti_generate_step(text, ids, w, h, d, depth, gumbel):
    """One step of Parti.generate (models/parti.py:135-152): the prefix `ids` (B, n) behind the start token through the
    decoder -- no causal mask, no norms, text embeddings as given -- then the top-(1 - 0.9) filter and the argmax of
    logits + gumbel on the last row.  Returns (unfiltered last-row logits (B, V), chosen ids (B,))."""
    b, n = ids.shape
    x = w["token_emb.weight"][ids] + _pe(w, n, text.shape[-1], text.dtype)
    x = torch.cat((w["start_token"].expand(b, 1, -1), x), dim=1)
    x = decoder(x, text, w, "transformer_decoder", depth, h, d)
    last = (x @ w["to_logits.weight"].t() + w["to_logits.bias"])[:, -1, :]
    k = math.ceil((1 - 0.9) * last.shape[-1])
    val, ind = last.topk(k, dim=-1)
    filtered = torch.full_like(last, float("-inf")).scatter_(1, ind, val)
    return last, (filtered + gumbel).argmax(dim=-1)


def transformer_logits(src, tgt, w, h, d, enc_depth, dec_depth):
    """Transformer.forward (models/transformer.py:204-228), eval mode; the context mask is all true."""
    dim = w["enc_input_proj.weight"].shape[1]
    dtype = w["enc_input_proj.weight"].dtype
    context_mask = torch.ones(src.shape, dtype=torch.bool)
    x = w["enc_input_proj.weight"][src] + _pe(w, src.shape[1], dim, dtype)
    x = _gamma_ln(x, w, "enc_init_norm")
    ctx = _gamma_ln(encoder(x, w, "encoder", enc_depth, h, d, context_mask=context_mask), w, "enc_final_norm")
    t = tgt.shape[1]
    y = w["dec_input_proj.weight"][tgt] + _pe(w, t, dim, dtype)
    y = _gamma_ln(y, w, "dec_init_norm")
    y = decoder(y, ctx, w, "decoder", dec_depth, h, d, context_mask=context_mask, causal=causal_mask(t, t))
    y = _gamma_ln(y, w, "dec_final_norm")
    return y @ w["linear.weight"].t() + w["linear.bias"]
