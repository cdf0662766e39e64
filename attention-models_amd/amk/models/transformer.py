"""Pre-LN encoder / decoder stacks around SoftmaxAttention (scaffolding of SURVEY.md section 8
a15; reference: models/transformer.py:11-135), and the seq2seq ``Transformer`` on top of them (reference :138-228).
Plain PyTorch except for the attention cores, the LayerNorms and the Linear layers.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .attention import SoftmaxAttention
from .layers import Linear
from .positional_encoding import PositionalEncoding


class LayerNorm(nn.Module):
    """Learnable gain, fixed zero shift kept as a BUFFER named ``beta`` (it is in the state_dict
    but never trained), as the reference has it."""

    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))
        self.register_buffer("beta", torch.zeros(dim))

    def forward(self, x, residual=None):
        """LN(x), or with ``residual``: (x + residual, LN(x + residual)) from one kernel."""
        if residual is None:
            if x.is_cuda:
                return ops.layer_norm(x, self.gamma, self.beta)   # amk_add_layernorm_fwd / _bwd
            return F.layer_norm(x, x.shape[-1:], self.gamma, self.beta)
        if x.is_cuda:
            return ops.add_layer_norm(x, residual, self.gamma, self.beta)
        h = x + residual
        return h, F.layer_norm(h, h.shape[-1:], self.gamma, self.beta)


class GEGLU(nn.Module):
    def forward(self, x):
        if x.is_cuda and x.shape[-1] % 8 == 0 and x.numel() > 0:
            return ops.geglu(x)                     # amk_geglu_fwd / _bwd: one pass each
        val, gate = x.chunk(2, dim=-1)
        return gate * F.gelu(val)


class FeedForward(nn.Module):
    """Linear(dim, 2*inner, no bias) -> GEGLU -> LayerNorm(inner) -> Linear(inner, dim, no bias),
    inner = int(dim * mult * 2 / 3)."""

    def __init__(self, dim, mult=4):
        super().__init__()
        inner = int(dim * mult * 2 / 3)
        self.ff = nn.Sequential(nn.Linear(dim, inner * 2, bias=False), GEGLU(), LayerNorm(inner),
                                nn.Linear(inner, dim, bias=False))

    def forward(self, x):
        lin1, _, norm, lin2 = self.ff
        if ops.geglu_ffn_ok(x, lin1.weight, norm.gamma, norm.beta, lin2.weight):
            # bf16 autocast: gate + LayerNorm as one kernel each way, f32 weight gradients (ops._GEGLUFFNMixed)
            return ops.geglu_ffn(x, lin1.weight, norm.gamma, norm.beta, lin2.weight)
        return self.ff(x)


class EncoderLayer(nn.Module):
    def __init__(self, dim, n_heads=8, d_head=64, mult=4, dropout=0.0):
        super().__init__()
        self.self_attn = SoftmaxAttention(dim, n_heads, d_head, dropout)
        self.feed_forward = FeedForward(dim, mult=mult)
        self.norm1 = LayerNorm(dim)
        self.norm2 = LayerNorm(dim)

    def forward(self, x, context_mask=None):
        # x + attn(LN(x)), then x + ffn(LN(x)): the first add happens inside the second LayerNorm kernel
        x, y = self.norm2(x, self.self_attn(x=self.norm1(x), context_mask=context_mask))
        return self.feed_forward(y) + x


class Encoder(nn.Module):
    def __init__(self, dim, n_heads=8, d_head=64, depth=6, mult=4, dropout=0.0):
        super().__init__()
        self.layers = nn.ModuleList(EncoderLayer(dim, n_heads, d_head, mult, dropout) for _ in range(depth))

    def forward(self, x, context_mask=None):
        for layer in self.layers:
            x = layer(x, context_mask=context_mask)
        return x


class DecoderLayer(nn.Module):
    """self-attention (causal mask) -> cross-attention over ``context`` (key-padding mask) -> FFN."""

    def __init__(self, dim, n_heads=8, d_head=64, mult=4, dropout=0.0):
        super().__init__()
        self.self_attn = SoftmaxAttention(dim, n_heads, d_head, dropout)
        self.cross_attn = SoftmaxAttention(dim, n_heads, d_head, dropout)
        self.feed_forward = FeedForward(dim, mult)
        self.norm1 = LayerNorm(dim)
        self.norm2 = LayerNorm(dim)
        self.norm3 = LayerNorm(dim)

    def forward(self, dec_inp, context, context_mask=None, causal_mask=None):
        # the adds after self- and cross-attention happen inside the LayerNorm kernels that follow them
        x, y = self.norm2(dec_inp, self.self_attn(x=self.norm1(dec_inp), causal_mask=causal_mask))
        x, y = self.norm3(x, self.cross_attn(x=y, context=context, context_mask=context_mask))
        return self.feed_forward(y) + x


class Decoder(nn.Module):
    def __init__(self, dim, n_heads=8, d_head=64, depth=6, mult=4, dropout=0.0):
        super().__init__()
        self.layers = nn.ModuleList(DecoderLayer(dim, n_heads, d_head, mult, dropout) for _ in range(depth))

    def forward(self, dec_in, context, context_mask=None, causal_mask=None):
        out = dec_in
        for layer in self.layers:
            out = layer(out, context, context_mask=context_mask, causal_mask=causal_mask)
        return out


class Transformer(nn.Module):
    """Encoder-decoder over token ids (reference: models/transformer.py:138-228): embeddings + sinusoidal positions,
    the encoder over the source, the decoder over the target with the causal mask and an all-true context mask, a Linear
    onto ``n_classes``.  The masks are built on the input's device (the reference builds them on the CPU and therefore
    only runs there)."""

    def __init__(self, dim, vocab_size=1000, n_heads=8, d_head=64, enc_depth=6, dec_depth=6, n_classes=None):
        super().__init__()
        self.enc_input_proj = nn.Embedding(vocab_size, dim)
        self.dec_input_proj = nn.Embedding(vocab_size, dim)
        self.pos_enc = PositionalEncoding(dim)
        self.enc_init_norm = LayerNorm(dim)
        self.encoder = Encoder(dim=dim, n_heads=n_heads, d_head=d_head, depth=enc_depth)
        self.enc_final_norm = LayerNorm(dim)

        self.dec_init_norm = LayerNorm(dim)
        self.decoder = Decoder(dim=dim, n_heads=n_heads, d_head=d_head, depth=dec_depth)
        self.dec_final_norm = LayerNorm(dim)
        self.linear = Linear(dim, n_classes)

    def get_decoder_mask(self, src_seq, tgt_seq):
        """(context mask (B, S), all true: no PAD handling in the reference either; causal mask (T, T), True = masked)."""
        t = tgt_seq.shape[1]
        context_mask = torch.ones(src_seq.shape, dtype=torch.bool, device=src_seq.device)
        return context_mask, ops.causal_mask(t, t, tgt_seq.device)

    def forward(self, src_seq, tgt_seq):
        context_mask, causal_mask = self.get_decoder_mask(src_seq, tgt_seq)
        src = self.enc_init_norm(self.pos_enc(self.enc_input_proj(src_seq)))
        context = self.enc_final_norm(self.encoder(src, context_mask=context_mask))
        dec_in = self.dec_init_norm(self.pos_enc(self.dec_input_proj(tgt_seq)))
        dec_out = self.decoder(dec_in=dec_in, context=context, context_mask=context_mask, causal_mask=causal_mask)
        return self.linear(self.dec_final_norm(dec_out))

    @torch.no_grad()
    def generate(self, src_seq, max_len=None):
        """Sampling as the reference writes it (:176-202): no norms, no masks, the whole prefix through the decoder at
        every step, Gumbel-softmax sampling, stop when the FIRST sequence draws the end token 2.  max_len (an addition):
        at most that many tokens are appended; None = the reference's unbounded loop."""
        context = self.encoder(self.pos_enc(self.enc_input_proj(src_seq)))
        end_token = 2
        out_seq = torch.ones((src_seq.shape[0], 1), dtype=torch.long, device=src_seq.device)
        while max_len is None or out_seq.shape[1] - 1 < max_len:
            dec_out = self.decoder(dec_in=self.pos_enc(self.dec_input_proj(out_seq)), context=context)
            logits = self.linear(dec_out)
            last_token = F.gumbel_softmax(logits[:, -1, :], tau=1, hard=False).argmax(dim=-1)
            if last_token[0] == end_token:
                break
            out_seq = torch.cat((out_seq, last_token.unsqueeze(1)), dim=1)
        return out_seq
