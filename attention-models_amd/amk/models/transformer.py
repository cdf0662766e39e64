"""Pre-LN encoder / decoder stacks around SoftmaxAttention (scaffolding of SURVEY.md section 8
a15; reference: models/transformer.py:11-135), and the seq2seq ``Transformer`` on top of them (reference :138-228).
Plain PyTorch except for the attention cores, the LayerNorms and the Linear layers.

``Decoder.init_state`` / ``Decoder.step`` are the causal forward one row at a time against cached keys and values
(models/decoding.py, the single-token kernel of csrc/attn_decode.hip); ``Transformer.begin_decode`` / ``next_logits`` /
``sample`` build the trained model's sampling loop on them.  ``Transformer.generate`` stays the reference's loop.
``Decoder.prefill`` / ``Transformer.prefill`` put n given rows through in one pass (csrc/attn_prefill.hip) and fill the caches.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .attention import SoftmaxAttention
from .decoding import DecoderState
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

    # ---- KV-cached decoding: the causal forward, one row per step (models/decoding.py, csrc/attn_decode.hip)
    @staticmethod
    def decode_dtype(device, dtype=None):
        """The dtype of a new decode state: ``dtype`` if given, else bf16 where bf16 autocast is enabled for the device
        and AMK_DECODE_BF16 is on, else f32."""
        if dtype is not None:
            if dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"a decode state is float32 or bfloat16, not {dtype}")
            return dtype
        device = torch.device(device)
        if (ops.DECODE_BF16 and device.type == "cuda" and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.bfloat16):
            return torch.bfloat16
        return torch.float32

    def _decode_weights(self, head):
        """[(name, [parameters stacked by rows])] per layer, then the head's: every Linear weight a bf16 step reads."""
        per_layer = []
        for layer in self.layers:
            sa, ca, ff = layer.self_attn, layer.cross_attn, layer.feed_forward.ff
            per_layer.append({"qkv": [sa.q[0].weight, sa.kv[0].weight], "wo": [sa.W_o.weight], "cq": [ca.q[0].weight],
                              "ckv": [ca.kv[0].weight], "cwo": [ca.W_o.weight], "ff1": [ff[0].weight], "ff2": [ff[3].weight]})
        return per_layer, ({"head": [head.weight]} if head is not None else None)

    @staticmethod
    def _fill_weights(dst, src):
        for name, params in src.items():
            r = 0
            for p in params:
                ops.fill_w16(dst[name][r:r + p.shape[0]], p)
                r += p.shape[0]

    @torch.no_grad()
    def init_state(self, context, capacity, context_mask=None, out=None, dtype=None, head=None):
        """The state of a decode of up to ``capacity`` rows over ``context`` (B, L, dim): empty self-attention caches
        and every layer's cross-attention K|V, projected here once.  out: a state of the same shapes to refill in place
        (its buffers keep their addresses: a captured step stays valid).

        dtype: None = bf16 where bf16 autocast is enabled for the device and AMK_DECODE_BF16 is on, else f32.  A bf16
        state holds bf16 caches and cross K|V and ITS OWN bf16 copies of every Linear weight the step reads (self-attention
        q and kv as one (3*h*d, dim) matrix; ``head``: the Linear onto the logits, read by ``logits``), filled from the
        optimizer's current bf16 shadow or the f32 master; ``out=`` refills them in place."""
        if capacity < 1:
            raise ValueError(f"capacity must be positive (got {capacity})")
        if out is not None and dtype is not None and dtype != out.dtype:
            raise ValueError("init_state(out=...): the state was made for another dtype")
        dtype = out.dtype if out is not None else self.decode_dtype(context.device, dtype)
        mask = ops._mask_u8(context_mask, (context.shape[0], context.shape[1]), "context_mask")
        weights = head_w = None
        if dtype == torch.bfloat16:
            if torch.is_autocast_enabled() and not ops.DECODE_BF16:
                raise RuntimeError(ops.DECODE_AUTOCAST_REFUSAL)
            if not context.is_cuda:
                raise RuntimeError("amk ops run only on MI355X (HIP) tensors; got a CPU tensor. There is no CPU fallback.")
            src_layers, src_head = self._decode_weights(head)
            if out is not None:
                weights, head_w = out.weights, out.head
                if (head_w is None) != (src_head is None):
                    raise ValueError("init_state(out=...): the state was made with / without a head")
            else:
                alloc = lambda src: {k: ops.empty_w16(sum(p.shape[0] for p in ps), ps[0].shape[1], context.device)  # noqa: E731
                                     for k, ps in src.items()}
                weights = [alloc(src) for src in src_layers]
                head_w = alloc(src_head) if src_head is not None else None
            for dst, src in zip(weights, src_layers):
                self._fill_weights(dst, src)
            if src_head is not None:
                self._fill_weights(head_w, src_head)
            with torch.autocast("cuda", enabled=False):
                c16 = context.to(torch.bfloat16)
                cross = [F.linear(c16, w["ckv"]) for w in weights]   # (B, L, 2*h*d) bf16, once per decode
        else:
            cross = [layer.cross_attn.project_context(context) for layer in self.layers]
        if out is not None:
            if (out.capacity != capacity or out.cross_kv[0].shape != cross[0].shape or len(out.cross_kv) != len(cross)
                    or (out.context_mask is None) != (mask is None)):
                raise ValueError("init_state(out=...): the state was made for other shapes")
            for dst, src in zip(out.cross_kv, cross):
                dst.copy_(src)
            if mask is not None:
                out.context_mask.copy_(mask)
            out.reset()
            return out
        b, width = context.shape[0], cross[0].shape[2]
        self_kv = [torch.empty((b, capacity, width), device=context.device, dtype=dtype) for _ in self.layers]
        ws = None
        if context.is_cuda:   # one workspace for every decode call of a step: the calls are ordered on the stream
            attn = self.layers[0].self_attn
            need = max(ops.attention_decode_ws_floats(b, attn.num_heads, attn.dim_head, n) for n in (capacity, context.shape[1]))
            ws = torch.empty((need,), device=context.device, dtype=torch.float32)
        return DecoderState(self_kv, [c.contiguous() for c in cross], mask, capacity, ws, weights=weights, head=head_w)

    @torch.no_grad()
    def step(self, x, state):
        """``forward`` with the causal mask for ONE new row x (B, 1, dim) at the state's position: the row's keys and
        values join the caches, the earlier rows are read from them.  The position itself is advanced by the caller
        (``state.advance()``) once the row is through.  On a bf16 state the step runs with autocast disabled inside,
        whatever the caller's context (``_step_bf16``); an f32 state runs outside autocast only."""
        if x.dim() != 3 or x.shape[1] != 1 or x.shape[0] != state.batch:
            raise ValueError(f"step takes one row per sequence, (B={state.batch}, 1, dim); got {tuple(x.shape)}")
        if state.host_pos >= state.capacity:
            raise RuntimeError(f"the decode state is full: {state.host_pos} of {state.capacity} rows")
        if state.dtype == torch.bfloat16:
            with torch.autocast("cuda", enabled=False):
                return self._step_bf16(x.float(), state)
        if x.is_cuda and torch.is_autocast_enabled():
            raise RuntimeError(ops.DECODE_AUTOCAST_REFUSAL)
        for layer, self_kv, cross_kv in zip(self.layers, state.self_kv, state.cross_kv):
            x, y = layer.norm2(x, layer.self_attn.decode_step(layer.norm1(x), self_kv, state.pos, ws=state.ws))
            x, y = layer.norm3(x, layer.cross_attn.decode_step(y, cross_kv, context_mask=state.context_mask, append=False,
                                                                   ws=state.ws))
            x = layer.feed_forward(y) + x
        return x

    def _step_bf16(self, x, state, prefill_ws=None):
        """The step on a bf16 state, or -- with ``prefill_ws``, a workspace of ops.attention_prefill -- the same arithmetic
        on the n rows of x (B, n, dim) in one pass (``prefill``; above ops.ROWS_GEMM_MAX_M rows ``linear_rows`` goes to
        the library's bf16 GEMM).  The residual stream x stays f32; every LayerNorm that only feeds projections
        writes bf16 directly (amk_add_layernorm_mixed_fwd, the bf16 branch output as its bf16 operand and the f32
        stream as the residual); projections, W_o and the FFN's two Linear layers run on the row GEMM
        (amk_gemm_rows_bf16) with bf16 output, q and kv of self-attention as ONE product whose column slices the
        attention kernel reads in place; the FFN's gate + LayerNorm is amk_geglu_ln_bf16_fwd, or -- where its inner
        width is no multiple of 8 or above 4096, as int(dim * 8 / 3) is at dim 64 and 512 -- gelu(val) * gate and the
        LayerNorm as f32 torch ops on the bf16 pre-activations.  A layer's FFN output joins the stream inside the
        next layer's first LayerNorm."""
        b, n = state.batch, x.shape[1]
        if prefill_ws is None:
            attend, ws = ops.attention_decode, state.ws
        else:
            attend, ws = ops.attention_prefill, prefill_ws
        branch = None                       # the bf16 branch output not yet added to the stream
        for layer, w, self_kv, cross_kv in zip(self.layers, state.weights, state.self_kv, state.cross_kv):
            sa, ca = layer.self_attn, layer.cross_attn
            hd = sa.num_heads * sa.dim_head
            if branch is None:
                y = ops.layer_norm_to_bf16(x, None, layer.norm1.gamma, layer.norm1.beta)[1]
            else:
                x, y = ops.layer_norm_to_bf16(branch, x, layer.norm1.gamma, layer.norm1.beta)
            qkv = ops.linear_rows(y.view(b * n, -1), w["qkv"]).view(b, n, 3 * hd)
            o = attend(qkv[:, :, :hd], qkv[:, :, hd:], self_kv, state.pos, sa.num_heads, sa.dim_head, sa.scale, ws=ws)
            o = ops.linear_rows(o.view(b * n, hd), w["wo"], sa.W_o.bias)
            x, y = ops.layer_norm_to_bf16(o.view(b, n, -1), x, layer.norm2.gamma, layer.norm2.beta)
            q = ops.linear_rows(y.view(b * n, -1), w["cq"]).view(b, n, hd)
            o = attend(q, None, cross_kv, None, ca.num_heads, ca.dim_head, ca.scale, key_mask=state.context_mask, ws=ws)
            o = ops.linear_rows(o.view(b * n, hd), w["cwo"], ca.W_o.bias)
            x, y = ops.layer_norm_to_bf16(o.view(b, n, -1), x, layer.norm3.gamma, layer.norm3.beta)
            norm = layer.feed_forward.ff[2]
            ab = ops.linear_rows(y.view(b * n, -1), w["ff1"])
            inner = ab.shape[1] // 2
            if inner % 8 == 0 and inner <= 4096 and ab.stride(0) % 8 == 0:
                g = ops.geglu_ln_bf16_fwd(ab, norm.gamma, norm.beta)[0]
            else:
                val, gate = ab.float().chunk(2, dim=-1)
                g = torch.empty((b * n, (inner + 7) // 8 * 8), device=ab.device, dtype=torch.bfloat16)[:, :inner]
                g.copy_(F.layer_norm(gate * F.gelu(val), (inner,), norm.gamma, norm.beta))   # rows at a stride of 8
            branch = ops.linear_rows(g, w["ff2"]).view(b, n, -1)
        return x + branch.float() if branch is not None else x

    @torch.no_grad()
    def prefill(self, x, state):
        """``forward`` with the causal mask for n new rows x (B, n, dim) at the state's position, in one pass: the rows'
        keys and values become cache rows pos .. pos + n - 1 and row i attends rows 0 .. pos + i (ops.attention_prefill,
        append mode for self-attention, read mode for cross-attention: no tile kernel and no mask tensor in either
        dtype).  Returns (B, n, dim); the caller advances the position (``state.advance(n)``).  The refusals are those of
        ``step``; a bf16 state runs ``_step_bf16``'s arithmetic on the n rows with autocast disabled inside.  Eager
        only: the launch's grid depends on n, so a prefill is never captured."""
        if x.dim() != 3 or x.shape[1] < 1 or x.shape[0] != state.batch:
            raise ValueError(f"prefill takes n >= 1 rows per sequence, (B={state.batch}, n, dim); got {tuple(x.shape)}")
        n = x.shape[1]
        if state.host_pos + n > state.capacity:
            raise RuntimeError(f"the decode state has no room for {n} rows: {state.host_pos} of {state.capacity} are taken")
        attn = self.layers[0].self_attn
        need = max(ops.attention_prefill_ws_floats(state.batch, attn.num_heads, attn.dim_head, rows, n)
                   for rows in (state.capacity, state.cross_kv[0].shape[1]))
        ws = torch.empty((need,), device=x.device, dtype=torch.float32)   # one for every call: ordered on the stream
        if state.dtype == torch.bfloat16:
            with torch.autocast("cuda", enabled=False):
                return self._step_bf16(x.float(), state, prefill_ws=ws)
        if x.is_cuda and torch.is_autocast_enabled():
            raise RuntimeError(ops.DECODE_AUTOCAST_REFUSAL)
        for layer, self_kv, cross_kv in zip(self.layers, state.self_kv, state.cross_kv):
            x, y = layer.norm2(x, layer.self_attn.prefill_rows(layer.norm1(x), self_kv, state.pos, ws=ws))
            x, y = layer.norm3(x, layer.cross_attn.prefill_rows(y, cross_kv, context_mask=state.context_mask, append=False,
                                                                  ws=ws))
            x = layer.feed_forward(y) + x
        return x

    @torch.no_grad()
    def logits_rows(self, out, state, norm, linear):
        """``logits`` for every row of ``out`` (B, n, dim): (B, n, classes) f32."""
        if state.dtype != torch.bfloat16:
            return linear(norm(out))
        if state.head is None:
            raise RuntimeError("this decode state was made without a head: pass init_state(head=...)")
        with torch.autocast("cuda", enabled=False):
            gamma, beta = (norm.gamma, norm.beta) if hasattr(norm, "gamma") else (norm.weight, norm.bias)
            y = ops.layer_norm_to_bf16(out.float(), None, gamma, beta)[1]
            lg = ops.linear_rows(y.view(-1, y.shape[-1]), state.head["head"], linear.bias, torch.float32, w32=linear.weight)
            return lg.reshape(out.shape[0], out.shape[1], -1)

    @torch.no_grad()
    def logits(self, out, state, norm, linear):
        """(B, n) f32 logits of a step's output ``out`` (B, 1, dim): ``linear(norm(out))``.  On a bf16 state: the
        LayerNorm writes bf16, the product runs on the row GEMM over the state's bf16 copy of the head with the f32
        master bias added in f32, and the logits stay f32 (the sampler and ``trace`` read f32)."""
        if state.dtype != torch.bfloat16:
            return linear(norm(out))[:, 0, :]
        if state.head is None:
            raise RuntimeError("this decode state was made without a head: pass init_state(head=...)")
        with torch.autocast("cuda", enabled=False):
            gamma, beta = (norm.gamma, norm.beta) if hasattr(norm, "gamma") else (norm.weight, norm.bias)
            y = ops.layer_norm_to_bf16(out.float(), None, gamma, beta)[1]
            lg = ops.linear_rows(y.view(state.batch, -1), state.head["head"], linear.bias, torch.float32, w32=linear.weight)
            return lg if lg.is_contiguous() else lg.contiguous()


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

    # ---- KV-cached causal decoding: ``forward``'s arithmetic row by row (``generate`` above stays the reference's loop)
    @torch.no_grad()
    def begin_decode(self, src_seq, capacity=256, out=None):
        """Encode ``src_seq`` as ``forward`` does (enc_init_norm, the all-true context mask, enc_final_norm) and return
        the decode state for up to ``capacity`` target positions (bf16 under bf16 autocast, see ``Decoder.init_state``).
        out: a state to refill in place."""
        context_mask = torch.ones(src_seq.shape, dtype=torch.bool, device=src_seq.device)
        src = self.enc_init_norm(self.pos_enc(self.enc_input_proj(src_seq)))
        context = self.enc_final_norm(self.encoder(src, context_mask=context_mask))
        return self.decoder.init_state(context, capacity, context_mask=context_mask, out=out, head=self.linear)

    @torch.no_grad()
    def next_logits(self, state, prev_tokens):
        """(B, n_classes) logits of the next position given the token ``prev_tokens`` (B,) at the state's position:
        row ``pos`` of ``forward(src, tgt)`` with tgt[:, pos] = prev_tokens and the earlier columns as fed before."""
        pe = self.pos_enc.pe.index_select(0, state.pos)
        x = self.pos_enc.dropout(self.dec_input_proj(prev_tokens.view(-1, 1)) + pe)
        out = self.decoder.step(self.dec_init_norm(x), state)
        logits = self.decoder.logits(out, state, self.dec_final_norm, self.linear)
        state.advance()
        return logits

    @torch.no_grad()
    def prefill(self, state, tokens, all_logits=False):
        """``next_logits`` for the n target tokens ``tokens`` (B, n) at positions pos .. pos + n - 1 in ONE pass
        (``Decoder.prefill``): what n calls of ``next_logits(state, tokens[:, i])`` compute and leave in the caches.
        Returns the last row's logits (B, n_classes), or every row's (B, n, n_classes) with ``all_logits``; f32.  The
        position advances by n."""
        if tokens.dim() != 2 or tokens.shape[0] != state.batch or tokens.shape[1] < 1:
            raise ValueError(f"prefill takes tokens (B={state.batch}, n >= 1); got {tuple(tokens.shape)}")
        p, n = state.host_pos, tokens.shape[1]
        if p + n > state.capacity:
            raise RuntimeError(f"the decode state has no room for {n} rows: {p} of {state.capacity} are taken")
        x = self.pos_enc.dropout(self.dec_input_proj(tokens) + self.pos_enc.pe[p:p + n])
        out = self.decoder.prefill(self.dec_init_norm(x), state)
        if all_logits:
            logits = self.decoder.logits_rows(out, state, self.dec_final_norm, self.linear)
        else:
            logits = self.decoder.logits(out[:, -1:], state, self.dec_final_norm, self.linear)
        state.advance(n)
        return logits

    @torch.no_grad()
    def sample(self, src_seq, max_len, gumbel=None, prefix=None):
        """``generate``'s loop on the trained (causal, normed) model with cached keys and values: start token 1,
        Gumbel-argmax over the unfiltered logits, stop when the FIRST sequence draws the end token 2 (one host read per
        step) or after ``max_len`` tokens.  gumbel: explicit noise (steps, B, n_classes), indexed by the absolute step.
        prefix (B, k), k < max_len: target tokens the caller already has; they follow the start token, go through the
        decoder in one ``prefill`` pass and are kept in the result, and the loop starts at step k."""
        if max_len is None or max_len < 1:
            raise ValueError("Transformer.sample needs a positive max_len: it sizes the key / value cache")
        end_token = 2
        out_seq = torch.ones((src_seq.shape[0], 1), dtype=torch.long, device=src_seq.device)
        state = self.begin_decode(src_seq, capacity=max_len)
        first = 0
        if prefix is not None:
            if prefix.dim() != 2 or prefix.shape[0] != src_seq.shape[0] or prefix.shape[1] >= max_len:
                raise ValueError(f"prefix must be (B={src_seq.shape[0]}, k < max_len={max_len}); got {tuple(prefix.shape)}")
        if prefix is not None and prefix.shape[1] > 0:
            first = prefix.shape[1]
            out_seq = torch.cat((out_seq, prefix.to(out_seq)), dim=1)
            self.prefill(state, out_seq[:, :-1])      # rows 0 .. k - 1; the loop feeds the prefix's last token
        for i in range(first, max_len):
            logits = self.next_logits(state, out_seq[:, -1])
            noise = gumbel[i] if gumbel is not None else -torch.empty_like(logits).exponential_().log()
            last_token = (logits + noise).argmax(dim=-1)
            if last_token[0] == end_token:
                break
            out_seq = torch.cat((out_seq, last_token.unsqueeze(1)), dim=1)
        return out_seq
