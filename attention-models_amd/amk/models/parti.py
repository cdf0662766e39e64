"""Autoregressive text-to-image transformer over frozen VQ codes (reference: models/parti.py:49-155).  The decoder stack
runs on the HIP attention kernels: causal self-attention over the image tokens, cross-attention onto the text positions.

What differs from the reference, and why: its TextEncoder downloads a CLIP text tower (``CLIPTextModel.from_pretrained``,
models/parti.py:36-37), which is not available here, so -- as ``MUSE`` does -- ``Parti`` takes the tower's OUTPUT
(``text_hidden`` (B, L, dim)) instead of strings and constructs no TextEncoder; ``enc_type``, ``enc_name`` and
``max_length`` keep their places in the constructor and are not used.  Everything downstream follows the reference,
quirks included: ``generate`` runs the whole prefix through the decoder at every step, WITHOUT a causal mask, without
``context_norm`` on the text embeddings, and discards the results of ``init_norm`` and ``final_norm`` (reference
:142-144), so a KV-cached causal decode would not compute what it computes.  ``generate`` stays that loop.

Sampling from the distribution ``forward`` trains is a loop of its own next to it: ``begin_decode`` (context_norm, the
context's K|V projected once), ``next_logits`` (one row through init_norm, ``Decoder.step`` on the single-token attention
kernel of csrc/attn_decode.hip, final_norm, to_logits) and ``sample`` (``generate``'s top-k filter and Gumbel-argmax, one
token per step against cached keys and values; ``graph=True`` replays one captured step for every position).
"""
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .layers import LayerNorm, Linear
from .muse import filter_logits
from .positional_encoding import PositionalEncoding
from .transformer import Decoder


# module -> its captured decode step (Parti._sample_graphed)
_DECODE_GRAPHS = weakref.WeakKeyDictionary()


class Parti(nn.Module):
    def __init__(self, dim, vq, enc_type=None, enc_name=None, max_length=77, n_heads=8, d_head=64, depth=6):
        super().__init__()
        self.dim = dim
        self.vq = vq
        self.max_length = max_length
        self.context_norm = LayerNorm(dim)

        self.start_token = nn.Parameter(torch.randn(dim))
        codebook_size = vq.codebook.codebook_size
        self.token_emb = nn.Embedding(codebook_size, dim)
        self.pos_enc = PositionalEncoding(dim)

        self.transformer_decoder = Decoder(dim, n_heads, d_head, depth)
        self.init_norm = LayerNorm(dim)
        self.final_norm = LayerNorm(dim)
        self.to_logits = Linear(dim, codebook_size)

        self.vq.requires_grad_(False)
        self.decode_graph_captures = 0   # captures taken by sample(graph=True), for tests and diagnostics

    @staticmethod
    def _context(text_hidden):
        if not torch.is_tensor(text_hidden):
            raise TypeError("Parti here takes CLIP's last hidden state (B, L, dim); the CLIP tower itself "
                            "(CLIPTextModel.from_pretrained) needs a download that is not available")
        return text_hidden

    def forward(self, text_hidden, imgs):
        """The training loss (reference :84-124): next-token cross-entropy over all T image tokens."""
        text_embeds = self.context_norm(self._context(text_hidden))
        with torch.no_grad():
            labels = self.vq.encode_imgs(imgs)                       # (B, T)
        b = labels.shape[0]
        x = self.pos_enc(self.token_emb(labels[:, :-1]))             # the decoder's input: tokens shifted right ...
        x = torch.cat((self.start_token.expand(b, 1, -1), x), dim=1)  # ... behind the start token
        t = x.shape[1]
        x = self.init_norm(x)
        out = self.transformer_decoder(dec_in=x, context=text_embeds, causal_mask=ops.causal_mask(t, t, x.device))
        if ops.ce_head_ok(out, self.to_logits.weight, self.to_logits.bias):
            return self.loss_from_hidden(out, labels)
        logits = self.to_logits(self.final_norm(out))
        return F.cross_entropy(logits.transpose(1, 2), labels)

    def loss_from_hidden(self, hidden, labels):
        """The training loss from the decoder's output without the logits in memory: final_norm, then the fused logits +
        bias + cross-entropy head (csrc/ce_head.hip, csrc/ce_head_bf16.hip under bf16 autocast)."""
        return ops.linear_cross_entropy(self.final_norm(hidden), self.to_logits.weight, labels, -100,
                                        bias=self.to_logits.bias)

    @torch.no_grad()
    def generate(self, text_hidden, gumbel=None, trace=None):
        """Token-by-token sampling (reference :126-155), as written there -- see the module docstring.  gumbel: explicit
        noise (steps, B, V) in place of the sampler's own draw (tests replay the reference's); trace: a list that
        receives every step's unfiltered last-row logits (B, V)."""
        text_embeds = self._context(text_hidden)
        b = text_embeds.shape[0]
        start = self.start_token.expand(b, 1, -1)
        indices = torch.zeros(b, 0, dtype=torch.long, device=text_embeds.device)
        for i in range(self.vq.num_patches):
            x = torch.cat((start, self.pos_enc(self.token_emb(indices))), dim=1)
            logits = self.to_logits(self.transformer_decoder(dec_in=x, context=text_embeds))
            if trace is not None:
                trace.append(logits[:, -1, :].clone())
            last = filter_logits(logits, p=0.9)[:, -1, :]
            if gumbel is None:
                token = F.gumbel_softmax(last, tau=1, hard=False).argmax(dim=-1)
            else:
                token = (last + gumbel[i]).argmax(dim=-1)             # argmax softmax(x + g) = argmax (x + g)
            indices = torch.cat((indices, token.unsqueeze(1)), dim=1)
        return self.vq.decode_indices(indices)

    # ---- KV-cached causal decoding: ``forward``'s arithmetic row by row, i.e. sampling from the trained distribution
    @torch.no_grad()
    def begin_decode(self, text_hidden, capacity=None, out=None):
        """The decode state over ``context_norm(text_hidden)`` for up to ``capacity`` image tokens (default: all
        ``vq.num_patches``).  out: a state to refill in place."""
        capacity = self.vq.num_patches if capacity is None else int(capacity)
        if capacity < self.vq.num_patches:
            raise ValueError(f"capacity {capacity} is smaller than the {self.vq.num_patches} image tokens of a sample")
        text_embeds = self.context_norm(self._context(text_hidden))
        return self.transformer_decoder.init_state(text_embeds, capacity, out=out, head=self.to_logits)

    @torch.no_grad()
    def next_logits(self, state, prev_tokens=None):
        """(B, V) logits of the token at the state's position: row ``pos`` of ``forward``'s logits.  The decoder's input
        row is the start token at position 0 (prev_tokens None) and token_emb(prev_tokens) + pe[pos - 1] after it; it
        goes through init_norm, ``Decoder.step``, final_norm and to_logits, then the position advances.  The position
        and the ``pe`` row are read on the device."""
        if prev_tokens is None:
            if state.host_pos != 0:
                raise ValueError("only position 0 takes the start token; pass the previous tokens")
            x = self.start_token.expand(state.batch, 1, -1)
        else:
            pe = self.pos_enc.pe.index_select(0, state.pos - 1)
            x = self.pos_enc.dropout(self.token_emb(prev_tokens.view(-1, 1)) + pe)
        out = self.transformer_decoder.step(self.init_norm(x), state)
        logits = self.transformer_decoder.logits(out, state, self.final_norm, self.to_logits)
        state.advance()
        return logits

    @torch.no_grad()
    def prefill(self, state, tokens, all_logits=False):
        """The decode conditioned on tokens the caller already has, in ONE pass (``Decoder.prefill``, the many-row kernel
        of csrc/attn_prefill.hip): what ``next_logits(state, None)`` followed by ``next_logits(state, tokens[:, i])`` in
        turn compute and leave in the caches.  tokens (B, n) are the image tokens from the state's position on.  At
        position 0 the start-token row is prepended, so n + 1 rows go through and the last one is the row of token n;
        at position p > 0 the rows are token_emb(tokens) + pe[p - 1 ...], as ``next_logits`` feeds them.  Returns the
        last row's logits (B, V), or every row's (B, rows, V) with ``all_logits``; f32.  The position advances by the
        number of rows."""
        if tokens.dim() != 2 or tokens.shape[0] != state.batch:
            raise ValueError(f"prefill takes tokens (B={state.batch}, n); got {tuple(tokens.shape)}")
        p, n = state.host_pos, tokens.shape[1]
        rows = n + 1 if p == 0 else n
        if rows < 1:
            raise ValueError("prefill needs at least one token after position 0")
        if p + rows > state.capacity:
            raise RuntimeError(f"the decode state has no room for {rows} rows: {p} of {state.capacity} are taken")
        x = self.token_emb(tokens) + self.pos_enc.pe[max(p - 1, 0):max(p - 1, 0) + n]
        x = self.pos_enc.dropout(x)
        if p == 0:
            x = torch.cat((self.start_token.expand(state.batch, 1, -1), x), dim=1)
        out = self.transformer_decoder.prefill(self.init_norm(x), state)
        if all_logits:
            logits = self.transformer_decoder.logits_rows(out, state, self.final_norm, self.to_logits)
        else:
            logits = self.transformer_decoder.logits(out[:, -1:], state, self.final_norm, self.to_logits)
        state.advance(rows)
        return logits

    def _prefill_prefix(self, state, prefix_ids, trace):
        """``prefill`` of a sample's given tokens from position 0: the logits of the first token to draw, with every
        earlier step's logits appended to ``trace`` so that it stays indexed by the absolute step."""
        if trace is None:
            return self.prefill(state, prefix_ids)
        logits = self.prefill(state, prefix_ids, all_logits=True)
        trace.extend(logits[:, i].clone() for i in range(logits.shape[1] - 1))
        return logits[:, -1].contiguous()

    def _draw(self, logits, ids, noise, tau, p):
        """generate's sampler on (B, V) logits into ids (B, 1) int64, in place: top-ceil((1 - p) V) filter, then the
        argmax of logits + Gumbel noise (= the argmax of the Gumbel-softmax at any temperature tau > 0).  noise None:
        drawn by the kernel's own Philox stream (eager only: its seed and offset are host values)."""
        v = logits.shape[-1]
        if v % 4 == 0 and v <= 36864:     # csrc/sample.hip holds one row in LDS
            if noise is None:
                ops.sample_step(logits.unsqueeze(1), ids, tau=tau, p=p)
            else:   # explicit noise: the kernel draws nothing; a fixed seed keeps torch's generator out of a capture
                ops.sample_step(logits.unsqueeze(1), ids, tau=tau, p=p, gumbel=noise.unsqueeze(1), seed=0)
            return
        if noise is None:
            noise = -torch.empty_like(logits).exponential_().log()
        ids.copy_((filter_logits(logits.unsqueeze(1), p=p)[:, 0, :] + noise).argmax(dim=-1, keepdim=True))

    @torch.no_grad()
    def sample(self, text_hidden, gumbel=None, trace=None, tau=1.0, p=0.9, graph=False, prefix_ids=None):
        """Sample ``vq.num_patches`` tokens from the model as trained -- context_norm, init_norm, causal self-attention,
        final_norm -- one token per step against cached keys and values, with ``generate``'s sampler; returns
        ``vq.decode_indices(ids)``.  gumbel: explicit noise (steps, B, V); trace: a list that receives every step's
        unfiltered logits (B, V).  graph=True: the step from the previous ids on the device to the next ids on the
        device is captured once as a HIP graph and replayed ``num_patches - 1`` times (the start-token step stays
        eager); without explicit noise the noise is then drawn inside the graph by torch's capture-aware generator.  The
        captured step and its caches stay alive with the module until ``drop_decode_graph()`` (see ``_sample_graphed``).

        prefix_ids (B, k), k < num_patches: the sample's first k tokens, given (the first rows of an image from
        ``vq.encode_imgs``, say).  They are kept as they are and go through the decoder in one ``prefill`` pass; the
        loop starts at step k.  ``gumbel`` and ``trace`` stay indexed by the absolute step (the trace receives the given
        steps' logits too).  With graph=True the prefill runs eagerly and the captured step is replayed after it: that
        step reads the position on the device, so nothing new is captured."""
        if not tau > 0:
            raise ValueError("sample needs a temperature tau > 0")
        steps = self.vq.num_patches
        text_hidden = self._context(text_hidden)
        if gumbel is not None and gumbel.shape[0] < steps:
            raise ValueError(f"gumbel holds {gumbel.shape[0]} steps of noise, the sample has {steps}")
        k = 0
        if prefix_ids is not None:
            if prefix_ids.dim() != 2 or prefix_ids.shape[0] != text_hidden.shape[0] or prefix_ids.shape[1] >= steps:
                raise ValueError(f"prefix_ids must be (B={text_hidden.shape[0]}, k < {steps}); got {tuple(prefix_ids.shape)}")
            k = prefix_ids.shape[1]
        if graph:
            indices = self._sample_graphed(text_hidden, gumbel, trace, tau, p, prefix_ids if k else None)
            return self.vq.decode_indices(indices)
        state = self.begin_decode(text_hidden)
        b = state.batch
        indices = torch.empty((b, steps), dtype=torch.long, device=state.device)
        token = torch.zeros((b, 1), dtype=torch.long, device=state.device)
        if k:
            indices[:, :k] = prefix_ids
        for i in range(k, steps):
            if i == k and k:
                logits = self._prefill_prefix(state, prefix_ids, trace)   # the start token and the k given tokens
            else:
                logits = self.next_logits(state, token if i else None)
            if trace is not None:
                trace.append(logits.clone())
            self._draw(logits, token, None if gumbel is None else gumbel[i], tau, p)
            indices[:, i] = token[:, 0]
        return self.vq.decode_indices(indices)

    def drop_decode_graph(self):
        """Free the captured step of ``sample(graph=True)`` with its caches and noise buffer (see ``_sample_graphed``)."""
        _DECODE_GRAPHS.pop(self, None)

    def _sample_graphed(self, text_hidden, gumbel, trace, tau, p, prefix_ids=None):
        """One captured step per module, kept in a table outside the module (weakly keyed: it goes with the module, is
        not part of its attributes or state_dict, and copy.deepcopy does not meet it) until ``drop_decode_graph()`` or
        a call whose key differs: it holds the DecoderState -- every layer's (B, capacity, 2*h*d) cache -- and the
        noise buffer.  A captured graph replays against the ADDRESSES it was captured with, so the key holds, besides
        the shapes and the sampler's settings, the train / eval mode, ops.GEMM_MODE and the data pointer of every
        parameter and buffer: a module moved, cast or re-flattened is captured anew instead of replayed on stale
        memory.  Parameter VALUES may change between calls (the graph reads them where they are).

        prefix_ids: the sample's given tokens.  They are no part of the key: the capture is the one-row step, taken
        after an eager start-token step as without a prefix; the prefill then runs eagerly from position 0 again and
        rewrites every cache row the start step and the warm-up wrote, and the replays go on from position k + 1."""
        steps = self.vq.num_patches
        k = 0 if prefix_ids is None else prefix_ids.shape[1]
        key = (tuple(text_hidden.shape), text_hidden.device, None if gumbel is None else tuple(gumbel.shape),
               float(tau), float(p), steps, self.training, ops.GEMM_MODE,
               self.transformer_decoder.decode_dtype(text_hidden.device), ops.DECODE_BF16,
               tuple(t.data_ptr() for t in list(self.parameters()) + list(self.buffers())))
        cached = _DECODE_GRAPHS.get(self)
        if cached is None or cached["key"] != key:
            cached = {"key": key, "state": self.begin_decode(text_hidden), "graph": None,
                      "noise": None if gumbel is None else torch.empty_like(gumbel)}
            b = cached["state"].batch
            cached["token"] = torch.zeros((b, 1), dtype=torch.long, device=text_hidden.device)
            _DECODE_GRAPHS[self] = cached
        else:
            self.begin_decode(text_hidden, out=cached["state"])   # new context K|V into the same buffers, position 0
        state, token, noise = cached["state"], cached["token"], cached["noise"]
        if noise is not None:
            noise.copy_(gumbel)
        indices = torch.empty((state.batch, steps), dtype=torch.long, device=state.device)
        if k == 0 or cached["graph"] is None:
            # the start-token step, eager (with a prefix: only as the ground the capture below warms up on)
            logits = self.next_logits(state, None)
            if trace is not None and k == 0:
                trace.append(logits.clone())
            self._draw(logits, token, None if noise is None else noise[0], tau, p)
            indices[:, 0] = token[:, 0]
            if steps == 1:
                return indices

        def step():
            # previous ids (token) -> next ids (token, in place); position, pe row and noise row by the device position
            if noise is not None:
                g = noise.index_select(0, state.pos)[0]
            else:
                g = None
            lg = self.next_logits(state, token)
            if g is None:
                g = -torch.empty_like(lg).exponential_().log()
            self._draw(lg, token, g, tau, p)
            return lg

        if cached["graph"] is None:
            first = token.clone()
            check, ops.CHECK_INDICES = ops.CHECK_INDICES, False   # no host read inside a capture
            try:
                # warm-up on a side stream, then the capture, as amk.graphs.GraphedStep does; every run starts at
                # position 1 (one stream, no parallel branches, no host reads in `step`)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(3):
                        state.set_position(1)
                        step()
                torch.cuda.current_stream().wait_stream(side)
                state.set_position(1)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static_logits = step()
                cached["graph"], cached["logits"] = graph, static_logits
                self.decode_graph_captures += 1
            finally:
                ops.CHECK_INDICES = check
            # the warm-up runs moved the position and the ids; the cache row they wrote is rewritten before it is read
            state.set_position(1)
            token.copy_(first)
        if k:
            state.reset()
            logits = self._prefill_prefix(state, prefix_ids, trace)
            if trace is not None:
                trace.append(logits.clone())
            self._draw(logits, token, None if noise is None else noise[k], tau, p)
            indices[:, :k] = prefix_ids
            indices[:, k] = token[:, 0]
        for i in range(k + 1, steps):
            cached["graph"].replay()
            if trace is not None:
                trace.append(cached["logits"].clone())
            indices[:, i] = token[:, 0]
        state.host_pos = steps
        return indices
