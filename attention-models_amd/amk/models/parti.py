"""Autoregressive text-to-image transformer over frozen VQ codes (reference: models/parti.py:49-155).  The decoder stack
runs on the HIP attention kernels: causal self-attention over the image tokens, cross-attention onto the text positions.

What differs from the reference, and why: its TextEncoder downloads a CLIP text tower (``CLIPTextModel.from_pretrained``,
models/parti.py:36-37), which is not available here, so -- as ``MUSE`` does -- ``Parti`` takes the tower's OUTPUT
(``text_hidden`` (B, L, dim)) instead of strings and constructs no TextEncoder; ``enc_type``, ``enc_name`` and
``max_length`` keep their places in the constructor and are not used.  Everything downstream follows the reference,
quirks included: ``generate`` runs the whole prefix through the decoder at every step, WITHOUT a causal mask, without
``context_norm`` on the text embeddings, and discards the results of ``init_norm`` and ``final_norm`` (reference
:142-144), so a KV-cached causal decode would not compute what it computes.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .layers import LayerNorm, Linear
from .muse import filter_logits
from .positional_encoding import PositionalEncoding
from .transformer import Decoder


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
