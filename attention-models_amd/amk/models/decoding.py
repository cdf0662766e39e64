"""State of a KV-cached causal decode (``Decoder.init_state`` / ``Decoder.step``): what one new row per step needs from
the rows before it, kept on the device.

Per decoder layer: the self-attention cache (B, capacity, 2*h*d) in the kv projection's own '(kv h d)' columns, filled
one row per step by the decode kernel itself (csrc/attn_decode.hip, append mode), and the cross-attention K|V of the
context (B, L, 2*h*d), projected ONCE.  The position is a device int32: the kernel reads the number of valid rows on
the device, so a captured step can be replayed for every position.  ``host_pos`` mirrors it on the host for the eager
loop's capacity check only; a graph replay advances the device position alone (see ``Parti.sample``).
``Decoder.prefill`` fills n rows of every cache in one pass (csrc/attn_prefill.hip) from the same position.

A bf16 state (``Decoder.init_state`` under bf16 autocast, AMK_DECODE_BF16) holds bf16 caches and cross K|V and its own
bf16 copies of the Linear weights the step reads, so that a captured step reads state-owned and parameter memory only
-- never autocast's weight-cast cache, which is freed when the autocast context exits.
"""
import torch


class DecoderState:
    def __init__(self, self_kv, cross_kv, context_mask, capacity, ws=None, weights=None, head=None):
        self.self_kv = self_kv            # per layer (B, capacity, 2*h*d)
        self.cross_kv = cross_kv          # per layer (B, L, 2*h*d)
        self.context_mask = context_mask  # uint8 (B, L) or None
        self.capacity = int(capacity)
        self.ws = ws                      # the decode kernel's workspace, shared by every call of a step (stream order)
        self.dtype = self_kv[0].dtype      # float32, or bfloat16: the decode under bf16 autocast
        self.weights = weights            # bf16 state: per layer {name: bf16 copy of the Linear weights the step reads}
        self.head = head                  # bf16 state: {"head": bf16 copy of the Linear onto the logits} or None
        self.batch = self_kv[0].shape[0]
        self.pos = torch.zeros(1, dtype=torch.int32, device=self_kv[0].device)
        self.host_pos = 0

    @property
    def device(self):
        return self.pos.device

    def reset(self):
        """Back to position 0.  The caches keep their rows: a row is rewritten before any step reads it."""
        self.pos.zero_()
        self.host_pos = 0

    def advance(self, n=1):
        """n more rows are valid: one after a step, the whole chunk after ``Decoder.prefill``."""
        self.pos.add_(int(n))
        self.host_pos += int(n)

    def set_position(self, n):
        self.pos.fill_(int(n))
        self.host_pos = int(n)
