"""torch.autograd wrappers over the libamk.so C ABI.

torch is plumbing here: it owns device memory, streams and the autograd graph; every FLOP of
the hot path runs in the HIP kernels of ``csrc/``.  Inputs must be fp32 HIP tensors -- there
is deliberately no CPU / eager path ("no fallback").
"""
import ctypes
import os
import weakref

import torch
from torch.autograd.function import once_differentiable

from . import lib as _lib

_NULL = ctypes.c_void_p(0)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else _NULL


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional in-situ kernel timing: set to a dict and every hot-path ABI call is bracketed by two HIP
# events on the launch stream (bench.py does this during its timed steps); None = no events.
KERNEL_EVENTS = None


class _timed:
    """with _timed("name"): <one ABI call>  -- records (start, end) events when KERNEL_EVENTS is a dict."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if KERNEL_EVENTS is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if KERNEL_EVENTS is not None:
            self.b.record()
            KERNEL_EVENTS.setdefault(self.name, []).append((self.a, self.b))
        return False


def kernel_event_summary(events):
    """{name: (launches, average ms)} after a device synchronize."""
    out = {}
    for name, pairs in events.items():
        ms = [a.elapsed_time(b) for a, b in pairs]
        out[name] = (len(ms), sum(ms) / len(ms))
    return out


def _require_device(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "amk ops run only on MI355X (HIP) tensors; got a CPU tensor. There is no CPU fallback."
            )
        if t.is_floating_point() and t.dtype != torch.float32:
            raise RuntimeError(f"amk kernels compute in fp32; got {t.dtype}")


# ---------------------------------------------------------------------------- attention
def _strides4(t):
    """(sb, st, sh) element strides of a (B, H, T, D) view whose last axis is contiguous."""
    return (t.stride(0), t.stride(2), t.stride(1))


def _kernel_view_ok(t):
    return (
        t.stride(3) == 1
        and t.data_ptr() % 16 == 0
        and all(s % 4 == 0 for s in (t.stride(0), t.stride(1), t.stride(2)))
    )


def _as_kernel_view(t):
    """Return a (B,H,T,D) view the kernels can address; copy only if the layout forces it."""
    if _kernel_view_ok(t):
        return t
    B, H, T, D = t.shape
    return t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)  # (B,T,H,D) storage


def _new_bthd(B, H, T, D, like, dtype=torch.float32):
    """(B,H,T,D) view over fresh (B,T,H*D) storage: the layout the W_o projection consumes."""
    return torch.empty((B, T, H, D), device=like.device, dtype=dtype).permute(0, 2, 1, 3)


def _mask_u8(mask, shape, what):
    if mask is None:
        return None
    m = mask
    while m.dim() > len(shape) and m.shape[0] == 1:
        m = m[0]
    if m.dim() != len(shape):
        raise RuntimeError(f"{what} must have {len(shape)} dims (got shape {tuple(mask.shape)})")
    m = m.expand(*shape)
    return m.to(torch.uint8).contiguous()


# The reference's models build one causal mask only, torch.ones(I, J).triu(J - I + 1) (models/parti.py:111-112,
# models/transformer.py:167-168): key j of query i is masked iff j >= i + (J - I + 1).  causal_mask returns it, one
# tensor per (I, J, device), so that a model does not rebuild it every step.
_causal_masks = {}


def causal_mask(I, J, device):
    """The reference's causal mask, bool (I, J), True = masked: torch.ones(I, J).triu(J - I + 1).  Cached per
    (I, J, device); do not write to it."""
    key = (int(I), int(J), torch.device(device))
    m = _causal_masks.get(key)
    if m is None:
        m = torch.ones((key[0], key[1]), dtype=torch.bool, device=key[2]).triu(key[1] - key[0] + 1)
        _causal_masks[key] = m
    return m


# Forward path of the attention core (head dim 64, f32): "f32" = exact-f32 MFMA (v_mfma_f32_32x32x2_f32); "bf16x6" = the
# same algorithm with every product formed from three-way bf16 splits of its f32 operands (six exact partial products,
# f32 accumulation, csrc/attn_fwd_x6.hip): f32-level error at 2.6x the matrix rate, for a pre-pass that splits K and V
# once per call.  Both keep the scores for the fused backward under the same conditions.  "auto" (the default): the
# autograd entry points (attention, attention_fused_kv and the modules on top of them) take the split-bf16 forward when
# the call is large enough (ATTENTION_X6_MIN_KEYS, ATTENTION_X6_MIN_SCORES), the f32 one below; a direct _attn_forward call stays on the f32
# kernel (bench.py times that call against the f32 MFMA peak).  AMK_ATTENTION_FORWARD=f32 restores the f32 launches
# everywhere.
ATTENTION_FORWARD = os.environ.get("AMK_ATTENTION_FORWARD", "auto")
if ATTENTION_FORWARD not in ("auto", "f32", "bf16x6"):
    raise RuntimeError(f"AMK_ATTENTION_FORWARD must be auto, f32 or bf16x6 (got {ATTENTION_FORWARD!r})")
# "auto": the pre-pass is a fixed cost per call (one more launch, 48 KiB written per (batch, head, 64-key tile)) that a
# small call does not earn back.  Measured at batch 32, 8 heads, scores kept, f32 against split-bf16 (pre-pass included,
# profiles/kbench_attn_fwd_x6.log): (I, J) = (1024, 1024) 0.584 / 0.530 ms, (1024, 77) 0.094 / 0.076 ms, (65, 65)
# 0.025 / 0.030 ms.  Back to back the split-bf16 forward wins at 77 keys, but the Muse decoder step, whose
# cross-attention has that shape, ran 0.25 % slower with it under graph replay (194.55 against 194.06 ms, three
# alternating runs each, profiles/attn_fwd_x6_keep_step_breakdown.log).  So "auto" asks for at least two 64-key tiles and
# for at least 2^22 scores in the call ((65, 65) at batch 32 has 2^20).
ATTENTION_X6_MIN_KEYS = 128
ATTENTION_X6_MIN_SCORES = 1 << 22

# Training: the forward leaves the raw scores S (4 bytes per (b, h, i, j), 32x32 tiles) in HBM and the fused
# backward reads them back instead of recomputing S = QK^T -- four matrix products instead of five, bit for
# bit the same results.  The reference keeps the same tensor alive for autograd; 288 GB of HBM make it
# affordable here (1.07 GB per ViT-VQGAN layer at batch 32, 12.9 GB for the twelve layers).  A call whose
# scores would exceed ATTENTION_KEEP_SCORES_MAX_BYTES, or that would take the scores alive across all layers beyond
# ATTENTION_KEEP_SCORES_BUDGET_BYTES (default: a quarter of the device's memory), recomputes instead -- the same
# results from five products, so a deeper model or a larger batch degrades in speed, not into an out-of-memory error.
ATTENTION_KEEP_SCORES = os.environ.get("AMK_ATTN_KEEP_SCORES", "1") == "1"
ATTENTION_KEEP_SCORES_MAX_BYTES = 8 << 30
ATTENTION_KEEP_SCORES_BUDGET_BYTES = int(os.environ.get("AMK_ATTN_KEEP_BUDGET", "0")) or None   # None: memory / 4
_kept_scores_bytes = [0]   # bytes of kept scores alive right now (released when the tensors are freed)


def _keep_budget(device):
    if ATTENTION_KEEP_SCORES_BUDGET_BYTES is not None:
        return ATTENTION_KEEP_SCORES_BUDGET_BYTES
    return torch.cuda.get_device_properties(device).total_memory // 4


def _release_kept(nbytes):
    _kept_scores_bytes[0] -= nbytes
# keys per workgroup of the fused backward: 0 = library default, 128 or 256
ATTENTION_BACKWARD_KEYS = int(os.environ.get("AMK_ATTN_BWD_KEYS", "0"))


def _attn_forward(q, k, v, key_mask, causal_mask, scale, keep_scores=False, auto_x6=False):
    """Returns (q, k, v, o, stats, scores); scores is None unless keep_scores and the scores fit the budgets.
    auto_x6: what ATTENTION_FORWARD == "auto" resolves to for this caller (the autograd entry points pass True)."""
    B, H, I, D = q.shape
    J = k.shape[2]
    _require_device(q, k, v, key_mask, causal_mask)
    if k.shape != (B, H, J, D) or v.shape != (B, H, J, D):
        raise RuntimeError(f"attention shapes disagree: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)}")
    q, k, v = _as_kernel_view(q), _as_kernel_view(k), _as_kernel_view(v)
    o = _new_bthd(B, H, I, D, q)
    stats = torch.empty((B, H, I, 2), device=q.device, dtype=torch.float32)
    L = _lib.load()
    if ATTENTION_FORWARD not in ("auto", "f32", "bf16x6"):
        raise RuntimeError(f"ops.ATTENTION_FORWARD must be auto, f32 or bf16x6 (got {ATTENTION_FORWARD!r})")
    x6 = D == 64 and (ATTENTION_FORWARD == "bf16x6"   # every other head dim runs the plain f32 kernels
                      or (ATTENTION_FORWARD == "auto" and auto_x6 and J >= ATTENTION_X6_MIN_KEYS
                          and B * H * I * J >= ATTENTION_X6_MIN_SCORES))
    ws = torch.empty((L.amk_attn_fwd_x6_ws_bytes(B, H, J),), device=q.device, dtype=torch.uint8) if x6 else None
    scores = None
    # (head dim 128: the score-keeping forward exists without masks, and its one-pass backward takes atomics only.  Head dim
    # 32 has both too, but recomputing wins there -- 0.618 against 0.609 of the f32 MFMA peak: the scores are 4 bytes per
    # (query, key) against only 32 multiply-adds, 2.1 GB per launch at the benchmark shape -- so its scores are not kept.
    # The other head dims, 96 to 256, have no score-keeping forward nor one-pass backward: they always recompute)
    det = DETERMINISTIC_ATTENTION_BACKWARD or torch.are_deterministic_algorithms_enabled()
    keepable = D == 64 or (D == 128 and key_mask is None and causal_mask is None and not det)
    if keep_scores and keepable and ATTENTION_KEEP_SCORES and not ATTENTION_BACKWARD_TWO_KERNEL:
        nbytes = L.amk_attn_scores_bytes(B, H, I, J)
        if nbytes <= ATTENTION_KEEP_SCORES_MAX_BYTES and _kept_scores_bytes[0] + nbytes <= _keep_budget(q.device):
            scores = torch.empty((nbytes // 4,), device=q.device, dtype=torch.float32)
            _kept_scores_bytes[0] += nbytes
            weakref.finalize(scores.untyped_storage(), _release_kept, nbytes)
    # (the split-bf16 launches under names of their own: bench.py sets the attn_fwd_* names against the f32 MFMA peak)
    with _timed(("attn_fwd_x6" if x6 else "attn_fwd") + ("_keep_kernel" if scores is not None else "_kernel")):
        if x6 and scores is not None:
            rc = L.amk_attn_fwd_x6_keep(
                _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(stats), _ptr(ws), _ptr(scores), _ptr(key_mask), _ptr(causal_mask),
                B, H, I, J, D, *_strides4(q), *_strides4(k), *_strides4(v), *_strides4(o),
                float(scale), _stream(),
            )
        elif scores is not None:
            rc = L.amk_attn_fwd_keep(
                _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(stats), _ptr(scores), _ptr(key_mask), _ptr(causal_mask),
                B, H, I, J, D, *_strides4(q), *_strides4(k), *_strides4(v), *_strides4(o),
                float(scale), _stream(),
            )
        elif x6:
            rc = L.amk_attn_fwd_x6(
                _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(stats), _ptr(ws), _ptr(key_mask), _ptr(causal_mask),
                B, H, I, J, D, *_strides4(q), *_strides4(k), *_strides4(v), *_strides4(o),
                float(scale), _stream(),
            )
        else:
            rc = L.amk_attn_fwd(
                _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(stats), _ptr(key_mask), _ptr(causal_mask),
                B, H, I, J, D, *_strides4(q), *_strides4(k), *_strides4(v), *_strides4(o),
                float(scale), _stream(),
            )
    _lib.check(rc, "amk_attn_fwd")
    return q, k, v, o, stats, scores


# Backward path of the attention core (include/amk.h, amk_attn_bwd `stages`): one fused pass.
# Default: dq accumulated with f32 atomics into a zeroed buffer -- the fastest form (1.135 ms at the ViT-VQGAN layer
# shape); dk, dv are reproducible, dq differs in the last bits from run to run.  Reproducible mode (4 % slower,
# 1.179 ms): dq as plain stores -- directly when one workgroup holds all keys of a (batch, head), else per-key-block
# partials summed in order by a second launch -- every gradient bitwise reproducible.  It is taken when
# DETERMINISTIC_ATTENTION_BACKWARD is set (AMK_DETERMINISTIC=1) or torch.use_deterministic_algorithms(True) is on,
# PyTorch's own convention for atomics-based backward kernels.
DETERMINISTIC_ATTENTION_BACKWARD = os.environ.get("AMK_DETERMINISTIC", "0") == "1"
ATTENTION_BACKWARD_TWO_KERNEL = False

# amk_attn_bwd `stages`: the AMK_ATTN_BWD_* defines of include/amk.h (tests/test_abi.py holds the two together)
ATTN_BWD_DELTA = 1
ATTN_BWD_DKDV = 2
ATTN_BWD_DQ = 4
ATTN_BWD_FUSED = 8
ATTN_BWD_ALL = 7          # delta + dK/dV + dQ: reproducible
ATTN_BWD_FAST = 9         # delta + fused
ATTN_BWD_KEYS128 = 16
ATTN_BWD_KEYS256 = 32
ATTN_BWD_DQ_REPRO = 64
ATTN_BWD_FAST_REPRO = 73  # delta + fused + reproducible dq
ATTN_BWD_X6 = 128         # kept-scores fused pass: dV / dK products on split-bf16 MFMA

# The kept-scores backward of head dim 64 at 256 keys per workgroup with its dV and dK products on split-bf16 MFMA
# (csrc/attn_bwd_fused_x6.hip; f32-grade results, dq unchanged): "1" whenever the call qualifies, "0" never, "auto" from
# ATTENTION_BWD_X6_MIN_SCORES scores (B*H*I*J) on.  Only the autograd path (stages=None) takes it: a caller that passes
# `stages` gets exactly those bits.
ATTENTION_BACKWARD_X6 = os.environ.get("AMK_ATTN_BWD_X6", "auto")
ATTENTION_BWD_X6_MIN_SCORES = 1 << 22


def _attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, key_mask, causal_mask, scale, stages=None, delta=None,
                   scores=None):
    auto_stages = stages is None
    if stages is None:
        det = DETERMINISTIC_ATTENTION_BACKWARD or torch.are_deterministic_algorithms_enabled()
        stages = ATTN_BWD_ALL if ATTENTION_BACKWARD_TWO_KERNEL else (ATTN_BWD_FAST_REPRO if det else ATTN_BWD_FAST)
    if stages & ATTN_BWD_FUSED and not stages & (ATTN_BWD_KEYS128 | ATTN_BWD_KEYS256):
        stages |= {128: ATTN_BWD_KEYS128, 256: ATTN_BWD_KEYS256}.get(ATTENTION_BACKWARD_KEYS, 0)
    if not stages & ATTN_BWD_FUSED:
        scores = None
    B, H, I, D = q.shape
    if D != 64 and stages & ATTN_BWD_DQ_REPRO:
        scores = None   # head dims other than 64 under the reproducible mode: the two recompute kernels (no kept scores)
    J = k.shape[2]
    if ATTENTION_BACKWARD_X6 not in ("auto", "0", "1"):
        raise RuntimeError(f"ops.ATTENTION_BACKWARD_X6 must be auto, 0 or 1 (got {ATTENTION_BACKWARD_X6!r})")
    keys256 = bool(stages & ATTN_BWD_KEYS256) or (not stages & ATTN_BWD_KEYS128 and J >= 256)
    if (auto_stages and scores is not None and D == 64 and keys256 and dq.stride() == (I * H * D, D, H * D, 1)
            and (ATTENTION_BACKWARD_X6 == "1"
                 or (ATTENTION_BACKWARD_X6 == "auto" and B * H * I * J >= ATTENTION_BWD_X6_MIN_SCORES))):
        stages |= ATTN_BWD_X6
    d_o = _as_kernel_view(d_o)
    L = _lib.load()
    need = L.amk_attn_bwd_ws_floats(B, H, I, J, int(stages))
    if delta is None or delta.numel() < need:
        delta = torch.empty((need,), device=q.device, dtype=torch.float32)

    def call(st):
        kept = scores is not None and st & ATTN_BWD_FUSED
        fn, head = (L.amk_attn_bwd_kept, (_ptr(scores),)) if kept else (L.amk_attn_bwd, ())
        rc = fn(
            *head, _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(stats), _ptr(d_o),
            _ptr(dq), _ptr(dk), _ptr(dv), _ptr(delta), _ptr(key_mask), _ptr(causal_mask),
            B, H, I, J, D,
            *_strides4(q), *_strides4(k), *_strides4(v), *_strides4(o), *_strides4(d_o),
            *_strides4(dq), *_strides4(dk), *_strides4(dv),
            float(scale), int(st), _stream(),
        )
        _lib.check(rc, "amk_attn_bwd")

    if KERNEL_EVENTS is not None and (stages & ATTN_BWD_DELTA) and (stages & ~ATTN_BWD_DELTA):
        call(ATTN_BWD_DELTA)  # delta on its own so that the events bracket the main kernel(s) only
        name = "attn_bwd_dkdv+dq" if not stages & ATTN_BWD_FUSED else (
            "attn_bwd_fused_kernel(kept scores)" if scores is not None else "attn_bwd_fused_kernel")
        with _timed(name):
            call(stages & ~ATTN_BWD_DELTA)
    else:
        call(stages)


# Mixed precision (the reference's shipped config trains under accelerate's bf16 autocast, cfg/vitvqgan.yaml:73): the
# kernels here are f32, so inside a torch.autocast region every autograd Function below takes its floating-point
# inputs as f32 (custom_fwd(cast_inputs=float32): bf16 activations coming out of autocast Linear layers are upcast,
# the op runs with autocast off) and hands f32 back; the library GEMMs around them run in bf16 as autocast decides.
_amp_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_amp_bwd = torch.amp.custom_bwd(device_type="cuda")


class _AttnCore(torch.autograd.Function):
    """o = softmax(fill(q*scale @ k^T)) @ v on (B,H,T,D) views."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, q, k, v, key_mask, causal_mask, scale):
        need = any(ctx.needs_input_grad[:3])
        q, k, v, o, stats, scores = _attn_forward(q, k, v, key_mask, causal_mask, scale, keep_scores=need, auto_x6=True)
        ctx.save_for_backward(q, k, v, o, stats, key_mask, causal_mask, scores)
        ctx.scale = scale
        return o

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, d_o):
        q, k, v, o, stats, key_mask, causal_mask, scores = ctx.saved_tensors
        B, H, I, D = q.shape
        J = k.shape[2]
        dq = _new_bthd(B, H, I, D, q)
        dk = _new_bthd(B, H, J, D, q)
        dv = _new_bthd(B, H, J, D, q)
        _attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, key_mask, causal_mask, ctx.scale, scores=scores)
        return dq, dk, dv, None, None, None


class _AttnFusedKV(torch.autograd.Function):
    """Same core fed by the projection outputs in place: q (B,I,h*d), kv (B,J,2*h*d) with the
    reference's '(kv h d)' column order (models/softmax_attention.py:39); returns (B,I,h*d).
    The backward writes dk and dv straight into one (B,J,2*h*d) buffer."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, q2, kv2, key_mask, causal_mask, H, D, scale):
        B, I, _ = q2.shape
        J = kv2.shape[1]
        q2 = q2.contiguous()
        kv2 = kv2.contiguous()
        q = q2.view(B, I, H, D).permute(0, 2, 1, 3)
        kv = kv2.view(B, J, 2, H, D)
        k = kv[:, :, 0].permute(0, 2, 1, 3)
        v = kv[:, :, 1].permute(0, 2, 1, 3)
        need = any(ctx.needs_input_grad[:2])
        q, k, v, o, stats, scores = _attn_forward(q, k, v, key_mask, causal_mask, scale, keep_scores=need, auto_x6=True)
        ctx.save_for_backward(q, k, v, o, stats, key_mask, causal_mask, scores)
        ctx.scale = scale
        return o.permute(0, 2, 1, 3).reshape(B, I, H * D)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, d_o2):
        q, k, v, o, stats, key_mask, causal_mask, scores = ctx.saved_tensors
        B, H, I, D = q.shape
        J = k.shape[2]
        d_o = d_o2.contiguous().view(B, I, H, D).permute(0, 2, 1, 3)
        dq2 = torch.empty((B, I, H * D), device=q.device, dtype=torch.float32)
        dkv2 = torch.empty((B, J, 2 * H * D), device=q.device, dtype=torch.float32)
        dq = dq2.view(B, I, H, D).permute(0, 2, 1, 3)
        dkv = dkv2.view(B, J, 2, H, D)
        dk = dkv[:, :, 0].permute(0, 2, 1, 3)
        dv = dkv[:, :, 1].permute(0, 2, 1, 3)
        _attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, key_mask, causal_mask, ctx.scale, scores=scores)
        return dq2, dkv2, None, None, None, None, None


# Mixed precision (the reference's shipped bf16 autocast): with bf16 projections coming in and head dim 64 the core runs
# on the bf16-MFMA kernels of csrc/attn_bf16.hip (bf16 q / k / v / o and gradients, f32 scores, softmax and statistics),
# with or without key-padding / causal masks; AMK_ATTENTION_BF16=0 keeps the round-2 behaviour (inputs upcast, exact-f32
# kernels).
ATTENTION_BF16 = os.environ.get("AMK_ATTENTION_BF16", "1") == "1"


def _parse_bf16_dims(text):
    """AMK_ATTENTION_BF16_DIMS: a comma list out of 32, 64, 128 -> frozenset of ints."""
    dims = set()
    for part in text.split(","):
        part = part.strip()
        if part not in ("32", "64", "128"):
            raise ValueError(f"AMK_ATTENTION_BF16_DIMS={text!r}: a comma list out of 32, 64, 128 (got {part!r})")
        dims.add(int(part))
    return frozenset(dims)


# Head dims whose bf16 projections take the bf16-MFMA core under ATTENTION_BF16: 64 on csrc/attn_bf16.hip, 32 and 128 on
# csrc/attn_bf16_hd.hip (opt-in: AMK_ATTENTION_BF16_DIMS=32,64,128).  A head dim outside the set takes the exact-f32
# kernels on upcast inputs.  Read once per process.
ATTENTION_BF16_DIMS = _parse_bf16_dims(os.environ.get("AMK_ATTENTION_BF16_DIMS", "64"))


class _AttnFusedKVBF16(torch.autograd.Function):
    """_AttnFusedKV on bf16 tensors: q2 (B,I,h*d), kv2 (B,J,2*h*d) bf16 -> (B,I,h*d) bf16.  dim_head 64 (the default)
    runs on amk_attn_bf16_fwd / _bwd, 32 and 128 on amk_attn_bf16_hd_fwd / _bwd."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, q2, kv2, H, scale, key_mask=None, causal_mask=None, dim_head=64):
        """key_mask: uint8 (B, J), 1 = keep; causal_mask: uint8 (I, J), 1 = masked (see _mask_u8); or None."""
        B, I, _ = q2.shape
        J = kv2.shape[1]
        D = int(dim_head)
        if D not in (32, 64, 128) or q2.shape[2] != H * D or kv2.shape[2] != 2 * H * D:
            raise RuntimeError(f"bf16 attention: q {tuple(q2.shape)} / kv {tuple(kv2.shape)} do not fit heads={H}, "
                               f"dim_head={D} (dim_head 32, 64 or 128)")
        hd = "_hd" if D != 64 else ""
        q2 = q2.contiguous()
        kv2 = kv2.contiguous()
        o2 = torch.empty((B, I, H * D), device=q2.device, dtype=torch.bfloat16)
        stats = torch.empty((B, H, I, 2), device=q2.device, dtype=torch.float32)
        L = _lib.load()
        qs, kvs = (I * H * D, H * D, D), (J * 2 * H * D, 2 * H * D, D)
        masked = key_mask is not None or causal_mask is not None
        fwd = L.amk_attn_bf16_hd_fwd if hd else L.amk_attn_bf16_fwd
        with _timed(f"attn_bf16{hd}_fwd_kernel<masked>" if masked else f"attn_bf16{hd}_fwd_kernel"):
            rc = fwd(_ptr(q2), _ptr(kv2), ctypes.c_void_p(kv2.data_ptr() + 2 * H * D), _ptr(o2), _ptr(stats),
                     _ptr(key_mask), _ptr(causal_mask),
                     B, H, I, J, D, *qs, *kvs, *kvs, *qs, float(scale), _stream())
        _lib.check(rc, f"amk_attn_bf16{hd}_fwd")
        ctx.save_for_backward(q2, kv2, o2, stats, key_mask, causal_mask)
        ctx.cfg = (H, scale, D)
        return o2

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, d_o2):
        q2, kv2, o2, stats, key_mask, causal_mask = ctx.saved_tensors
        H, scale, D = ctx.cfg
        B, I, _ = q2.shape
        J = kv2.shape[1]
        hd = "_hd" if D != 64 else ""
        d_o2 = d_o2.to(torch.bfloat16).contiguous()
        dq2 = torch.empty_like(q2)
        dkv2 = torch.empty_like(kv2)
        L = _lib.load()
        ws_floats = L.amk_attn_bf16_hd_bwd_ws_floats(B, H, I, J, D) if hd else L.amk_attn_bf16_bwd_ws_floats(B, H, I, J)
        ws = torch.empty((ws_floats,), device=q2.device, dtype=torch.float32)
        qs, kvs = (I * H * D, H * D, D), (J * 2 * H * D, 2 * H * D, D)
        masked = key_mask is not None or causal_mask is not None
        bwd = L.amk_attn_bf16_hd_bwd if hd else L.amk_attn_bf16_bwd
        with _timed(f"attn_bf16{hd}_bwd_kernel<masked>" if masked else f"attn_bf16{hd}_bwd_kernel"):
            rc = bwd(_ptr(q2), _ptr(kv2), ctypes.c_void_p(kv2.data_ptr() + 2 * H * D), _ptr(o2), _ptr(stats), _ptr(d_o2),
                     _ptr(dq2), _ptr(dkv2), ctypes.c_void_p(dkv2.data_ptr() + 2 * H * D), _ptr(ws),
                     _ptr(key_mask), _ptr(causal_mask),
                     B, H, I, J, D, *qs, *kvs, *kvs, *qs, *qs, *qs, *kvs, *kvs, float(scale), _stream())
        _lib.check(rc, f"amk_attn_bf16{hd}_bwd")
        return dq2, dkv2, None, None, None, None, None


def attention(q, k, v, scale, key_mask=None, causal_mask=None):
    """Fused attention core on (B,H,T,D) tensors (any strides with a contiguous last axis).

    key_mask: bool (B,J), True = keep (reference ``context_mask``); causal_mask: bool (I,J),
    True = masked (reference ``causal_mask``); both filled with -1e9 as masked_fill does.
    """
    B, H, I, D = q.shape
    J = k.shape[2]
    km = _mask_u8(key_mask, (B, J), "context_mask")
    cm = _mask_u8(causal_mask, (I, J), "causal_mask")
    return _AttnCore.apply(q, k, v, km, cm, scale)


def attention_fused_kv(q2, kv2, num_heads, dim_head, scale, key_mask=None, causal_mask=None):
    """q2 (B,I,h*d), kv2 (B,J,2*h*d) -> (B,I,h*d); see _AttnFusedKV."""
    B, I, _ = q2.shape
    J = kv2.shape[1]
    km = _mask_u8(key_mask, (B, J), "context_mask")
    cm = _mask_u8(causal_mask, (I, J), "causal_mask")
    if ATTENTION_BF16 and q2.dtype == torch.bfloat16 and kv2.dtype == torch.bfloat16 and q2.is_cuda and dim_head in ATTENTION_BF16_DIMS:
        return _AttnFusedKVBF16.apply(q2, kv2, num_heads, scale, km, cm, dim_head)
    return _AttnFusedKV.apply(q2, kv2, km, cm, num_heads, dim_head, scale)


def attention_decode(q2, kv_new2, cache, n_dev, num_heads, dim_head, scale, key_mask=None, ws=None):
    """One new query row per (batch, head) against a key / value cache (csrc/attn_decode.hip), inference only.

    q2 (B, 1, h*d); cache (B, capacity, 2*h*d) in the kv projection's '(kv h d)' columns; n_dev: int32 device tensor
    holding the number of valid cache rows (the kernel reads it on the device, so a captured step replays for every
    position).  kv_new2 (B, 1, 2*h*d): append mode -- row n of the cache becomes kv_new2 and the query attends rows
    0 .. n.  kv_new2 None: read mode -- the query attends rows 0 .. n - 1, all `capacity` rows when n_dev is None.
    key_mask: bool / uint8 (B, capacity), True = keep.  Returns (B, 1, h*d) in the cache's dtype.

    The cache's dtype picks the kernel: float32 (amk_attn_decode) or bfloat16 (amk_attn_decode_bf16: f32 scores, softmax
    and sums on bf16 operands, the output rounded once); q2 and kv_new2 must have the cache's dtype.  Inside or outside
    autocast alike -- the call casts nothing.  The cache is consumed in place and must be contiguous; q2 and kv_new2 are
    consumed in place too and may be column slices of one projection output: unit last stride, the row stride and the
    offset multiples of 4 elements (f32) or 8 (bf16).  ws: a float32 workspace of at least
    attention_decode_ws_floats(B, h, d, capacity) elements to reuse across calls (DecoderState keeps one); None
    allocates one."""
    if any(t is not None and t.requires_grad for t in (q2, kv_new2, cache)):
        raise RuntimeError("attention_decode is inference only: it has no backward; call it under torch.no_grad() "
                           "on tensors that do not require grad")
    if cache.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"attention_decode runs on a float32 or a bfloat16 cache; got {cache.dtype}")
    for t in (q2, kv_new2, cache):
        if t is not None and not t.is_cuda:
            raise RuntimeError("amk ops run only on MI355X (HIP) tensors; got a CPU tensor. There is no CPU fallback.")
    if q2.dtype != cache.dtype or (kv_new2 is not None and kv_new2.dtype != cache.dtype):
        raise RuntimeError(f"attention_decode: q ({q2.dtype}) and kv_new ({None if kv_new2 is None else kv_new2.dtype}) "
                           f"must have the cache's dtype ({cache.dtype})")
    b16 = cache.dtype == torch.bfloat16
    H, D = int(num_heads), int(dim_head)
    B, capacity = cache.shape[0], cache.shape[1]
    hd = H * D
    if tuple(q2.shape) != (B, 1, hd) or cache.dim() != 3 or cache.shape[2] != 2 * hd or not cache.is_contiguous():
        raise RuntimeError(f"attention_decode: q {tuple(q2.shape)} / cache {tuple(cache.shape)} do not fit "
                           f"B={B}, heads={H}, dim_head={D} (q (B, 1, h*d); cache: contiguous (B, capacity, 2*h*d))")
    if kv_new2 is not None and tuple(kv_new2.shape) != (B, 1, 2 * hd):
        raise RuntimeError(f"attention_decode: kv_new {tuple(kv_new2.shape)} is not one (kv h d) row per batch")
    if n_dev is not None and (n_dev.dtype != torch.int32 or not n_dev.is_cuda or n_dev.numel() != 1):
        raise RuntimeError("attention_decode: n_dev must be a one-element int32 device tensor")
    if kv_new2 is not None and n_dev is None:
        raise RuntimeError("attention_decode: append mode needs n_dev")
    unit = 8 if b16 else 4
    for t, what in ((q2, "q"), (kv_new2, "kv_new")):
        if t is not None and (t.stride(2) != 1 or (B > 1 and t.stride(0) % unit) or t.data_ptr() % 16):
            raise RuntimeError(f"attention_decode consumes {what} in place: unit last stride, a row stride that is a multiple "
                               f"of {unit} elements and a 16-byte aligned start (a contiguous tensor or a column slice of one)")
    km = _mask_u8(key_mask, (B, capacity), "key_mask")
    L = _lib.load()
    o = torch.empty((B, 1, hd), device=q2.device, dtype=cache.dtype)
    need = L.amk_attn_decode_ws_floats(B, H, D, capacity)
    if ws is None:
        ws = torch.empty((need,), device=q2.device, dtype=torch.float32)
    elif ws.dtype != torch.float32 or not ws.is_cuda or not ws.is_contiguous() or ws.numel() < need:
        raise RuntimeError(f"attention_decode: ws must be a contiguous float32 device tensor of at least {need} elements")
    esz = 2 if b16 else 4
    q_sb = q2.stride(0) if B > 1 else hd
    n_sb = (kv_new2.stride(0) if B > 1 else 2 * hd) if kv_new2 is not None else 2 * hd
    fn, name = (L.amk_attn_decode_bf16, "amk_attn_decode_bf16") if b16 else (L.amk_attn_decode, "amk_attn_decode")
    with _timed("attn_decode"):
        rc = fn(_ptr(q2), _ptr(kv_new2), ctypes.c_void_p(kv_new2.data_ptr() + esz * hd) if kv_new2 is not None else _NULL,
                _ptr(cache), ctypes.c_void_p(cache.data_ptr() + esz * hd), _ptr(o), _ptr(ws), _ptr(n_dev), _ptr(km),
                B, H, D, capacity, q_sb, D, n_sb, D, capacity * 2 * hd, 2 * hd, D, hd, D,
                float(scale), _stream())
    _lib.check(rc, name)
    return o


def attention_decode_ws_floats(B, num_heads, dim_head, capacity):
    """Elements of the float32 workspace attention_decode needs at these sizes (amk_attn_decode_ws_floats)."""
    return int(_lib.load().amk_attn_decode_ws_floats(int(B), int(num_heads), int(dim_head), int(capacity)))


def attention_prefill(q2, kv_new2, cache, n_dev, num_heads, dim_head, scale, key_mask=None, ws=None):
    """n new query rows per (batch, head) against a key / value cache in one pass (csrc/attn_prefill.hip), inference
    only: the n-row twin of attention_decode, for a decode that starts from tokens the caller already has.

    q2 (B, n, h*d); cache (B, capacity, 2*h*d); n_dev: int32 device tensor holding p0, the number of valid cache rows.
    kv_new2 (B, n, 2*h*d): append mode -- cache rows p0 .. p0 + n - 1 become kv_new2 and row i attends rows 0 .. p0 + i
    (the causal mask's rows, from indices: no mask tensor).  kv_new2 None: read mode -- every row attends rows
    0 .. p0 - 1, all `capacity` rows when n_dev is None.  key_mask: bool / uint8 (B, capacity), True = keep.  Returns
    (B, n, h*d) in the cache's dtype.  Dtypes, strides, alignment and ws follow attention_decode (ws: at least
    attention_prefill_ws_floats(B, h, d, capacity, n) float32 elements; None allocates one).  Never captured: its grid
    depends on n."""
    if any(t is not None and t.requires_grad for t in (q2, kv_new2, cache)):
        raise RuntimeError("attention_prefill is inference only: it has no backward; call it under torch.no_grad() "
                           "on tensors that do not require grad")
    if cache.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"attention_prefill runs on a float32 or a bfloat16 cache; got {cache.dtype}")
    for t in (q2, kv_new2, cache):
        if t is not None and not t.is_cuda:
            raise RuntimeError("amk ops run only on MI355X (HIP) tensors; got a CPU tensor. There is no CPU fallback.")
    if q2.dtype != cache.dtype or (kv_new2 is not None and kv_new2.dtype != cache.dtype):
        raise RuntimeError(f"attention_prefill: q ({q2.dtype}) and kv_new ({None if kv_new2 is None else kv_new2.dtype}) "
                           f"must have the cache's dtype ({cache.dtype})")
    b16 = cache.dtype == torch.bfloat16
    H, D = int(num_heads), int(dim_head)
    B, capacity = cache.shape[0], cache.shape[1]
    hd = H * D
    if (q2.dim() != 3 or q2.shape[0] != B or q2.shape[1] < 1 or q2.shape[2] != hd or cache.dim() != 3
            or cache.shape[2] != 2 * hd or not cache.is_contiguous()):
        raise RuntimeError(f"attention_prefill: q {tuple(q2.shape)} / cache {tuple(cache.shape)} do not fit "
                           f"B={B}, heads={H}, dim_head={D} (q (B, n >= 1, h*d); cache: contiguous (B, capacity, 2*h*d))")
    n = q2.shape[1]
    if kv_new2 is not None and tuple(kv_new2.shape) != (B, n, 2 * hd):
        raise RuntimeError(f"attention_prefill: kv_new {tuple(kv_new2.shape)} is not n={n} (kv h d) rows per batch")
    if n_dev is not None and (n_dev.dtype != torch.int32 or not n_dev.is_cuda or n_dev.numel() != 1):
        raise RuntimeError("attention_prefill: n_dev must be a one-element int32 device tensor")
    if kv_new2 is not None and n_dev is None:
        raise RuntimeError("attention_prefill: append mode needs n_dev")
    unit = 8 if b16 else 4
    for t, what in ((q2, "q"), (kv_new2, "kv_new")):
        if t is not None and (t.stride(2) != 1 or (B > 1 and t.stride(0) % unit) or (n > 1 and t.stride(1) % unit)
                              or t.data_ptr() % 16):
            raise RuntimeError(f"attention_prefill consumes {what} in place: unit last stride, row strides that are multiples "
                               f"of {unit} elements and a 16-byte aligned start (a contiguous tensor or a column slice of one)")
    km = _mask_u8(key_mask, (B, capacity), "key_mask")
    L = _lib.load()
    o = torch.empty((B, n, hd), device=q2.device, dtype=cache.dtype)
    need = L.amk_attn_prefill_ws_floats(B, H, D, capacity, n)
    if ws is None:
        ws = torch.empty((need,), device=q2.device, dtype=torch.float32)
    elif ws.dtype != torch.float32 or not ws.is_cuda or not ws.is_contiguous() or ws.numel() < need:
        raise RuntimeError(f"attention_prefill: ws must be a contiguous float32 device tensor of at least {need} elements")
    esz = 2 if b16 else 4

    def strides(t, width):   # (sb, st) of a (B, n, width) tensor; a size-1 axis may carry any stride
        if t is None:
            return n * width, width
        st = t.stride(1) if n > 1 else width
        return (t.stride(0) if B > 1 else n * st), st

    q_sb, q_st = strides(q2, hd)
    n_sb, n_st = strides(kv_new2, 2 * hd)
    fn, name = (L.amk_attn_prefill_bf16, "amk_attn_prefill_bf16") if b16 else (L.amk_attn_prefill, "amk_attn_prefill")
    with _timed("attn_prefill"):
        rc = fn(_ptr(q2), _ptr(kv_new2), ctypes.c_void_p(kv_new2.data_ptr() + esz * hd) if kv_new2 is not None else _NULL,
                _ptr(cache), ctypes.c_void_p(cache.data_ptr() + esz * hd), _ptr(o), _ptr(ws), _ptr(n_dev), _ptr(km),
                B, H, D, capacity, n, q_sb, q_st, D, n_sb, n_st, D, capacity * 2 * hd, 2 * hd, D, n * hd, hd, D,
                float(scale), _stream())
    _lib.check(rc, name)
    return o


def attention_prefill_ws_floats(B, num_heads, dim_head, capacity, n):
    """Elements of the float32 workspace attention_prefill needs at these sizes (amk_attn_prefill_ws_floats)."""
    return int(_lib.load().amk_attn_prefill_ws_floats(int(B), int(num_heads), int(dim_head), int(capacity), int(n)))


# AMK_DECODE_BF16 (default 1): under bf16 autocast Decoder.init_state builds a bf16 decode state -- bf16 caches, the state's
# own bf16 weight copies, the step on amk_attn_decode_bf16 and amk_gemm_rows_bf16 (models/transformer.py).  0: the decode
# refuses to run under autocast, as it did before that path existed.  Read once per process.
DECODE_BF16 = os.environ.get("AMK_DECODE_BF16", "1") != "0"
DECODE_AUTOCAST_REFUSAL = ("attention_decode runs on f32 tensors outside autocast; a bf16 cache is not implemented "
                           "with AMK_DECODE_BF16=0 (an f32 decode state does not run under autocast)")


def empty_w16(rows, k, device):
    """A zeroed bf16 (rows, k) matrix whose row stride is a multiple of 8 elements, as the row GEMM takes it."""
    return torch.zeros((rows, (k + 7) // 8 * 8), device=device, dtype=torch.bfloat16)[:, :k]


def fill_w16(dst, param):
    """dst (bf16, in place) <- the parameter: its bf16 shadow where FlatAdam(bf16_shadow=True) keeps one current, else
    the f32 master rounded to nearest even."""
    shadow = getattr(param, "_amk_bf16", None)
    current = shadow is not None and param._version == param._amk_bf16_version
    dst.copy_(shadow if current else param.detach())


def layer_norm_to_bf16(x, res, gamma, beta, eps=1e-5):
    """(h, y): h = x + res in f32 (x itself with res None), y = LayerNorm(h) written in bf16 (amk_add_layernorm_mixed_fwd);
    x f32 or bf16, res f32 or None.  For callers that have autocast disabled and feed y to bf16 products."""
    if not _ln_supported(x.shape[-1]):
        raise RuntimeError(f"layer_norm_to_bf16: width {x.shape[-1]} not supported (a multiple of 4 up to 4096)")
    return _AddLayerNormMixed.apply(x, res, gamma, beta, eps)


# rows up to which linear_rows takes the row GEMM; above it the library's bf16 GEMM (F.linear) on the same operands
ROWS_GEMM_MAX_M = 64


def linear_rows_bf16(x16, w16, bias32=None, out_dtype=torch.bfloat16):
    """x16 (M, K) . w16 (N, K)^T + bias32 on amk_gemm_rows_bf16 (csrc/gemm_rows_bf16.hip): bf16 operands with unit column
    stride and row strides that are multiples of 8, an f32 bias added in f32, f32 accumulation; out_dtype float32, or
    bfloat16 rounded once.  Built for M of a decode batch: row m of the result is bitwise independent of M.  Inference
    only, no autograd."""
    if x16.dtype != torch.bfloat16 or w16.dtype != torch.bfloat16 or x16.dim() != 2 or w16.dim() != 2:
        raise RuntimeError(f"linear_rows_bf16 takes bf16 matrices; got {x16.dtype} {tuple(x16.shape)}, {w16.dtype} {tuple(w16.shape)}")
    if not x16.is_cuda or not w16.is_cuda:
        raise RuntimeError("amk ops run only on MI355X (HIP) tensors; got a CPU tensor. There is no CPU fallback.")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"linear_rows_bf16 writes float32 or bfloat16, not {out_dtype}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x16, w16, bias32)):
        raise RuntimeError("linear_rows_bf16 is inference only: it has no backward; call it under torch.no_grad()")
    M, K = x16.shape
    N = w16.shape[0]
    if w16.shape[1] != K or (bias32 is not None and (bias32.dtype != torch.float32 or tuple(bias32.shape) != (N,)
                                                     or not bias32.is_contiguous())):
        raise RuntimeError(f"linear_rows_bf16: x {tuple(x16.shape)}, w {tuple(w16.shape)} and an f32 bias (N,) do not fit")
    if x16.stride(1) != 1 or (M > 1 and x16.stride(0) % 8) or x16.data_ptr() % 16:
        x16 = _rows_padded(x16)
    if w16.stride(1) != 1 or (N > 1 and w16.stride(0) % 8) or w16.data_ptr() % 16:
        w16 = _rows_padded(w16)
    ldx = x16.stride(0) if M > 1 else (K + 7) // 8 * 8
    ldw = w16.stride(0) if N > 1 else (K + 7) // 8 * 8
    ldy = (N + 3) // 4 * 4
    y = torch.empty((M, ldy), device=x16.device, dtype=out_dtype)
    with _timed(f"gemm_rows_bf16 N{N} K{K}"):
        rc = _lib.load().amk_gemm_rows_bf16(_ptr(x16), ldx, _ptr(w16), ldw, _ptr(bias32), _ptr(y), ldy, M, N, K,
                                            1 if out_dtype == torch.bfloat16 else 0, _stream())
    _lib.check(rc, "amk_gemm_rows_bf16")
    return y if ldy == N else y[:, :N]


def _rows_padded(t):
    """A copy of a bf16 matrix with its rows at a stride that is a multiple of 8 elements (a view of the padded buffer)."""
    r, k = t.shape
    buf = torch.zeros((r, (k + 7) // 8 * 8), device=t.device, dtype=t.dtype)
    buf[:, :k].copy_(t)
    return buf[:, :k]


def linear_rows(x16, w16, bias32=None, out_dtype=torch.bfloat16, w32=None):
    """The decode step's Linear on bf16 weights: the row GEMM up to ROWS_GEMM_MAX_M rows, above it F.linear on the same
    bf16 operands (with an f32 result -- the head -- on the f32 master w32)."""
    if x16.shape[0] <= ROWS_GEMM_MAX_M:
        return linear_rows_bf16(x16, w16, bias32, out_dtype)
    if out_dtype == torch.float32 and w32 is not None:
        return torch.nn.functional.linear(x16.float(), w32, bias32)
    y = torch.nn.functional.linear(x16, w16, None if bias32 is None else bias32.to(torch.bfloat16))
    return y if out_dtype == torch.bfloat16 else y.float()


# ---------------------------------------------------------------------------- VQ lookup
# vq_gather (indices_to_embeddings) takes indices from the caller: an index outside the codebook is never
# dereferenced by the kernel, and with CHECK_INDICES the call raises IndexError like nn.Embedding does -- at
# the price of one device-to-host read.  Set False (AMK_CHECK_INDICES=0) inside HIP-graph capture.
CHECK_INDICES = os.environ.get("AMK_CHECK_INDICES", "1") == "1"


def vq_nsplit(N, K):
    """Codebook slices per row block.  The sweep kernel keeps 4 workgroups per CU resident and hides
    its LDS latency behind the other workgroups' MFMAs, so it wants >= 16 workgroups per CU
    (measured at N = 32768, K = 8192: 1 slice 0.545 of the f32 MFMA peak, 2: 0.591, 4: 0.626, 8: 0.642),
    with slices no shorter than 1024 codes (at N = 8192 sixteen slices of 512 lose to eight of 1024)."""
    row_blocks = (N + 127) // 128
    nsplit = 1
    while row_blocks * nsplit < 4096 and K // (2 * nsplit) >= 1024:
        nsplit *= 2
    return nsplit


class _VQLookup(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, z, codebook, beta):
        _require_device(z, codebook)
        C = z.shape[-1]
        K = codebook.shape[0]
        zf = z.contiguous().view(-1, C)
        cb = codebook.contiguous()
        N = zf.shape[0]
        dev = z.device
        L = _lib.load()
        nsplit = vq_nsplit(N, K)
        f32 = dict(device=dev, dtype=torch.float32)
        kp = L.amk_vq_padded_codes(K, nsplit)  # any K: the normalised copy is padded to whole tiles per slice
        en = torch.empty((kp, C), **f32)
        ee = torch.empty((kp,), **f32)
        pmin = torch.empty((N, nsplit), **f32)
        pidx = torch.empty((N, nsplit), device=dev, dtype=torch.int32)
        idx = torch.empty((N,), device=dev, dtype=torch.int64)
        out = torch.empty((N, C), **f32)
        zq = torch.empty((N, C), **f32)
        zn = torch.empty((N, C), **f32)
        partial = torch.empty((L.amk_vq_num_partials(N),), **f32)
        with _timed("vq_lookup_fwd"):
            rc = L.amk_vq_lookup_fwd(
                _ptr(zf), _ptr(cb), N, K, C, nsplit, _ptr(en), _ptr(ee), _ptr(pmin), _ptr(pidx),
                _ptr(idx), _ptr(out), _ptr(zq), _ptr(zn), _ptr(partial), _stream(),
            )
        _lib.check(rc, "amk_vq_lookup_fwd")
        mean_sq = partial.sum() / float(N * C)
        # beta*mean((zq.detach()-z)^2) + mean((zq-z.detach())^2): the two means are one value
        loss = beta * mean_sq + mean_sq
        ctx.save_for_backward(zf, cb, zn, zq, idx)
        ctx.beta = beta
        ctx.z_shape = z.shape
        idx_v = idx.view(z.shape[:-1])
        ctx.mark_non_differentiable(idx_v)
        return out.view(z.shape), idx_v, loss

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, g_out, _g_idx, g_loss):
        zf, cb, zn, zq, idx = ctx.saved_tensors
        N, C = zf.shape
        K = cb.shape[0]
        if g_out is None:
            g_out = torch.zeros_like(zf)
        if g_loss is None:
            g_loss = torch.zeros((), device=zf.device, dtype=torch.float32)
        g_out = g_out.contiguous().view(N, C)
        g_loss = g_loss.contiguous().to(torch.float32)
        dz = torch.empty_like(zf)
        L = _lib.load()
        if DETERMINISTIC_ATTENTION_BACKWARD or torch.are_deterministic_algorithms_enabled():
            # reproducible codebook gradient: per-row contributions, added in a fixed order instead of the kernel's
            # f32 atomics
            ge = torch.empty_like(zf)
            rc = L.amk_vq_lookup_bwd_rows(
                _ptr(zf), _ptr(cb), _ptr(zn), _ptr(zq), _ptr(idx), _ptr(g_out), _ptr(g_loss),
                float(ctx.beta), N, K, C, _ptr(dz), _ptr(ge), _stream(),
            )
            _lib.check(rc, "amk_vq_lookup_bwd_rows")
            # ordered sum per code without touching torch's global determinism switches: rows sorted by code
            # (stable: equal codes keep their row order), then one sequential sum per segment
            flat_idx = idx.clamp(0, K - 1)
            srt, order = torch.sort(flat_idx, stable=True)
            bounds = torch.searchsorted(srt, torch.arange(K + 1, device=srt.device, dtype=srt.dtype))
            dcb = torch.segment_reduce(ge.index_select(0, order), "sum", offsets=bounds, axis=0, unsafe=True)
            return dz.view(ctx.z_shape), dcb, None
        dcb = torch.empty_like(cb)
        rc = L.amk_vq_lookup_bwd(
            _ptr(zf), _ptr(cb), _ptr(zn), _ptr(zq), _ptr(idx), _ptr(g_out), _ptr(g_loss),
            float(ctx.beta), N, K, C, _ptr(dz), _ptr(dcb), _stream(),
        )
        _lib.check(rc, "amk_vq_lookup_bwd")
        return dz.view(ctx.z_shape), dcb, None


def vq_lookup(z, codebook, beta):
    """Codebook.forward of the reference: returns (z_q straight-through, int64 indices, loss)."""
    return _VQLookup.apply(z, codebook, beta)


def vq_gather(indices, codebook):
    """Codebook.indices_to_embeddings: l2norm(E[indices]).  Differentiable w.r.t. nothing
    (the reference only uses it for decoding under no_grad / frozen VQ)."""
    _require_device(indices, codebook)
    K, C = codebook.shape
    flat = indices.contiguous().view(-1).to(torch.int64)
    N = flat.shape[0]
    out = torch.empty((N, C), device=codebook.device, dtype=torch.float32)
    bad = torch.zeros((1,), device=codebook.device, dtype=torch.int32)
    L = _lib.load()
    rc = L.amk_vq_gather(_ptr(flat), _ptr(codebook.detach().contiguous()), N, K, C, _ptr(out), _ptr(bad), _stream())
    _lib.check(rc, "amk_vq_gather")
    if CHECK_INDICES and int(bad.item()):  # one host read per call; nn.Embedding raises here too
        raise IndexError(f"vq_gather: {int(bad.item())} of {N} indices are outside the codebook [0, {K})")
    return out.view(*indices.shape, C)


# ---------------------------------------------------------------------------- masked-token sampling step
_SAMPLE_CALLS = 0


def sample_step(logits, ids, mask=None, null_logits=None, cfg_scale=3.0, tau=1.0, p=0.9, gumbel=None, seed=None,
                unmasked_score=None, generator=None):
    """One step of the parallel decode on (B, T, V) logits, in one pass (csrc/sample.hip): classifier-free
    guidance, softmax, top-(1-p) filter, Gumbel-argmax at temperature tau, chosen probability.
    ids (B, T) int64 is updated IN PLACE where mask (B, T) bool is True (everywhere without a mask);
    returns scores (B, T).  gumbel: explicit noise (B, T, V) -- else drawn in-kernel: Philox4x32-10 keyed by the seed
    and stream offset of torch's CUDA generator (`generator`, default the device's), which is advanced by the call, so
    torch.manual_seed reproduces a run; an explicit `seed` uses this module's call counter as the offset instead.
    Ties at the keep-th largest logit: every logit >= that value is kept (the reference's topk keeps exactly k);
    -0.0 and +0.0 are one value there, as for torch.topk (the kernel stores the scaled logit as x + 0.0).
    In-kernel noise: word w of the stream gives u = ((w >> 9) + 0.5) 2^-23, strictly inside (0, 1), and
    g = -log(-log u), always finite."""
    import math

    global _SAMPLE_CALLS
    _require_device(logits, null_logits, gumbel)
    B, T, V = logits.shape
    logits = logits.contiguous()
    null_logits = null_logits.contiguous() if null_logits is not None else None
    gumbel = gumbel.contiguous() if gumbel is not None else None
    if ids.dtype != torch.int64 or not ids.is_contiguous():
        raise RuntimeError("sample_step: ids must be a contiguous int64 tensor (updated in place)")
    m8 = mask.to(torch.uint8).contiguous() if mask is not None else None
    scores = torch.empty((B, T), device=logits.device, dtype=torch.float32)
    if seed is not None:
        _SAMPLE_CALLS += 1          # explicit seed: the stream position is this module's call counter
        offset = _SAMPLE_CALLS
    else:
        # torch's generator for this device supplies the Philox key and stream position, and is advanced past what
        # this call consumes: torch.manual_seed(s); generate(); torch.manual_seed(s); generate() repeats the samples
        gen = generator if generator is not None else torch.cuda.default_generators[logits.device.index or 0]
        seed = int(gen.initial_seed()) & ((1 << 63) - 1)
        offset = int(gen.get_offset())
        gen.set_offset(offset + 4 * ((B * T * V + 3) // 4))
    L = _lib.load()
    rc = L.amk_sample_step(_ptr(logits), _ptr(null_logits), float(cfg_scale), _ptr(gumbel), seed, offset, float(tau),
                           B * T, V, math.ceil((1 - p) * V), _ptr(m8), -1.0 if unmasked_score is None else float(unmasked_score),
                           _ptr(ids), _ptr(scores), _stream())
    _lib.check(rc, "amk_sample_step")
    return scores


# ---------------------------------------------------------------------------- routed experts
def _i32(n, dev):
    return torch.empty((n,), device=dev, dtype=torch.int32)


def moe_route(logits2, k):
    """logits2 (U,E) -> dict(ids int64 (U,k), gate (U,k), offsets int32 (E+1), perm int32 (U*k))."""
    _require_device(logits2)
    U, E = logits2.shape
    dev = logits2.device
    ids = torch.empty((U, k), device=dev, dtype=torch.int64)
    gate = torch.empty((U, k), device=dev, dtype=torch.float32)
    L = _lib.load()
    counts, rank = _i32(E, dev), _i32(U * k, dev)
    blockhist = _i32(L.amk_moe_route_ws_ints(U, E, k), dev)
    offsets, perm = _i32(E + 1, dev), _i32(U * k, dev)
    rc = L.amk_moe_route(_ptr(logits2.contiguous()), U, E, k, _ptr(ids), _ptr(gate), _ptr(counts), _ptr(rank),
                         _ptr(blockhist), _ptr(offsets), _ptr(perm), _stream())
    _lib.check(rc, "amk_moe_route")
    return dict(ids=ids, gate=gate, offsets=offsets, perm=perm)


# Sums over the pairs of a row inside the expert GEMM (f32 atomics, amk_grouped_gemm_*_acc) instead of a (pairs, width)
# intermediate and an ordered pass over it.  OFF by default: measured at the ViTMoE SwitchHead layer (16 pairs per row,
# 68 M element adds) the atomics cost more than the 272 MB intermediate they remove -- output experts 0.237 ms against
# 0.131 + 0.065 ms, V experts' input gradient 0.246 against 0.140 + 0.065 -- and the ordered combine keeps the
# reference's accumulation order.  AMK_MOE_SUM_IN_GEMM=1 turns it on (never under the deterministic switches).
MOE_SUM_IN_GEMM = os.environ.get("AMK_MOE_SUM_IN_GEMM", "0") == "1"


# Where a row sums many pairs -- SwitchHead: 8 heads x top-2 = 16 pairs per token over 32 experts -- the sum over the pairs
# of (pair row) x (its expert's matrix) is one dense product of the per-expert sums of the pair rows, Z (G, E*d), with the
# stacked expert matrices (E*d, N): E/fan times the routed FLOPs, but no (pairs, N) intermediate to write and re-read
# (272 MB per launch at the ViTMoE layer).  Measured there: 0.147 + 0.074 ms (routed GEMM + combine) against
# ~0.17 ms (sums + dense GEMM), and 0.163 + 0.074 against ~0.155 for the V experts' input gradient.  The sums differ
# from the ordered combine in accumulation order only; both are reproducible.  AMK_MOE_DENSE_Z=0: the routed form.
MOE_DENSE_Z = os.environ.get("AMK_MOE_DENSE_Z", "1") != "0"


def _moe_dense_z(width, depth, fan, E):
    """width: output row length; depth: contraction length per pair; fan: pairs per output row; E experts."""
    return MOE_DENSE_Z and E <= 2 * fan and width >= 256 and width >= 4 * depth and depth % 4 == 0


class _MoeElem:
    """The element type of a Function's expert products: label prefix, dtype of the operands and of Z, and the names of its
    entry points, put together once.  Routing, combine and gate gradient are the f32 kernels for every element type."""

    def __init__(self, prefix, suffix, dtype, wgrad_db):
        self.prefix, self.dtype, self.f32 = prefix, dtype, dtype == torch.float32
        self.nt, self.nn, self.wgrad = (f"amk_grouped_gemm_{kind}{suffix}" for kind in ("nt", "nn", "wgrad"))
        self.wgrad_db = wgrad_db   # the weight gradient's entry point takes a bias gradient
        self.sums = "amk_moe_expert_sums" if self.f32 else "amk_moe_expert_sums_bf16"


_MOE_F32 = _MoeElem("", "", torch.float32, True)                     # csrc/moe.hip
_MOE_BF16 = _MoeElem("bf16_", "_bf16", torch.bfloat16, True)         # csrc/moe_bf16.hip, 256-output tiles (MoELayer)
_MOE_BF16_64 = _MoeElem("bf16_", "64_bf16", torch.bfloat16, False)   # its 64-output tiles (SwitchHead, d <= 64)


def _expert_sums(a2, a_div, ids, scale, G, fan, E, d, elem=_MOE_F32):
    """Z (G, E*d): per output row and expert, the (scaled) sum of the rows of a2 its pairs read.  scale: a pointer.  bf16
    elements: the same f32 sums rounded once into a bf16 Z; a2 f32 or bf16."""
    Z = torch.empty((G, E * d), device=a2.device, dtype=elem.dtype)
    fn = getattr(_lib.load(), elem.sums)
    with _timed(f"{elem.prefix}moe_expert_sums G{G} fan{fan} E{E} d{d}"):
        if elem.f32:
            rc = fn(_ptr(a2), a2.stride(0), a_div, _ptr(ids), scale, G, fan, E, d, _ptr(Z), _stream())
        else:
            rc = fn(_ptr(a2), int(a2.dtype == torch.bfloat16), a2.stride(0), a_div, _ptr(ids), scale, G, fan, E, d, _ptr(Z), _stream())
    _lib.check(rc, elem.sums)
    return Z


def _moe_sum_in_gemm(width, depth, fan):
    """width: output row length; depth: contraction length; fan: pairs per output row."""
    if not MOE_SUM_IN_GEMM or DETERMINISTIC_ATTENTION_BACKWARD or torch.are_deterministic_algorithms_enabled():
        return False
    return fan >= 4 and width >= 128 and depth % 32 == 0


_DISTINCT = " (distinct rows)"   # label of a launch on amk_moe_route_distinct's lists: it stands for `pairs` routed pairs


def _grouped(nn, elem, A, lda, a_div, W, vec, offsets, perm, P, pairs=None, note=""):
    """One expert product for ALL experts, f32 result: pair p reads row p // a_div of A (row stride lda) and the matrix W[e]
    (N, Kd) of its expert.  nt: Y (P, N) = row x W[e]^T + vec[e] (bias (E, N)); nn: Y (P, Kd) = vec[p] (scale (P,)) x row
    x W[e]; vec may be None."""
    E, N, Kd = W.shape
    name = elem.nn if nn else elem.nt
    Y = torch.empty((P, Kd if nn else N), device=A.device, dtype=torch.float32)
    with _timed(f"{elem.prefix}grouped_{'nn' if nn else 'nt'} P{pairs or P} N{N} K{Kd}{note}"):
        rc = getattr(_lib.load(), name)(_ptr(A), lda, a_div, _ptr(W), _ptr(vec), _ptr(offsets), _ptr(perm), P, E, N, Kd, _ptr(Y),
                                        _stream())
    _lib.check(rc, name)
    return Y


def _grouped_acc(nn, A, lda, a_div, W, vec, offsets, perm, P, y_div):
    """_grouped on f32 (the f32 kernels alone have the form) with the pairs p // y_div summed by f32 atomics in the GEMM's
    epilogue, into a zeroed (P // y_div, width) result."""
    E, N, Kd = W.shape
    kind = "nn" if nn else "nt"
    name = f"amk_grouped_gemm_{kind}_acc"
    Y = torch.zeros((P // y_div, Kd if nn else N), device=A.device, dtype=torch.float32)
    with _timed(f"grouped_{kind}_acc P{P} N{N} K{Kd}"):
        rc = getattr(_lib.load(), name)(_ptr(A), lda, a_div, _ptr(W), _ptr(vec), _ptr(offsets), _ptr(perm), P, E, N, Kd, _ptr(Y),
                                        y_div, _stream())
    _lib.check(rc, name)
    return Y


def _grouped_wgrad(elem, Gm, ldg, g_div, X, ldx, x_div, scale, offsets, perm, P, shape, has_bias=False, pairs=None, note=""):
    """(dW (E, N, Kd), db (E, N) or None), f32: per expert, the sum over its pairs of scale[p] x (Gm row p // g_div)^T x
    (X row p // x_div)."""
    E, N, Kd = shape
    dW = torch.empty((E, N, Kd), device=X.device, dtype=torch.float32)
    db = torch.empty((E, N), device=X.device, dtype=torch.float32) if has_bias else None
    fn = getattr(_lib.load(), elem.wgrad)
    with _timed(f"{elem.prefix}grouped_wgrad P{pairs or P} N{N} K{Kd}{note}"):
        if elem.wgrad_db:
            rc = fn(_ptr(Gm), ldg, g_div, _ptr(X), ldx, x_div, _ptr(scale), _ptr(offsets), _ptr(perm), P, E, N, Kd, _ptr(dW), _ptr(db),
                    _stream())
        else:
            rc = fn(_ptr(Gm), ldg, g_div, _ptr(X), ldx, x_div, _ptr(scale), _ptr(offsets), _ptr(perm), P, E, N, Kd, _ptr(dW), _stream())
    _lib.check(rc, elem.wgrad)
    return dW, db


def _combine(Y, ids, gate, G, outer, k):
    """out (G, N): row g is the sum of Y's rows of its outer*k pairs in ascending expert id, gated (gate (U, k)) or plain."""
    N = Y.shape[1]
    out = torch.empty((G, N), device=Y.device, dtype=torch.float32)
    _lib.check(_lib.load().amk_moe_combine(_ptr(Y), _ptr(ids), _ptr(gate), G, outer, k, N, _ptr(out), _stream()), "amk_moe_combine")
    return out


def _combine_rows(V, ids, gate, U, k, fan, E):
    """_combine over the distinct rows V (G*E, N): unit u's k pairs read the rows (u // (fan // k)) * E + e."""
    N = V.shape[1]
    out = torch.empty((U, N), device=V.device, dtype=torch.float32)
    _lib.check(_lib.load().amk_moe_combine_rows(_ptr(V), _ptr(ids), _ptr(gate), U, 1, k, N, fan, E, _ptr(out), _stream()),
               "amk_moe_combine_rows")
    return out


def _gate_grad(d_out, Y, ids, gate, k, E, g_div, fan=None):
    """dlogits (U, E) f32 from d_out (pair p's row p // g_div) and the pairs' outputs Y; fan: Y holds the distinct rows."""
    P, N = ids.numel(), Y.shape[1]
    dlogits = torch.empty((P // k, E), device=Y.device, dtype=torch.float32)
    L = _lib.load()
    if fan is None:
        _lib.check(L.amk_moe_gate_grad(_ptr(d_out), _ptr(Y), _ptr(ids), _ptr(gate), P, k, E, N, g_div, _ptr(dlogits), _stream()),
                   "amk_moe_gate_grad")
    else:
        _lib.check(L.amk_moe_gate_grad_rows(_ptr(d_out), _ptr(Y), _ptr(ids), _ptr(gate), P, k, E, N, g_div, fan, _ptr(dlogits),
                                            _stream()), "amk_moe_gate_grad_rows")
    return dlogits


def _done(ctx, elem, saved, cfg, out, ids):
    ctx.elem = elem
    ctx.save_for_backward(*saved)
    ctx.cfg = cfg
    ctx.mark_non_differentiable(ids)
    ctx.set_materialize_grads(False)   # no zero-filled "gradient" of the ids handed to backward
    return out, ids


def _routed_dims(x2, logits2, W, k, x_div, outer):
    U = logits2.shape[0]
    if x2.shape != (U * k // x_div, W.shape[2]) or U % outer:
        raise RuntimeError(f"routed linear shapes disagree: x {tuple(x2.shape)} U {U} k {k} x_div {x_div} W {tuple(W.shape)}")


def _routed_fwd(ctx, elem, x, logits32, W, bias, k, x_div, weighted, outer, dtypes):
    """x (rows, Kd) and W (E, N, Kd) in elem's dtype, f32 logits and bias; dtypes: those of the caller's x and logits."""
    U, E = logits32.shape
    N, Kd = W.shape[1], W.shape[2]
    P, G, fan = U * k, U // outer, outer * k
    f32 = elem.f32   # the bf16 kernels have the routed form alone
    ldx = Kd if f32 else x.stride(0)
    with _timed(f"moe_route U{U} E{E} k{k}"):
        r = moe_route(logits32, k)
    Y = None
    if f32 and not weighted and bias is None and _moe_dense_z(N, Kd, fan, E):
        Z = _expert_sums(x, x_div, r["ids"], _NULL, G, fan, E, Kd)
        with _timed(f"dense_z_gemm M{G} N{N} K{E * Kd}"):
            out = Z @ W.permute(0, 2, 1).reshape(E * Kd, N)   # (E, N, Kd) -> (E*Kd, N): an 8 MB copy at the ViTMoE layer
    elif f32 and not weighted and _moe_sum_in_gemm(N, Kd, fan):
        # un-weighted sum over the pairs of an output row (SwitchHead's output experts): folded into the GEMM's
        # epilogue -- the (P, N) per-pair intermediate (272 MB at the ViTMoE layer) is never written
        out = _grouped_acc(False, x, ldx, x_div, W, bias, r["offsets"], r["perm"], P, fan)
    else:
        Y = _grouped(False, elem, x, ldx, x_div, W, bias, r["offsets"], r["perm"], P)
        out = torch.empty((G, N), device=x.device, dtype=torch.float32)
        with _timed(f"moe_combine G{G} N{N} x{fan}"):   # (the forward's combine has a label, so not _combine)
            rc = _lib.load().amk_moe_combine(_ptr(Y), _ptr(r["ids"]), _ptr(r["gate"] if weighted else None), G, outer, k, N,
                                             _ptr(out), _stream())
        _lib.check(rc, "amk_moe_combine")
    return _done(ctx, elem, (x, W, Y, r["ids"], r["gate"], r["offsets"], r["perm"]),
                 (k, x_div, weighted, outer, E, bias is not None) + dtypes, out, r["ids"])


def _routed_bwd(ctx, d_out):
    """(dx, dlogits, dW, db); the bf16 kernels have the routed form of dx alone."""
    elem = ctx.elem
    f32 = elem.f32
    x, W, Y, ids, gate, offsets, perm = ctx.saved_tensors
    k, x_div, weighted, outer, E, has_bias, x_dtype, l_dtype = ctx.cfg
    N, Kd = W.shape[1], W.shape[2]
    P, rows, g_div = ids.numel(), x.shape[0], outer * k
    if f32:
        dA = d_out = d_out.contiguous()
    else:
        d_out = d_out.to(torch.float32).contiguous()
        dA = d_out.to(torch.bfloat16)   # once, for both products
    scale = gate if weighted else None
    dlogits = _gate_grad(d_out, Y, ids, gate, k, E, g_div) if weighted else None
    if not ctx.needs_input_grad[0]:
        dx = None
    elif f32 and _moe_dense_z(Kd, N, x_div, E):
        # dx[r] = sum over the x_div pairs of input row r of scale * dOut-row x W[e] (N, Kd): per-expert sums of the
        # dOut rows, then one product with W viewed as (E*N, Kd) -- no copy
        Z = _expert_sums(d_out, g_div, ids, _ptr(scale), rows, x_div, E, N)
        with _timed(f"dense_z_gemm M{rows} N{Kd} K{E * N}"):
            dx = Z @ W.view(E * N, Kd)
    elif f32 and _moe_sum_in_gemm(Kd, N, x_div):
        # the input rows' gradients are sums over the x_div pairs that read them: folded into the GEMM's epilogue
        dx = _grouped_acc(True, d_out, N, g_div, W, scale, offsets, perm, P, x_div)
    else:
        dxp = _grouped(True, elem, dA, N, g_div, W, scale, offsets, perm, P)
        dx = _combine(dxp, ids, None, rows, x_div // k, k)
    dW, db = _grouped_wgrad(elem, dA, N, g_div, x, Kd if f32 else x.stride(0), x_div, scale, offsets, perm, P, W.shape, has_bias)
    if not f32:   # back in the dtypes of the caller's x and logits
        dx, dlogits = dx if dx is None else dx.to(x_dtype), dlogits.to(l_dtype)
    return dx, dlogits, dW, db


class _RoutedLinear(torch.autograd.Function):
    """Top-k routed expert Linear + ordered combine, one launch per stage for ALL experts.

    x2 (Rx,Kd); logits2 (U,E) with U*k pairs, pair p reads x row p // x_div; W (E,N,Kd);
    bias (E,N) or None.  out[g] = sum over the `outer` units of group g and their k slots (in
    ascending expert id) of gate*expert(x) (weighted) or expert(x) (un-weighted, SwitchHead
    moe_out).  Returns (out (U/outer, N), ids (U,k) int64)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x2, logits2, W, bias, k, x_div, weighted, outer):
        _require_device(x2, logits2, W, bias)
        x2, W = x2.contiguous(), W.contiguous()
        _routed_dims(x2, logits2, W, k, x_div, outer)
        return _routed_fwd(ctx, _MOE_F32, x2, logits2.detach(), W, bias, k, x_div, weighted, outer, (torch.float32,) * 2)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, d_out, _d_ids):
        return (None,) * 8 if d_out is None else _routed_bwd(ctx, d_out) + (None,) * 4


# AMK_MOE_BF16: MoELayer's routed expert products under bf16 autocast on bf16 operands (csrc/moe_bf16.hip,
# v_mfma_f32_32x32x16_bf16, f32 accumulation and f32 outputs) instead of upcasting the activations and running the f32
# kernels of csrc/moe.hip.  0: the path before (inputs upcast, f32 kernels).  Measurements: README, "Switches".  Read once
# per process.
MOE_BF16 = os.environ.get("AMK_MOE_BF16", "1") != "0"


class _RoutedLinearBF16(torch.autograd.Function):
    """_RoutedLinear in MoELayer's form (weighted, outer 1) under bf16 autocast: the routing on the f32 logits as ever, x
    cast to bf16 if it arrives in f32, the weight through _w16 (the optimizer's bf16 shadow when it is current), the
    three expert products by csrc/moe_bf16.hip with f32 Y / dW / db, combine and gate gradient by the f32 kernels.  out is
    f32; dx and dlogits come back in the dtypes of x and logits."""

    @staticmethod
    def forward(ctx, x2, logits2, W, bias, k, x_div):
        _require_device(W, bias)
        _routed_dims(x2, logits2, W, k, x_div, 1)
        if not (x2.is_cuda and logits2.is_cuda):
            raise RuntimeError("amk ops run only on MI355X (HIP) tensors; got a CPU tensor. There is no CPU fallback.")
        x16 = _row_major_view(x2.to(torch.bfloat16), 8)
        w16 = _w16(W).contiguous()
        b32 = bias.detach().contiguous() if bias is not None else None
        return _routed_fwd(ctx, _MOE_BF16, x16, logits2.detach().float(), w16, b32, k, x_div, True, 1, (x2.dtype, logits2.dtype))

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, _d_ids):
        return (None,) * 6 if d_out is None else _routed_bwd(ctx, d_out) + (None,) * 2


def _moe_bf16_ok(x2, logits2, W, bias, weighted, outer):
    """MoELayer's form under bf16 autocast on HIP tensors, an f32 master weight, N and Kd multiples of 8."""
    return (MOE_BF16 and weighted and outer == 1 and _bf16_autocast() and x2.is_cuda and logits2.is_cuda and W.is_cuda
            and W.dtype == torch.float32 and W.dim() == 3 and W.shape[1] % 8 == 0 and W.shape[2] % 8 == 0
            and x2.dtype in (torch.float32, torch.bfloat16) and logits2.dtype in (torch.float32, torch.bfloat16)
            and (bias is None or bias.dtype == torch.float32))


def routed_linear(x2, logits2, W, bias, k, x_div, weighted=True, outer=1):
    if _moe_bf16_ok(x2, logits2, W, bias, weighted, outer):
        with torch.autocast("cuda", enabled=False):
            return _RoutedLinearBF16.apply(x2, logits2, W, bias, k, x_div)
    return _RoutedLinear.apply(x2, logits2, W, bias, k, x_div, weighted, outer)


def _topk(logits2, k):
    """(ids int64 (U,k), gate (U,k)): amk_moe_route's selection stage alone."""
    U, E = logits2.shape
    ids = torch.empty((U, k), device=logits2.device, dtype=torch.int64)
    gate = torch.empty((U, k), device=logits2.device, dtype=torch.float32)
    _lib.check(_lib.load().amk_moe_topk(_ptr(logits2.contiguous()), U, E, k, _ptr(ids), _ptr(gate), _stream()), "amk_moe_topk")
    return ids, gate


def _route_distinct(ids, G, fan, E):
    """(offsets (E+1), perm): the distinct (row group, expert) combinations as virtual pairs g*E + e, by expert."""
    dev = ids.device
    mask = torch.empty((G,), device=dev, dtype=torch.int64)
    offsets, perm = _i32(E + 1, dev), _i32(G * min(fan, E), dev)
    _lib.check(_lib.load().amk_moe_route_distinct(_ptr(ids), G, fan, E, _ptr(mask), _ptr(offsets), _ptr(perm), _stream()),
               "amk_moe_route_distinct")
    return offsets, perm


def distinct_experts_ok(dim, d, fan, E, *weights):
    """The SwitchHead forms below apply: a token's fan = h*k pairs are at least E/2, at most 64 experts, model rows at least
    256 wide and 4x the head dim (ops._moe_dense_z), everything on the GPU."""
    return E <= 64 and _moe_dense_z(dim, d, fan, E) and dim % 4 == 0 and all(w.is_cuda for w in weights)


def _switchhead_dims(what, name, a2, rows, logits2, W, H):
    U = logits2.shape[0]
    if a2.shape != (rows, W.shape[2]) or U % H:
        raise RuntimeError(f"{what}: shapes disagree: {name} {tuple(a2.shape)} U {U} H {H} W {tuple(W.shape)}")


def _shared_rows_fwd(ctx, elem, x, logits32, W, k, H, dtypes):
    U, E = logits32.shape
    N, Kd = W.shape[1], W.shape[2]
    G, fan = U // H, H * k
    with _timed(f"moe_topk U{U} E{E} k{k} + distinct lists"):
        ids, gate = _topk(logits32, k)
        offsets, perm = _route_distinct(ids, G, fan, E)
    # V (G*E, N): rows of chosen (token, expert) only
    V = _grouped(False, elem, x, Kd if elem.f32 else x.stride(0), E, W, None, offsets, perm, G * E, U * k, _DISTINCT)
    out = _combine_rows(V, ids, gate, U, k, fan, E)
    return _done(ctx, elem, (x, W, V, ids, gate, offsets, perm), (k, H) + dtypes, out, ids)


def _shared_rows_bwd(ctx, d_out):
    elem = ctx.elem
    x, W, V, ids, gate, offsets, perm = ctx.saved_tensors
    k, H, x_dtype, l_dtype = ctx.cfg
    E, N, Kd = W.shape
    G, fan = x.shape[0], H * k
    f32 = elem.f32
    if f32:
        d_in = d32 = d_out.contiguous()
    else:
        d32 = d_out.to(torch.float32).contiguous()   # the gate gradient reads f32 rows
        d_in = _row_major_view(d_out, 8) if d_out.dtype == torch.bfloat16 else d32   # the sums read bf16 rows as they are
    dlogits = _gate_grad(d32, V, ids, gate, k, E, k, fan)
    Z = _expert_sums(d_in, k, ids, _ptr(gate), G, fan, E, N, elem)   # (G, E*N): gated output gradients per (token, expert)
    dx = None
    if ctx.needs_input_grad[0]:
        with _timed(f"{elem.prefix}dense_z_gemm M{G} N{Kd} K{E * N}"):
            dx = Z @ W.view(E * N, Kd)
            if not f32:
                dx = dx.to(x_dtype)
    dW, _ = _grouped_wgrad(elem, Z, N, 1, x, Kd if f32 else x.stride(0), E, None, offsets, perm, G * E, W.shape, False, G * fan,
                           _DISTINCT)
    return dx, dlogits if f32 else dlogits.to(l_dtype), dW, None, None


class _SharedRowExperts(torch.autograd.Function):
    """SwitchHead's V experts (reference switchhead_attention.py:58-73): U = G*H units, the H units (heads) of group g
    (token) all read x row g; out[u] = sum over the unit's k slots of gate * x[g] W[e]^T.  The product x[g] W[e]^T does not
    depend on the head, so it is formed once per DISTINCT (token, expert) -- amk_moe_route_distinct's lists feed the same
    grouped GEMMs -- and fanned out to the units that chose it; backward: per-expert sums of the (gated) output gradients,
    then dx as one dense product and dW from the distinct rows.  Returns (out (U, N), ids (U, k))."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x2, logits2, W, k, H):
        _require_device(x2, logits2, W)
        x2, W = x2.contiguous(), W.contiguous()
        _switchhead_dims("shared-row experts", "x", x2, logits2.shape[0] // H, logits2, W, H)
        return _shared_rows_fwd(ctx, _MOE_F32, x2, logits2.detach(), W, k, H, (torch.float32,) * 2)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, d_out, _d_ids):
        return (None,) * 5 if d_out is None else _shared_rows_bwd(ctx, d_out)


def _summed_fwd(ctx, elem, a2, logits32, W, k, H):
    U, E = logits32.shape
    N, Kd = W.shape[1], W.shape[2]
    G, fan = U // H, H * k
    with _timed(f"moe_topk U{U} E{E} k{k}"):
        ids, _gate = _topk(logits32, k)
    Z = _expert_sums(a2, k, ids, _NULL, G, fan, E, Kd, elem)
    with _timed(f"{elem.prefix}dense_z_gemm M{G} N{N} K{E * Kd}"):
        out = Z @ W.permute(0, 2, 1).reshape(E * Kd, N)
    return _done(ctx, elem, (W, Z, ids), (k, H, a2.dtype), out, ids)


def _summed_bwd(ctx, d_out):
    elem = ctx.elem
    W, Z, ids = ctx.saved_tensors
    k, H, a_dtype = ctx.cfg
    E, N, Kd = W.shape
    G, fan = Z.shape[0], H * k
    if elem.f32:
        d, ldd = d_out.contiguous(), N
    else:
        d = _row_major_view(d_out.to(torch.bfloat16), 8)   # once, for both products
        ldd = d.stride(0)
    offsets, perm = _route_distinct(ids, G, fan, E)
    da = None
    if ctx.needs_input_grad[0]:
        D = _grouped(True, elem, d, ldd, E, W, None, offsets, perm, G * E, G * fan, _DISTINCT)
        da = _combine_rows(D, ids, None, G * H, k, fan, E)
        if not elem.f32:
            da = da.to(a_dtype)
    dW, _ = _grouped_wgrad(elem, d, ldd, E, Z, Kd, 1, None, offsets, perm, G * E, W.shape, False, G * fan, _DISTINCT)
    return da, None, dW, None, None


class _SummedExperts(torch.autograd.Function):
    """SwitchHead's output experts + head sum (reference switchhead_attention.py:75-88,115): U = G*H units with their own
    rows a2[u]; out[g] = sum over the group's H*k pairs of a2[u] W[e]^T, un-weighted.  Forward: per-expert sums of the rows,
    one dense product.  Backward: d_out[g] W[e] once per distinct (token, expert), fanned out to the units; dW from the
    distinct rows of the forward's sums.  Returns (out (G, N), ids (U, k)); the logits get no gradient (un-weighted)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, a2, logits2, W, k, H):
        _require_device(a2, logits2, W)
        a2, W = a2.contiguous(), W.contiguous()
        _switchhead_dims("summed experts", "a", a2, logits2.shape[0], logits2, W, H)
        return _summed_fwd(ctx, _MOE_F32, a2, logits2.detach(), W, k, H)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, d_out, _d_ids):
        return (None,) * 5 if d_out is None else _summed_bwd(ctx, d_out)


# AMK_SWITCHHEAD_BF16: SwitchHeadAttention's experts under bf16 autocast on bf16 operands -- the narrow grouped kernels
# and the bf16 per-expert sums of csrc/moe_bf16.hip, the dense Z products on the library's bf16 GEMM -- instead of
# upcasting what autocast hands over and running the f32 kernels.  0: the path before.  Measurements: README,
# "Switches".  Read once per process.
SWITCHHEAD_BF16 = os.environ.get("AMK_SWITCHHEAD_BF16", "1") != "0"


class _SharedRowExpertsBF16(torch.autograd.Function):
    """_SharedRowExperts under bf16 autocast: the routing on the f32 logits as ever, x cast to bf16 once, the weight
    through _w16 (the optimizer's bf16 shadow when it is current); V (G*E, d) f32 by amk_grouped_gemm_nt64_bf16, combine
    and gate gradient by the f32 kernels (out is f32); backward: Z16 = the gated per-expert sums of d_out in bf16,
    dx = Z16 @ W16 on the library's bf16 GEMM (handed back in x's dtype), dW f32 by amk_grouped_gemm_wgrad64_bf16."""

    @staticmethod
    def forward(ctx, x2, logits2, W, k, H):
        _require_device(W)
        _switchhead_dims("shared-row experts", "x", x2, logits2.shape[0] // H, logits2, W, H)
        x16 = _row_major_view(x2.detach().to(torch.bfloat16), 8)
        w16 = _w16(W).detach().contiguous()
        return _shared_rows_fwd(ctx, _MOE_BF16_64, x16, logits2.detach().float(), w16, k, H, (x2.dtype, logits2.dtype))

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, _d_ids):
        return (None,) * 5 if d_out is None else _shared_rows_bwd(ctx, d_out)


class _SummedExpertsBF16(torch.autograd.Function):
    """_SummedExperts under bf16 autocast: Z16 = the per-expert sums of the (f32) attention rows in bf16, out = Z16 @ W16
    as (E*d, dim) on the library's bf16 GEMM -- out leaves in bf16, as an autocast nn.Linear's does; backward: d_out cast
    to bf16 once, D (G*E, d) f32 by amk_grouped_gemm_nn64_bf16 fanned out by the f32 combine (da f32), dW f32 by
    amk_grouped_gemm_wgrad64_bf16 on (d16, Z16).  The logits get no gradient."""

    @staticmethod
    def forward(ctx, a2, logits2, W, k, H):
        _require_device(W)
        _switchhead_dims("summed experts", "a", a2, logits2.shape[0], logits2, W, H)
        a2 = _row_major_view(a2.detach(), 8)
        w16 = _w16(W).detach().contiguous()
        return _summed_fwd(ctx, _MOE_BF16_64, a2, logits2.detach().float(), w16, k, H)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, _d_ids):
        return (None,) * 5 if d_out is None else _summed_bwd(ctx, d_out)


def _switchhead_bf16_ok(a2, logits2, W, d):
    """bf16 autocast on HIP tensors, an f32 master weight with d <= 64 and both sides multiples of 8, and either the
    weight trains or nothing does (a frozen weight under a trainable input keeps the f32 Functions)."""
    return (SWITCHHEAD_BF16 and _bf16_autocast()
            and a2.is_cuda and logits2.is_cuda and W.is_cuda and W.dtype == torch.float32 and W.dim() == 3
            and d <= 64 and W.shape[1] % 8 == 0 and W.shape[2] % 8 == 0
            and a2.dtype in (torch.float32, torch.bfloat16) and logits2.dtype in (torch.float32, torch.bfloat16)
            and (W.requires_grad or not (torch.is_grad_enabled() and (a2.requires_grad or logits2.requires_grad))))


def switchhead_bf16_shapes(dim, d, fan, E):
    """A SwitchHeadAttention of these sizes takes the bf16 Functions under bf16 autocast (with f32 master weights on the
    GPU): the switch, the distinct form (distinct_experts_ok) and d <= 64 with d and dim multiples of 8."""
    return SWITCHHEAD_BF16 and distinct_experts_ok(dim, d, fan, E) and d <= 64 and d % 8 == 0 and dim % 8 == 0


def shared_row_experts(x2, logits2, W, k, H):
    if _switchhead_bf16_ok(x2, logits2, W, W.shape[1] if W.dim() == 3 else 0):
        with torch.autocast("cuda", enabled=False):
            return _SharedRowExpertsBF16.apply(x2, logits2, W, k, H)
    return _SharedRowExperts.apply(x2, logits2, W, k, H)


def summed_experts(a2, logits2, W, k, H):
    if _switchhead_bf16_ok(a2, logits2, W, W.shape[2] if W.dim() == 3 else 0):
        with torch.autocast("cuda", enabled=False):
            return _SummedExpertsBF16.apply(a2, logits2, W, k, H)
    return _SummedExperts.apply(a2, logits2, W, k, H)


# ---------------------------------------------------------------------------- agent attention
# The op's two element types: (dtype of qkv, o and their gradients, forward, backward, workspace query).  agents, vagent,
# stats1, the workspaces and the convolution's parameters and gradients are f32 in both.
_AGENT_F32 = (torch.float32, "amk_agent_attn_fwd", "amk_agent_attn_bwd", "amk_agent_ws_floats_dh")
_AGENT_BF16 = (torch.bfloat16, "amk_agent_attn_bf16_fwd", "amk_agent_attn_bf16_bwd", "amk_agent_bf16_ws_floats")


def _agent_fwd(ctx, elem, qkv2, conv_w, conv_b, H, D, P, scale):
    ctx.elem = elem
    dtype, fwd, _, ws_floats = elem
    B, T, _ = qkv2.shape
    qkv2 = qkv2.contiguous()
    qkv = qkv2.view(B, T, 3, H, D)
    q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
    dev = qkv2.device
    o = _new_bthd(B, H, T, D, qkv2, dtype)
    agents = torch.empty((B, H, P, D), device=dev, dtype=torch.float32)
    vagent = torch.empty_like(agents)
    stats1 = torch.empty((B, H, P, 2), device=dev, dtype=torch.float32)
    cw, cb = conv_w.contiguous(), conv_b.contiguous()
    L = _lib.load()
    ws = torch.empty((max(getattr(L, ws_floats)(B, H, T, P, D, 0), 1),), device=dev, dtype=torch.float32)
    rc = getattr(L, fwd)(_ptr(q), _ptr(k), _ptr(v), _ptr(cw), _ptr(cb), _ptr(o), _ptr(agents), _ptr(vagent), _ptr(stats1),
                         _ptr(ws), B, H, T, D, P, *_strides4(q), *_strides4(k), *_strides4(v), *_strides4(o), float(scale),
                         _stream())
    _lib.check(rc, fwd)
    ctx.save_for_backward(qkv2, cw, agents, vagent, stats1)
    ctx.cfg = (H, D, P, scale)
    return o.permute(0, 2, 1, 3).reshape(B, T, H * D)


class _AgentAttn(torch.autograd.Function):
    """qkv (B,T,3*h*d) with the reference's '(qkv h d)' column order -> o (B,T,h*d)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, qkv2, conv_w, conv_b, *cfg):
        _require_device(qkv2, conv_w, conv_b)
        return _agent_fwd(ctx, _AGENT_F32, qkv2, conv_w, conv_b, *cfg)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, d_o2):
        dtype, _, bwd, ws_floats = ctx.elem
        qkv2, cw, agents, vagent, stats1 = ctx.saved_tensors
        H, D, P, scale = ctx.cfg
        B, T, _ = qkv2.shape
        dev = qkv2.device
        qkv = qkv2.view(B, T, 3, H, D)
        q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
        d_o = d_o2.to(dtype).contiguous().view(B, T, H, D).permute(0, 2, 1, 3)
        dqkv2 = torch.empty_like(qkv2)
        dqkv = dqkv2.view(B, T, 3, H, D)
        dq, dk, dv = (dqkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
        L = _lib.load()
        cells = B * H * L.amk_agent_num_chunks_dh(T, D)
        ws = torch.empty((max(getattr(L, ws_floats)(B, H, T, P, D, 1), 1),), device=dev, dtype=torch.float32)
        dw_part = torch.empty((cells, 9, D), device=dev, dtype=torch.float32)
        db_part = torch.empty((cells, D), device=dev, dtype=torch.float32)
        rc = getattr(L, bwd)(_ptr(q), _ptr(k), _ptr(v), _ptr(cw), _ptr(d_o), _ptr(agents), _ptr(vagent), _ptr(stats1),
                             _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), _ptr(dw_part), _ptr(db_part),
                             B, H, T, D, P, *_strides4(q), *_strides4(k), *_strides4(v), *_strides4(d_o),
                             *_strides4(dq), *_strides4(dk), *_strides4(dv), float(scale), _stream())
        _lib.check(rc, bwd)
        dconv_w = torch.empty((D, 1, 3, 3), device=dev, dtype=torch.float32)
        dconv_b = torch.empty((D,), device=dev, dtype=torch.float32)
        _lib.check(L.amk_agent_conv_grad_reduce(_ptr(dw_part), _ptr(db_part), cells, D, _ptr(dconv_w), _ptr(dconv_b), _stream()),
                   "amk_agent_conv_grad_reduce")
        return dqkv2, dconv_w, dconv_b, None, None, None, None


# Mixed precision: under bf16 autocast the qkv projection hands over bf16 and W_o takes bf16, so the f32 core above sits
# between an upcast of qkv, a downcast of o and the two casts of their gradients.  csrc/agent.hip instantiates the same
# kernels on bf16 elements (f32 arithmetic in the f32 path's order, o / dq / dk / dv rounded once on the store; agents,
# vagent, stats1, the workspaces and the convolution's parameters and gradients stay f32): the same bits as the cast
# path at half the bytes through the eight tensors, without the four cast kernels.  AMK_AGENT_BF16=0 keeps the cast
# path.  Read once per process.  Measured by tools/kbench_agent.py --autocast bf16 (profiles/kbench_agent_bf16.log).
AGENT_BF16 = os.environ.get("AMK_AGENT_BF16", "1") == "1"


class _AgentAttnBF16(_AgentAttn):
    """_AgentAttn on bf16 elements: qkv (B,T,3*h*d) bf16 -> o (B,T,h*d) bf16; conv_w / conv_b and their gradients f32."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, *args):
        return _agent_fwd(ctx, _AGENT_BF16, *args)


def _agent_bf16_ok(qkv2, conv_w, conv_b, dim_head, pool):
    return (AGENT_BF16 and _bf16_autocast() and qkv2.is_cuda and qkv2.dtype == torch.bfloat16
            and conv_w.is_cuda and conv_b.is_cuda and conv_w.dtype == torch.float32 and conv_b.dtype == torch.float32
            and dim_head in (32, 64, 128) and pool <= 16)


def agent_attention(qkv2, conv_w, conv_b, num_heads, dim_head, pool, scale):
    if _agent_bf16_ok(qkv2, conv_w, conv_b, dim_head, pool):
        return _AgentAttnBF16.apply(qkv2, conv_w, conv_b, num_heads, dim_head, pool, scale)
    return _AgentAttn.apply(qkv2, conv_w, conv_b, num_heads, dim_head, pool, scale)


# ---------------------------------------------------------------------------- SwiGLU gate
def _c16(t):
    """t contiguous on 16-byte aligned storage, as the float4 kernels read it: a copy only where a view's storage offset
    (flat[1:1 + M * D].view(M, D)) or its strides force one."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _SwiGLU(torch.autograd.Function):
    FWD, BWD = "amk_swiglu_fwd", "amk_swiglu_bwd"

    @classmethod
    def forward(cls, ctx, ab):
        _require_device(ab)
        H = ab.shape[-1] // 2
        ab2 = _c16(ab).view(-1, 2 * H)
        M = ab2.shape[0]
        out = torch.empty((M, H), device=ab.device, dtype=torch.float32)
        L = _lib.load()
        _lib.check(getattr(L, cls.FWD)(_ptr(ab2), M, H, _ptr(out), _stream()), cls.FWD)
        ctx.save_for_backward(ab2)
        ctx.shape = ab.shape
        return out.view(*ab.shape[:-1], H)

    @classmethod
    def backward(cls, ctx, d_out):
        (ab2,) = ctx.saved_tensors
        M, H2 = ab2.shape
        d_out = _c16(d_out).view(M, H2 // 2)
        d_ab = torch.empty_like(ab2)
        L = _lib.load()
        _lib.check(getattr(L, cls.BWD)(_ptr(ab2), _ptr(d_out), M, H2 // 2, _ptr(d_ab), _stream()), cls.BWD)
        return d_ab.view(ctx.shape)


class _GEGLU(_SwiGLU):
    FWD, BWD = "amk_geglu_fwd", "amk_geglu_bwd"


def _f32_outside_autocast(fn, x, act):
    """(the gate Functions are classmethod-based: no custom_fwd; under autocast the input is upcast here)
    A half width that is no multiple of 4 has no kernel (16 bytes per lane): act(a) * b in torch, as layer_norm does
    for the widths it has no kernel for."""
    if x.shape[-1] % 8 != 0:
        a, b = x.chunk(2, dim=-1)
        return act(a) * b
    if torch.is_autocast_enabled():
        with torch.autocast("cuda", enabled=False):
            return fn(x.float())
    return fn(x)


class _SwiGLUBF16(torch.autograd.Function):
    """The gate on bf16 tensors (mixed precision): bf16 in, bf16 out, f32 arithmetic (csrc/mixed_bf16.hip)."""

    @staticmethod
    def forward(ctx, ab):
        H = ab.shape[-1] // 2
        ab2 = ab.contiguous().view(-1, 2 * H)
        M = ab2.shape[0]
        out = torch.empty((M, H), device=ab.device, dtype=torch.bfloat16)
        _lib.check(_lib.load().amk_swiglu_bf16_fwd(_ptr(ab2), M, H, _ptr(out), _stream()), "amk_swiglu_bf16_fwd")
        ctx.save_for_backward(ab2)
        ctx.shape = ab.shape
        return out.view(*ab.shape[:-1], H)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        (ab2,) = ctx.saved_tensors
        M, H2 = ab2.shape
        d_out = d_out.to(torch.bfloat16).contiguous().view(M, H2 // 2)
        d_ab = torch.empty_like(ab2)
        _lib.check(_lib.load().amk_swiglu_bf16_bwd(_ptr(ab2), _ptr(d_out), M, H2 // 2, _ptr(d_ab), _stream()), "amk_swiglu_bf16_bwd")
        return d_ab.view(ctx.shape)


# Mixed precision: bf16-in / bf16-out element-wise kernels between the bf16 GEMMs (no separate cast passes);
# AMK_MIXED_ELEMENTWISE=0 returns to the round-2 behaviour (inputs upcast, f32 kernels, outputs cast by autocast).
MIXED_ELEMENTWISE = os.environ.get("AMK_MIXED_ELEMENTWISE", "1") == "1"


def swiglu(ab):
    """silu(a) * b for ab = (..., 2H) = (a | b): one HBM pass forward, one backward."""
    if MIXED_ELEMENTWISE and ab.dtype == torch.bfloat16 and ab.is_cuda and ab.shape[-1] % 8 == 0:
        with torch.autocast("cuda", enabled=False):
            return _SwiGLUBF16.apply(ab)
    return _f32_outside_autocast(_SwiGLU.apply, ab, torch.nn.functional.silu)


def geglu(ab):
    """gelu(a) * b for ab = (..., 2H) = (a | b) (exact erf GELU): the transformer FFN gate."""
    return _f32_outside_autocast(_GEGLU.apply, ab, torch.nn.functional.gelu)


# ---------------------------------------------------------------------------- residual + LayerNorm
def _ln_supported(D):
    return 0 < D <= 4096 and D % 4 == 0


def _ln_param_grads(part, params):
    """(d gamma, d beta) from the kernel's (rows, 2, D) partial sums; summed straight into the reducer's gradient views
    where they can be claimed (amk.dp.GradReducer(direct_grads=True): those come back as None)."""
    weight, bias = params if params is not None else (None, None)
    (wr, wv), (br, bv) = _claim_late(weight), _claim_late(bias)
    if wv is None and bv is None:
        dgb = part.sum(0)
        return dgb[0], dgb[1]
    dw = db = None
    if wv is not None:
        torch.sum(part[:, 0], dim=0, out=wv)
        wr.wrote(weight)
    else:
        dw = part[:, 0].sum(0)
    if bv is not None:
        torch.sum(part[:, 1], dim=0, out=bv)
        br.wrote(bias)
    else:
        db = part[:, 1].sum(0)
    return dw, db


def _claim_late(p):
    return _claim(p)   # (_claim is defined with the Linear layers below)


def _ln_backward(dy, h, dh_in, weight, mean, rstd, params=None):
    M, D = h.shape
    L = _lib.load()
    dh = torch.empty_like(h)
    part = torch.empty((L.amk_rowsum_num_partials(M), 2, D), device=h.device, dtype=torch.float32)
    _lib.check(L.amk_add_layernorm_bwd(_ptr(dy), _ptr(h), _ptr(dh_in), _ptr(weight), _ptr(mean), _ptr(rstd),
                                       M, D, _ptr(dh), _ptr(part), _stream()), "amk_add_layernorm_bwd")
    dw, db = _ln_param_grads(part, params)
    return dh, dw, db


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, weight, bias, eps):
        _require_device(x, weight, bias)
        D = x.shape[-1]
        x2 = _c16(x).view(-1, D)
        M = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty((M,), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        w, b = _c16(weight), _c16(bias)
        L = _lib.load()
        _lib.check(L.amk_add_layernorm_fwd(_ptr(x2), _NULL, _ptr(w), _ptr(b), M, D, float(eps), _NULL, _ptr(y),
                                           _ptr(mean), _ptr(rstd), _stream()), "amk_add_layernorm_fwd")
        ctx.save_for_backward(x2, w, mean, rstd)
        ctx.shape = x.shape
        ctx.params = (weight, bias)
        return y.view(x.shape)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, dy):
        x2, w, mean, rstd = ctx.saved_tensors
        dx, dw, db = _ln_backward(_c16(dy).view(x2.shape), x2, None, w, mean, rstd, ctx.params)
        return dx.view(ctx.shape), dw, db, None


class _AddLayerNorm(torch.autograd.Function):
    """(x, res) -> (h, y) with h = x + res, y = LN(h); the gradient of h is added inside the LN backward."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, res, weight, bias, eps):
        _require_device(x, res, weight, bias)
        D = x.shape[-1]
        x2 = _c16(x).view(-1, D)
        r2 = _c16(res).view(-1, D)
        M = x2.shape[0]
        h = torch.empty_like(x2)
        y = torch.empty_like(x2)
        mean = torch.empty((M,), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        w, b = _c16(weight), _c16(bias)
        L = _lib.load()
        _lib.check(L.amk_add_layernorm_fwd(_ptr(x2), _ptr(r2), _ptr(w), _ptr(b), M, D, float(eps), _ptr(h), _ptr(y),
                                           _ptr(mean), _ptr(rstd), _stream()), "amk_add_layernorm_fwd")
        ctx.save_for_backward(h, w, mean, rstd)
        ctx.shape = x.shape
        ctx.params = (weight, bias)
        ctx.set_materialize_grads(False)
        return h.view(x.shape), y.view(x.shape)

    @staticmethod
    @once_differentiable
    @_amp_bwd
    def backward(ctx, dh_in, dy):
        h, w, mean, rstd = ctx.saved_tensors
        if dy is None:  # y unused downstream: only the residual stream carries gradient
            if dh_in is None:
                return None, None, None, None, None
            return dh_in, dh_in, None, None, None
        dh2 = _c16(dh_in).view(h.shape) if dh_in is not None else None
        dh, dw, db = _ln_backward(_c16(dy).view(h.shape), h, dh2, w, mean, rstd, ctx.params)
        dh = dh.view(ctx.shape)
        return dh, dh, dw, db, None


class _AddLayerNormMixed(torch.autograd.Function):
    """(x, res) -> (h, y) for the mixed-precision mode: x f32 or bf16 (a branch's output), res f32 (the residual stream)
    or None; h = x + res in f32 (x itself without a residual), y = LN(h) in bf16 for the bf16 GEMMs that consume it.
    Backward: dy bf16 or f32; the gradient of the residual stream stays f32, the branch gets it rounded to bf16."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        _require_device(res, weight, bias)
        D = x.shape[-1]
        x2 = x.contiguous().view(-1, D)
        M = x2.shape[0]
        xb = x2.dtype == torch.bfloat16
        if not xb and x2.dtype != torch.float32:
            raise RuntimeError(f"mixed LayerNorm takes f32 or bf16 inputs, got {x2.dtype}")
        r2 = res.contiguous().view(-1, D) if res is not None else None
        need_h = r2 is not None or xb
        h = torch.empty((M, D), device=x.device, dtype=torch.float32) if need_h else None
        y = torch.empty((M, D), device=x.device, dtype=torch.bfloat16)
        mean = torch.empty((M,), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        w, b = weight.contiguous(), bias.contiguous()
        _lib.check(_lib.load().amk_add_layernorm_mixed_fwd(_ptr(x2), 1 if xb else 0, _ptr(r2), _ptr(w), _ptr(b), M, D, float(eps),
                                                          _ptr(h), _ptr(y), _ptr(mean), _ptr(rstd), _stream()),
                   "amk_add_layernorm_mixed_fwd")
        hs = h if need_h else x2
        ctx.save_for_backward(hs, w, mean, rstd)
        ctx.cfg = (x.shape, xb, res is not None)
        ctx.params = (weight, bias)
        ctx.set_materialize_grads(False)
        return hs.view(x.shape), y.view(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dh_in, dy):
        h, w, mean, rstd = ctx.saved_tensors
        shape, xb, has_res = ctx.cfg
        M, D = h.shape
        if dy is None:
            if dh_in is None:
                return None, None, None, None, None
            dx = dh_in.to(torch.bfloat16) if xb else dh_in
            return dx, (dh_in if has_res else None), None, None, None
        dyb = dy.dtype == torch.bfloat16
        dy2 = (dy if dyb else dy.float()).contiguous().view(M, D)
        dh2 = dh_in.float().contiguous().view(M, D) if dh_in is not None else None
        L = _lib.load()
        dh = torch.empty((M, D), device=h.device, dtype=torch.float32)
        dh16 = torch.empty((M, D), device=h.device, dtype=torch.bfloat16) if xb else None
        part = torch.empty((L.amk_rowsum_num_partials(M), 2, D), device=h.device, dtype=torch.float32)
        _lib.check(L.amk_add_layernorm_mixed_bwd(_ptr(dy2), 1 if dyb else 0, _ptr(h), _ptr(dh2), _ptr(w), _ptr(mean), _ptr(rstd),
                                                 M, D, _ptr(dh), _ptr(dh16), _ptr(part), _stream()), "amk_add_layernorm_mixed_bwd")
        dw, db = _ln_param_grads(part, ctx.params)
        dhv = dh.view(shape)
        dx = dh16.view(shape) if xb else dhv
        return dx, (dhv if has_res else None), dw, db, None


def _mixed_ln():
    return (MIXED_ELEMENTWISE and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)


def layer_norm(x, weight, bias, eps=1e-5, branch=False):
    """LayerNorm over the last axis (one HBM pass forward, one backward incl. the gamma / beta partials).
    branch=True: the result only feeds Linear layers -- under bf16 autocast it is then produced in bf16 directly."""
    if not _ln_supported(x.shape[-1]) or x.numel() == 0 or not x.is_cuda:
        return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    if branch and _mixed_ln():
        with torch.autocast("cuda", enabled=False):
            return _AddLayerNormMixed.apply(x, None, weight, bias, eps)[1]
    return _LayerNorm.apply(x, weight, bias, eps)


def add_layer_norm(x, res, weight, bias, eps=1e-5, branch=False):
    """h = x + res, y = LayerNorm(h): returns (h, y) from one kernel (amk_add_layernorm_fwd).  branch: see layer_norm."""
    if not _ln_supported(x.shape[-1]) or x.numel() == 0 or not x.is_cuda:
        h = x + res
        return h, torch.nn.functional.layer_norm(h, (h.shape[-1],), weight, bias, eps)
    if branch and _mixed_ln():
        with torch.autocast("cuda", enabled=False):
            return _AddLayerNormMixed.apply(x, res.float(), weight, bias, eps)
    return _AddLayerNorm.apply(x, res, weight, bias, eps)


# ---------------------------------------------------------------------------- Linear with bias
def colsum(x2):
    """Column sums of an (M, N) matrix (the bias gradient of a Linear)."""
    M, N = x2.shape
    if N % 4 != 0 or N > 1024:  # wide matrices: torch's reduction is as fast (measured at N = 2736: 71 vs 88 us)
        return x2.sum(0)
    x2 = _c16(x2)
    L = _lib.load()
    part = torch.empty((L.amk_rowsum_num_partials(M), N), device=x2.device, dtype=torch.float32)
    _lib.check(L.amk_colsum(_ptr(x2), M, N, _ptr(part), _stream()), "amk_colsum")
    return part.sum(0)


class _BiasLinear(torch.autograd.Function):
    """F.linear with bias; the GEMMs stay with the vendor library (same calls autograd would make, so
    the shipped TunableOp selections apply), the bias gradient is amk_colsum instead of a strided sum."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_device(x, weight, bias)
        ctx.save_for_backward(x, weight)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, dy.shape[-1])
        dx = dy2.mm(weight).view(x.shape) if ctx.needs_input_grad[0] else None
        dw = dy2.t().mm(x.reshape(-1, x.shape[-1])) if ctx.needs_input_grad[1] else None
        db = colsum(dy2) if ctx.needs_input_grad[2] else None
        return dx, dw, db


# Dense GEMMs of the nn.Linear layers: "f32" = the vendor library's exact-f32 kernels (rocBLAS / hipBLASLt, chosen
# by TunableOp; 0.79 of the f32 MFMA peak) -- the parity mode and the headline; "bf16x6" = csrc/gemm_x6.hip for the
# forward and the input gradient (split-bf16 products: f32-level error, bound = bf16 MFMA peak / 6); the weight
# gradient stays with the library.  "auto" (default) = "f32", except that a Linear, q / kv pair or SwiGLU FFN whose weights
# carry CURRENT split-bf16 planes (amk.optim.FlatAdam.enable_planes: split once per optimizer step, not per call) runs its
# forward and input gradient on the fused forms of csrc/gemm_x6.hip (_X6Linear, _X6Linear2, _X6SwiGLUFFN below); a module
# called outside such a train step has no planes and takes exactly the "f32" paths.
GEMM_MODE = os.environ.get("AMK_GEMM", "auto")
if GEMM_MODE not in ("auto", "f32", "bf16x6"):
    raise RuntimeError(f"AMK_GEMM must be auto, f32 or bf16x6 (got {GEMM_MODE!r})")
# AMK_X6_LINEAR=0: no plane shadow, no x6 forms under "auto" (the A/B switch; read by VQGANTrainStep and at dispatch)
X6_LINEAR = os.environ.get("AMK_X6_LINEAR", "1") != "0"
# the layer kinds "auto" puts on the x6 forms (profiles/x6_linear_step_breakdown.log decides): linear, linear2, ffn
X6_AUTO_KINDS = frozenset(k for k in os.environ.get("AMK_X6_KINDS", "linear,linear2,ffn").split(",") if k)
# ... and the products of such a layer that run there: "fwd" = the forward products (always), "dx" = the input gradients
# too (against the planes of W^T, which are only kept with it).  "dx" is off by default: back to back every product wins
# (profiles/kbench_x6_linear.log), but in the step the input gradients' 1.2 ms came with 1.0 ms on the attention backward
# that runs between them and 0.9 ms on the weight-gradient kernels (profiles/x6_linear_step_breakdown.log).
# "dw" = the weight (and bias) gradients of such a layer on csrc/gemm_x6_tn.hip (both operands are activations and are
# split inside the kernel: no planes involved).  Default "fwd,dw": the weight gradients fall from 11.5 to 7.8 ms of device
# time per step and, unlike "dx", cost the kernels around them nothing measurable -- the headline gains 3.3 ms against a
# parent spread of 0.31 (profiles/x6_tn_step_breakdown.log).  All five gradient shapes of the step are on it: every one wins
# back to back (x1.40 - x1.47, profiles/kbench_x6_tn.log) and the step with all of them cleared the A/B at the first attempt,
# so no shape is held back on the f32 kernel.
X6_AUTO_FORMS = frozenset(k for k in os.environ.get("AMK_X6_FORMS", "fwd,dw").split(",") if k)
# AMK_X6_SHORT_K=0: the forward products with K <= 256 (q | kv, w12 + gate, the patch embedding) run the tile kernel of
# every other form instead of the row-block-stationary one, and q | kv is two launches again (the A/B switch; bit-identical
# results either way).  The library holds the switch (amk_gemm_x6_short_k); it is set here once.
X6_SHORT_K_MAX = 256
_lib.load().amk_gemm_x6_short_k(int(os.environ.get("AMK_X6_SHORT_K", "1") != "0"))


def _x6_tn_ok(M, N, K, *lds):
    """The preconditions of amk_gemm_x6_tn for a gradient (N, K) over M rows with operand row strides `lds`, so that other
    shapes take dense.gemm_tn instead of an error from the C side: multiples of 4, and every operand (with the three
    steps its prefetch runs past a chunk) under 1 GiB."""
    if M < 1 or N % 4 or K % 4 or any(ld % 4 for ld in lds):
        return False
    return all((M + 96) * ld * 4 < (1 << 30) for ld in lds) and N * K * 4 < (1 << 30)


def _x6_tn(y, x, **kw):
    """dense.gemm_tn's product for the backward of the x6 Functions: on dense.gemm_x6_tn when the "dw" form is on and the
    shapes are that kernel's, else on dense.gemm_tn (exact f32)."""
    from . import dense

    y2 = kw.get("y2")
    if "dw" in X6_AUTO_FORMS and _x6_tn_ok(y.shape[0], y.shape[1] + (y2.shape[1] if y2 is not None else 0), x.shape[1],
                                           *(t.stride(0) for t in (y, x, y2) if t is not None and t.stride(1) == 1)):
        return dense.gemm_x6_tn(y, x, **kw)
    return dense.gemm_tn(y, x, **kw)


def gemm_x6_nt(a2, b2, bias=None):
    """a2 (M, K) @ b2 (N, K)^T (+ bias): F.linear on 2-D operands through amk_gemm_x6_split + amk_gemm_x6_nt
    (b2, the weight, is split into bf16 planes once per call; a2 inside the GEMM)."""
    _require_device(a2, b2, bias)
    if a2.stride(1) != 1:
        a2 = a2.contiguous()
    if b2.stride(1) != 1:
        b2 = b2.contiguous()
    M, K = a2.shape
    N = b2.shape[0]
    L = _lib.load()
    planes = torch.empty((L.amk_gemm_x6_planes_bytes(N, K),), device=a2.device, dtype=torch.uint8)
    c = torch.empty((M, N), device=a2.device, dtype=torch.float32)
    with _timed(f"gemm_x6_nt M{M} N{N} K{K}"):
        _lib.check(L.amk_gemm_x6_split(_ptr(b2), b2.stride(0), N, K, _ptr(planes), _stream()), "amk_gemm_x6_split")
        rc = L.amk_gemm_x6_nt(_ptr(a2), a2.stride(0), _ptr(planes), _ptr(bias), _ptr(c), N, M, N, K, _stream())
    _lib.check(rc, "amk_gemm_x6_nt")
    return c


def _x6_ok(x, weight):
    """The preconditions of amk_gemm_x6_nt (csrc/gemm_x6.hip), so that other shapes take the library GEMM instead of
    an error from the C side: rows 16-byte aligned (K and the leading dimensions multiples of 4), operands < 2 GiB."""
    K = weight.shape[1]
    if K % 4 or x.numel() == 0 or x.data_ptr() % 16 or weight.data_ptr() % 16:
        return False
    if x.stride(-1) != 1 or (x.dim() >= 2 and x.stride(-2) % 4):
        return False
    return x.numel() * 4 < 0x7ffffff0 and weight.numel() * 8 < 0x7ffffff0   # (A's span; the three bf16 planes of W, padded)


class _LinearX6(torch.autograd.Function):
    """F.linear with the forward and the input gradient on the split-bf16 GEMM."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_device(x, weight, bias)
        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, weight)
        ctx.x_shape = x.shape
        ctx.has_bias = bias is not None
        return gemm_x6_nt(x2, weight, bias).view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, dy.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            N = weight.shape[0]
            if N % 4 == 0:
                dx = gemm_x6_nt(dy2, weight.t().contiguous()).view(ctx.x_shape)   # dY W = dY (W^T)^T
            else:
                dx = dy2.mm(weight).view(ctx.x_shape)
        if ctx.needs_input_grad[1]:
            dw = dy2.t().mm(x2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = colsum(dy2)
        return dx, dw, db


def _x6_planes(kind, x, *weights, gate=None):
    """The current planes of every weight (a tuple), when "auto" puts this layer on the x6 forms; else None."""
    if GEMM_MODE != "auto" or not X6_LINEAR or kind not in X6_AUTO_KINDS or torch.is_autocast_enabled():
        return None
    if not x.is_cuda or x.dtype != torch.float32 or x.numel() == 0 or x.shape[-1] % 4:
        return None
    if kind == "linear" and min(weights[0].shape) < 128:
        # a lone Linear under 128 features either way (the quant layers, 256 <-> 32) stays where it was: its weight gradient
        # would move from the library to dense.gemm_tn, whose tiles are 128 wide (+0.4 ms per step in the kernel trace,
        # profiles/x6_linear_step_breakdown.log), for a forward of a few microseconds
        return None
    out = []
    for w in weights:
        pl = getattr(w, "_amk_x6", None)
        if pl is None or w._version != w._amk_x6_version or pl.gate != (w is gate) or (pl.R, pl.K) != tuple(w.shape):
            return None   # none kept, or the weight was written in place since (load_state_dict, manual init)
        out.append(pl)
    return tuple(out)


class _X6Linear(torch.autograd.Function):
    """_DenseLinear with the forward and dX = dY W on the split-bf16 GEMM against the weight's kept planes (those of W^T
    for dX); dW and db from _x6_tn (dense.gemm_x6_tn with the "dw" form, else dense.gemm_tn, exact f32), written into the
    reducer's buckets."""

    @staticmethod
    def forward(ctx, x, weight, bias, pl):
        from . import dense

        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, weight)
        ctx.x_shape, ctx.has_bias, ctx.params, ctx.pl = x.shape, bias is not None, (weight, bias), pl
        return dense.gemm_x6_nt(x2, pl.w, pl.R, bias).view(*x.shape[:-1], pl.R)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from . import dense

        x2, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dense.gemm_x6_nt(dy2, ctx.pl.wt, ctx.pl.K) if ctx.pl.wt is not None else _nn_plain(dy2, weight)).view(ctx.x_shape)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            want_b = ctx.has_bias and ctx.needs_input_grad[2]
            dw, db = _tn_into(_x6_tn, dy2, x2, ctx.params[0], ctx.params[1] if want_b else None)
        return dx, dw, db, None


class _X6Linear2(torch.autograd.Function):
    """_DenseLinear2 on the kept planes: (x Wa^T, x Wb^T); dX = dA Wa + dB Wb as one launch over two contraction
    segments; (dWa, dWb) from one launch of _x6_tn, as there from dense.gemm_tn."""

    @staticmethod
    def forward(ctx, x, wa, wb, pa, pb):
        from . import dense

        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, wa, wb)
        ctx.x_shape, ctx.params, ctx.pl = x.shape, (wa, wb), (pa, pb)
        if X6_SHORT_K_MAX >= x2.shape[1] and _lib.load().amk_gemm_x6_short_k(-1):
            a, b = dense.gemm_x6_nt_cols2(x2, pa.w, pa.R, pb.w, pb.R)   # one launch: x2 is read and split once
        else:
            a, b = dense.gemm_x6_nt(x2, pa.w, pa.R), dense.gemm_x6_nt(x2, pb.w, pb.R)
        return a.view(*x.shape[:-1], pa.R), b.view(*x.shape[:-1], pb.R)

    @staticmethod
    @once_differentiable
    def backward(ctx, da, db_):
        from . import dense

        x2, wa, wb = ctx.saved_tensors
        pa, pb = ctx.pl
        da2 = da.reshape(-1, da.shape[-1])
        db2 = db_.reshape(-1, db_.shape[-1])
        dx = None
        if ctx.needs_input_grad[0]:
            dx = (dense.gemm_x6_nt(da2, pa.wt, pa.K, a2=db2, planes2=pb.wt) if pa.wt is not None and pb.wt is not None
                  else dense.gemm_nn(da2, wa, a2=db2, w2=wb)).view(ctx.x_shape)
        dwa = dwb = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            (ar, av), (br, bv) = _claim(ctx.params[0]), _claim(ctx.params[1])
            dwa, dwb, _ = _x6_tn(da2, x2, y2=db2, out=av, out2=bv)
            if av is not None:
                ar.wrote(ctx.params[0])
                dwa = None
            if bv is not None:
                br.wrote(ctx.params[1])
                dwb = None
        return dx, dwa, dwb, None, None


class _X6SwiGLUFFN(torch.autograd.Function):
    """_SwiGLUFFN on the kept planes: the gate in the epilogue of the w12 product (w12's planes in the gate order; (a | b)
    written only when a backward will read it), w3, dGate = dOut W3 with the gate's derivative in its epilogue and
    dX = d(a | b) W12 on the split-bf16 GEMM; the four weight / bias gradients from _x6_tn."""

    @staticmethod
    def forward(ctx, x, w12, b12, w3, b3, p12, p3):
        from . import dense

        x2 = x.reshape(-1, x.shape[-1])
        need = any(ctx.needs_input_grad)
        gate, ab = dense.gemm_x6_nt_swiglu(x2, p12.w, p12.R // 2, b12, keep_ab=need)
        out = dense.gemm_x6_nt(gate, p3.w, p3.R, b3)
        if need:
            ctx.save_for_backward(x2, w12, w3, ab, gate)
        ctx.x_shape, ctx.has_bias, ctx.params, ctx.pl = x.shape, (b12 is not None, b3 is not None), (w12, b12, w3, b3), (p12, p3)
        return out.view(*x.shape[:-1], p3.R)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        from . import dense

        x2, w12, w3, ab, gate = ctx.saved_tensors
        p12, p3 = ctx.pl
        d2 = dout.reshape(-1, dout.shape[-1])
        d_ab = dense.gemm_x6_nt_swiglu_bwd(d2, p3.wt, ab) if p3.wt is not None else dense.gemm_nn(d2, w3, swiglu_ab=ab)
        dw3, db3 = _tn_into(_x6_tn, d2, gate, ctx.params[2], ctx.params[3] if ctx.has_bias[1] else None)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = (dense.gemm_x6_nt(d_ab, p12.wt, p12.K) if p12.wt is not None else _nn_plain(d_ab, w12)).view(ctx.x_shape)
        dw12, db12 = _tn_into(_x6_tn, d_ab, x2, ctx.params[0], ctx.params[1] if ctx.has_bias[0] else None)
        return dx, dw12, db12, dw3, db3, None, None


# Dense GEMMs of the nn.Linear layers, default path: csrc/gemm_f32.hip (amk_gemm_f32) -- the forward with the bias in
# its epilogue, the weight gradient with the bias gradient (column sums of dY) inside the same product, q and kv
# projections as one launch, the SwiGLU gate of the FFN in the w12 GEMM's epilogue and its derivative in the epilogue
# of the w3 input gradient.  DENSE_MODE (AMK_DENSE): "amk" = every product on amk_gemm_f32; "auto" (default) = the
# plain input gradient dY W and forwards with fewer than 512 output columns stay with the vendor library where that is
# the faster kernel (measured, tools/kbench_dense.py: 0.80-0.96x), everything else on amk_gemm_f32; "lib" = the
# round-2 path (library GEMMs + amk_colsum / amk_swiglu launches).
DENSE_MODE = os.environ.get("AMK_DENSE", "auto")


# `auto` keeps the own kernels to contractions of at most this many input features.  They were built for (and win or tie
# on) the ViT-VQGAN layers, K = 256 / 512: short contractions, where the vendor kernels are epilogue-dominated and the
# persistent walk hides the epilogue.  At K >= 1024 -- the ViT classifier of configs[1], the ViTMoE projections -- the tuned
# vendor kernels are 10-45 % faster (tools/kbench_vit.py: 7.5 against 9.8 ms per step at batch 64; tools/scratch/dense_z_probe.py).
DENSE_AUTO_MAX_K = int(os.environ.get("AMK_DENSE_MAX_K", "512"))


def _dense_ok(x, *weights):
    if DENSE_MODE == "lib" or torch.is_autocast_enabled() or not x.is_cuda or x.dtype != torch.float32 or x.numel() == 0:
        return False
    if x.shape[-1] % 4 or x.shape[-1] < 128:
        return False
    if DENSE_MODE == "auto" and x.shape[-1] > DENSE_AUTO_MAX_K:
        return False
    return all(w.dtype == torch.float32 and w.shape[0] % 4 == 0 and w.shape[0] >= 128 and w.is_contiguous() for w in weights)


def _nn_plain(dy2, weight):
    """dY W: the one product the library still wins on the step's shapes."""
    from . import dense

    if DENSE_MODE == "amk":
        return dense.gemm_nn(dy2, weight)
    return dy2.mm(weight)


def _claim(p):
    """(reducer, view): the gradient view of amk.dp.GradReducer(direct_grads=True) to write parameter p's gradient into,
    when this is its first gradient of the step -- else (None, None) and the caller returns a tensor for autograd."""
    ref = getattr(p, "_amk_reducer", None) if p is not None else None
    red = ref() if ref is not None else None
    if red is None:
        return None, None
    view = red.claim(p)
    return (red, view) if view is not None else (None, None)


class _DenseLinear(torch.autograd.Function):
    """F.linear on amk_gemm_f32: forward NT (+ bias), dX = dY W, dW = dY^T X with db = colsum(dY) in the same launch."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import dense

        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, weight)
        ctx.x_shape = x.shape
        ctx.has_bias = bias is not None
        ctx.params = (weight, bias)
        if DENSE_MODE == "auto" and weight.shape[0] < 512:
            # outputs of one or two column tiles (W_o, w3, patch / quant layers: one tile per workgroup, nothing for the
            # persistent walk to overlap): the library's kernel is 5-10 % faster there (tools/kbench_dense.py)
            return torch.nn.functional.linear(x, weight, bias)
        return dense.gemm_nt(x2, weight, bias).view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from . import dense

        x2, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _nn_plain(dy2, weight).view(ctx.x_shape)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            want_b = ctx.has_bias and ctx.needs_input_grad[2]
            (wr, wv), (br, bv) = _claim(ctx.params[0]), (_claim(ctx.params[1]) if want_b else (None, None))
            dw, _, db = dense.gemm_tn(dy2, x2, want_bias=want_b, out=wv, bias_out=bv)
            if wv is not None:
                wr.wrote(ctx.params[0])
                dw = None
            if bv is not None:
                br.wrote(ctx.params[1])
                db = None
        return dx, dw, db


def _tn_into(tn, y, x, weight, bias):
    """(dW, db) of a Linear layer by `tn` (dense.gemm_tn / gemm_tn_bf16), written straight into the reducer's gradient views
    where they can be claimed (those come back as None: nothing for autograd to add)."""
    (wr, wv), (br, bv) = _claim(weight), _claim(bias)
    res = tn(y, x, want_bias=bias is not None, out=wv, bias_out=bv)
    dw, db = res[0], res[-1]
    if wv is not None:
        wr.wrote(weight)
        dw = None
    if bv is not None:
        br.wrote(bias)
        db = None
    return dw, db


class _DenseLinear2(torch.autograd.Function):
    """Two bias-free projections of the same input (q and kv of SoftmaxAttention) as one launch each way:
    (x Wa^T, x Wb^T); dX = dA Wa + dB Wb as one contraction in two segments; (dWa, dWb) from one launch."""

    @staticmethod
    def forward(ctx, x, wa, wb):
        from . import dense

        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, wa, wb)
        ctx.x_shape = x.shape
        ctx.params = (wa, wb)
        a, b = dense.gemm_nt(x2, wa, None, w2=wb)
        return a.view(*x.shape[:-1], wa.shape[0]), b.view(*x.shape[:-1], wb.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, da, db_):
        from . import dense

        x2, wa, wb = ctx.saved_tensors
        da2 = da.reshape(-1, da.shape[-1])
        db2 = db_.reshape(-1, db_.shape[-1])
        dx = dense.gemm_nn(da2, wa, a2=db2, w2=wb).view(ctx.x_shape) if ctx.needs_input_grad[0] else None
        dwa = dwb = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            (ar, av), (br, bv) = _claim(ctx.params[0]), _claim(ctx.params[1])
            dwa, dwb, _ = dense.gemm_tn(da2, x2, y2=db2, out=av, out2=bv)
            if av is not None:
                ar.wrote(ctx.params[0])
                dwa = None
            if bv is not None:
                br.wrote(ctx.params[1])
                dwb = None
        return dx, dwa, dwb


class _SwiGLUFFN(torch.autograd.Function):
    """w3(silu(a) * b) with (a | b) = w12(x) (models/vitvqgan.py:20-34 as built, see amk/models/vitvqgan.py): the gate in
    the epilogue of the w12 product ((a | b) is written only when a backward will read it), its derivative in the epilogue
    of dGate = dOut W3, both bias gradients inside the weight-gradient products: six launches forward + backward where
    the separate form took eighteen."""

    @staticmethod
    def forward(ctx, x, w12, b12, w3, b3):
        from . import dense

        x2 = x.reshape(-1, x.shape[-1])
        need = any(ctx.needs_input_grad)
        gate, ab = dense.gemm_nt_swiglu(x2, w12, b12, keep_ab=need)
        out = dense.gemm_nt(gate, w3, b3)
        if need:
            ctx.save_for_backward(x2, w12, w3, ab, gate)
        ctx.x_shape = x.shape
        ctx.has_bias = (b12 is not None, b3 is not None)
        ctx.params = (w12, b12, w3, b3)
        return out.view(*x.shape[:-1], w3.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        from . import dense

        x2, w12, w3, ab, gate = ctx.saved_tensors
        d2 = dout.reshape(-1, dout.shape[-1])
        d_ab = dense.gemm_nn(d2, w3, swiglu_ab=ab)
        dw3, db3 = _tn_into(dense.gemm_tn, d2, gate, ctx.params[2], ctx.params[3] if ctx.has_bias[1] else None)
        dx = _nn_plain(d_ab, w12).view(ctx.x_shape) if ctx.needs_input_grad[0] else None
        dw12, db12 = _tn_into(dense.gemm_tn, d_ab, x2, ctx.params[0], ctx.params[1] if ctx.has_bias[0] else None)
        return dx, dw12, db12, dw3, db3


# AMK_MIXED_WGRAD=0: nn.Linear under bf16 autocast entirely by the library and autograd (the round-2 behaviour).
MIXED_WGRAD = os.environ.get("AMK_MIXED_WGRAD", "1") == "1"


def _w16(t):
    """The bf16 copy of a parameter: the one FlatAdam(bf16_shadow=True) keeps current, else a cast."""
    if t is None:
        return None
    shadow = getattr(t, "_amk_bf16", None)
    if shadow is not None and t._version == t._amk_bf16_version:
        return shadow
    return t.to(torch.bfloat16)   # no copy kept, or the parameter was written in place since (load_state_dict, init): cast


class _LinearMixed(torch.autograd.Function):
    """nn.Linear under bf16 autocast: forward and input gradient by the library's bf16 GEMMs as autocast runs them,
    weight and bias gradient by amk_gemm_tn_bf16 -- one pass over dY and X, f32 results (csrc/gemm_bf16.hip; the library
    runs these products at 50-180 TFLOP/s, rounds dW to bf16 and leaves db to a separate reduction)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x16, w16 = x.to(torch.bfloat16), _w16(weight)
        ctx.save_for_backward(x16, w16)
        ctx.has_bias, ctx.x_dtype = bias is not None, x.dtype
        ctx.params = (weight, bias)
        return torch.nn.functional.linear(x16, w16, _w16(bias))

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from . import dense

        x16, w16 = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dx = dy2.mm(w16).view(x16.shape).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
        dw, db = _tn_into(dense.gemm_tn_bf16, dy2, x16.reshape(-1, x16.shape[-1]), ctx.params[0], ctx.params[1])
        return dx, dw, db


def _mixed_linear_ok(x, weight):
    return (MIXED_WGRAD and x.is_cuda and torch.get_autocast_dtype("cuda") == torch.bfloat16 and torch.is_grad_enabled()
            and weight.requires_grad and weight.dtype == torch.float32 and x.dtype in (torch.float32, torch.bfloat16)
            and weight.shape[0] % 8 == 0 and weight.shape[1] % 8 == 0 and x.numel() > 0)


def linear(x, weight, bias=None):
    if torch.is_autocast_enabled():  # mixed precision: the library GEMMs in the autocast dtype, own weight gradient
        if _mixed_linear_ok(x, weight):
            return _LinearMixed.apply(x, weight, bias)
        return torch.nn.functional.linear(x, weight, bias)
    if GEMM_MODE == "bf16x6" and _x6_ok(x, weight):
        return _LinearX6.apply(x, weight, bias)
    pl = _x6_planes("linear", x, weight)
    if pl is not None:
        return _X6Linear.apply(x, weight, bias, pl[0])
    if _dense_ok(x, weight):
        return _DenseLinear.apply(x, weight, bias)
    if bias is None:
        return torch.nn.functional.linear(x, weight)
    return _BiasLinear.apply(x, weight, bias)


def linear2(x, wa, wb):
    """(F.linear(x, wa), F.linear(x, wb)) -- one launch when the shapes allow (wa.shape[0] a multiple of 128)."""
    pl = _x6_planes("linear2", x, wa, wb) if wa.shape[0] % 128 == 0 else None
    if pl is not None:
        return _X6Linear2.apply(x, wa, wb, *pl)
    if GEMM_MODE != "bf16x6" and _dense_ok(x, wa, wb) and wa.shape[0] % 128 == 0:
        return _DenseLinear2.apply(x, wa, wb)
    return linear(x, wa), linear(x, wb)


class _SwiGLUFFNMixed(torch.autograd.Function):
    """The SwiGLU FFN under bf16 autocast (models/vitvqgan.py:20-34 under cfg/vitvqgan.yaml:73): w12 with the gate in its
    epilogue (amk_gemm_bf16, epi 1: (a | b) and silu(a) b from one launch), the gate's input gradient dY W3 by
    amk_gemm_bf16 (op 1), both weight / bias gradients by amk_gemm_tn_bf16; w3's forward and w12's input gradient stay
    on the library, which is faster on those two shapes (tools/kbench_tn_bf16.py)."""

    @staticmethod
    def forward(ctx, x, w12, b12, w3, b3):
        from . import dense

        x16 = x.to(torch.bfloat16).reshape(-1, x.shape[-1])
        w12h, w3h = _w16(w12), _w16(w3)
        g, ab = dense.gemm_nt_swiglu_bf16(x16, w12h, b12)
        y = torch.nn.functional.linear(g, w3h, _w16(b3))
        ctx.save_for_backward(x16, ab, g, w12h, w3h)
        ctx.x_shape, ctx.x_dtype, ctx.bias = x.shape, x.dtype, (b12 is not None, b3 is not None)
        ctx.params = (w12, b12, w3, b3)
        return y.view(*x.shape[:-1], w3.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from . import dense

        x16, ab, g, w12h, w3h = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dw3, db3 = _tn_into(dense.gemm_tn_bf16, dy2, g, ctx.params[2], ctx.params[3])
        dab = dense.gemm_nn_swiglu_bwd_bf16(dy2, w3h, ab)   # dY W3 with the gate's backward in its epilogue
        dw12, db12 = _tn_into(dense.gemm_tn_bf16, dab, x16, ctx.params[0], ctx.params[1])
        dx = dab.mm(w12h).view(ctx.x_shape).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
        return dx, dw12, db12, dw3, db3


def swiglu_ffn(x, w12, b12, w3, b3):
    """w3(silu(a) * b), (a | b) = w12(x): fused (see _SwiGLUFFN) when the shapes allow, else the separate launches."""
    if torch.is_autocast_enabled() and w12.shape[0] % 16 == 0 and w12.shape[0] >= 1024:
        if _mixed_linear_ok(x, w12) and _mixed_linear_ok(x, w3) and w3.requires_grad:
            with torch.autocast("cuda", enabled=False):
                return _SwiGLUFFNMixed.apply(x, w12, b12, w3, b3)
        no_grad = not torch.is_grad_enabled() or not any(
            t is not None and t.requires_grad for t in (x, w12, b12, w3, b3))   # (e.g. the generator's forward in the D phase)
        if (MIXED_WGRAD and no_grad and x.is_cuda and torch.get_autocast_dtype("cuda") == torch.bfloat16
                and w12.dtype == torch.float32 and x.dtype in (torch.float32, torch.bfloat16) and w12.shape[1] % 8 == 0 and x.numel()):
            from . import dense   # inference: the gate only, the pre-activations never reach HBM

            g, _ = dense.gemm_nt_swiglu_bf16(x.to(torch.bfloat16).reshape(-1, x.shape[-1]), _w16(w12), b12, keep_ab=False)
            return torch.nn.functional.linear(g, _w16(w3), _w16(b3)).view(*x.shape[:-1], w3.shape[0])
    pl = _x6_planes("ffn", x, w12, w3, gate=w12) if not torch.is_autocast_enabled() else None
    if pl is not None:
        return _X6SwiGLUFFN.apply(x, w12, b12, w3, b3, *pl)
    if GEMM_MODE != "bf16x6" and _dense_ok(x, w12) and w3.shape[1] % 4 == 0 and w3.shape[0] % 4 == 0 and w3.is_contiguous():
        return _SwiGLUFFN.apply(x, w12, b12, w3, b3)
    ab = linear(x, w12, b12)
    if ab.shape[-1] % 8 == 0:
        return linear(swiglu(ab), w3, b3)
    a, b = ab.chunk(2, dim=-1)
    return linear(torch.nn.functional.silu(a) * b, w3, b3)


# ---------------------------------------------------------------------------- GEGLU + LayerNorm FFN (bf16 autocast)
# AMK_GEGLU_FFN_BF16: the transformer FFN (models/transformer.py:22-43) under bf16 autocast as one Function: both Linear
# layers on the bf16 shadow weights with f32 weight gradients by amk_gemm_tn_bf16, and the gate + LayerNorm between them as
# one row-wise kernel each way (csrc/geglu_ln_bf16.hip) in place of an upcast copy, the f32 gate, the f32 LayerNorm and a
# downcast copy.  Measured at the Muse decoder's FFN (8192 rows, dim 1024, inner 4096; tools/kbench_geglu_ffn.py,
# profiles/kbench_geglu_ffn.log): 0.79 ms against 1.28 ms forward + backward (spread 0.01 ms), 612 MB against 923 MB of peak
# memory above the inputs; bench.py --model muse --autocast bf16 52.1 against 63.9 ms per step on the parent commit
# (profiles/bench_muse_geglu_ffn_bf16.log).  So the switch ships on.  Read once per process.
GEGLU_FFN_BF16 = os.environ.get("AMK_GEGLU_FFN_BF16", "1") != "0"


def geglu_ln_bf16_fwd(ab2, gamma, beta, eps=1e-5):
    """(y bf16 (M, H), mean, rstd f32 (M)) of LayerNorm(gate * gelu(val)) for ab2 = (val | gate), an (M, 2H) bf16 matrix
    with unit column stride (any row stride the kernel takes)."""
    M, H = ab2.shape[0], ab2.shape[1] // 2
    y = torch.empty((M, H), device=ab2.device, dtype=torch.bfloat16)
    mean = torch.empty((M,), device=ab2.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    with _timed(f"geglu_ln_bf16_fwd M{M} H{H}"):
        _lib.check(_lib.load().amk_geglu_ln_bf16_fwd(_ptr(ab2), ab2.stride(0), M, H, _ptr(gamma), _ptr(beta), float(eps),
                                                     _ptr(y), _ptr(mean), _ptr(rstd), _stream()), "amk_geglu_ln_bf16_fwd")
    return y, mean, rstd


def geglu_ln_bf16_bwd(ab2, dy, gamma, mean, rstd):
    """(d_ab bf16 (M, 2H), partial sums (parts, 2, H) f32 of dgamma / dbeta) -- the backward of geglu_ln_bf16_fwd."""
    M, H = ab2.shape[0], ab2.shape[1] // 2
    L = _lib.load()
    d_ab = torch.empty((M, 2 * H), device=ab2.device, dtype=torch.bfloat16)
    part = torch.empty((L.amk_geglu_ln_bf16_num_partials(M, H), 2, H), device=ab2.device, dtype=torch.float32)
    with _timed(f"geglu_ln_bf16_bwd M{M} H{H}"):
        _lib.check(L.amk_geglu_ln_bf16_bwd(_ptr(ab2), ab2.stride(0), _ptr(dy), _ptr(gamma), _ptr(mean), _ptr(rstd), M, H,
                                           _ptr(d_ab), _ptr(part), _stream()), "amk_geglu_ln_bf16_bwd")
    return d_ab, part


class _GEGLUFFNMixed(torch.autograd.Function):
    """w2(LN(gate * gelu(val))), (val | gate) = w1(x), under bf16 autocast: w1 and w2 forward and the two input gradients
    on the library's bf16 GEMMs, gate + LayerNorm by amk_geglu_ln_bf16_fwd / _bwd, both weight gradients in f32 by
    amk_gemm_tn_bf16.  Kept for the backward: x, (val | gate) and the LayerNorm's output in bf16, mean and rstd."""

    @staticmethod
    def forward(ctx, x, w1, gamma, beta, w2, eps):
        x16 = x.to(torch.bfloat16).reshape(-1, x.shape[-1])
        w1h, w2h = _w16(w1), _w16(w2)
        gm, bt = gamma.contiguous(), beta.contiguous()
        ab = torch.nn.functional.linear(x16, w1h)
        y, mean, rstd = geglu_ln_bf16_fwd(ab, gm, bt, eps)
        out = torch.nn.functional.linear(y, w2h)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x16, ab, y, mean, rstd, w1h, w2h, gm)
        ctx.x_shape, ctx.x_dtype = x.shape, x.dtype
        ctx.params = (w1, gamma, beta, w2)
        return out.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from . import dense

        x16, ab, y, mean, rstd, w1h, w2h, gm = ctx.saved_tensors
        w1, gamma, beta, w2 = ctx.params
        dy2 = dy.to(torch.bfloat16).reshape(-1, dy.shape[-1])
        dw2, _ = _tn_into(dense.gemm_tn_bf16, dy2, y, w2, None)
        dyn = dy2.mm(w2h)
        d_ab, part = geglu_ln_bf16_bwd(ab, dyn, gm, mean, rstd)
        dgamma, dbeta = _ln_param_grads(part, (gamma, beta if ctx.needs_input_grad[3] else None))
        dw1, _ = _tn_into(dense.gemm_tn_bf16, d_ab, x16, w1, None)
        dx = d_ab.mm(w1h).view(ctx.x_shape).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
        return dx, dw1, dgamma, (dbeta if ctx.needs_input_grad[3] else None), dw2, None


def geglu_ffn_ok(x, w1, gamma, beta, w2):
    """The gate of the fused FFN: the switch and bf16 autocast are on, HIP tensors, f32 master weights that both take a
    gradient (or nothing does), x f32 or bf16, dim and inner multiples of 8, 8 <= inner <= 4096, x not empty."""
    if not (GEGLU_FFN_BF16 and x.is_cuda and w1.is_cuda and w2.is_cuda and _bf16_autocast()):
        return False
    inner, dim = w2.shape[1], w2.shape[0]
    if not (w1.dtype == torch.float32 and w2.dtype == torch.float32 and gamma.dtype == torch.float32 and beta.dtype == torch.float32
            and x.dtype in (torch.float32, torch.bfloat16) and tuple(w1.shape) == (2 * inner, dim) and x.shape[-1] == dim
            and dim % 8 == 0 and inner % 8 == 0 and 8 <= inner <= 4096 and x.numel() > 0):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, w1, gamma, beta, w2)):
        return w1.requires_grad and w2.requires_grad
    return True


def geglu_ffn(x, w1, gamma, beta, w2, eps=1e-5):
    """w2(LayerNorm(gate * gelu(val)) * gamma + beta) with (val | gate) = w1(x), no biases: the transformer FFN.  Fused
    (see _GEGLUFFNMixed) when geglu_ffn_ok, else the separate ops; on CPU tensors plain PyTorch."""
    if geglu_ffn_ok(x, w1, gamma, beta, w2):
        with torch.autocast("cuda", enabled=False):
            return _GEGLUFFNMixed.apply(x, w1, gamma, beta, w2, eps)
    ab = torch.nn.functional.linear(x, w1)
    if ab.is_cuda and ab.shape[-1] % 8 == 0 and ab.numel() > 0:
        g = geglu(ab)
    else:
        val, gate = ab.chunk(2, dim=-1)
        g = gate * torch.nn.functional.gelu(val)
    return torch.nn.functional.linear(layer_norm(g, gamma, beta, eps), w2)


# ---------------------------------------------------------------------------- guided logits head of the parallel decode
# AMK_GUIDED_HEAD (default 1): under bf16 autocast MUSE.generate, parallel_decode and MaskGitTransformer.generate take the
# logits of each step from the decoder's hidden states by guided_logits below -- classifier-free guidance applied to the
# normalised activations (the head's Linear has no bias and the guidance is linear in the logits), one bf16 product with
# f32 logits, and the sampler on those.  0: the decode under autocast is what it was before this head existed: with
# fused_sampling it raises ("amk kernels compute in fp32"), without it the torch chain runs on bf16 logits.  Measurements:
# DESIGN.md section 4g.1, profiles/kbench_muse_generate.log.  Read once per process.
GUIDED_HEAD = os.environ.get("AMK_GUIDED_HEAD", "1") != "0"


def guided_logits_ok(h, weight):
    """The models' gate for guided_logits: the switch and bf16 autocast are on, HIP tensors, hidden states in f32 or bf16,
    an f32 master weight (V, dim) with dim and V multiples of 8, and a width the LayerNorm kernel takes."""
    if not (GUIDED_HEAD and h.is_cuda and weight.is_cuda and _bf16_autocast()):
        return False
    dim = h.shape[-1]
    return (weight.dtype == torch.float32 and h.dtype in (torch.float32, torch.bfloat16) and weight.dim() == 2
            and weight.shape[1] == dim and dim % 8 == 0 and weight.shape[0] % 8 == 0 and _ln_supported(dim) and h.numel() > 0)


def guided_logits(h, gamma, beta, weight, null_h=None, cfg_scale=3.0, eps=1e-5, w16=None):
    """f32 logits (..., V) of the parallel decode's head from the decoder's hidden states h (..., dim), f32 or bf16:
    weight @ (LN(null_h) + cfg_scale (LN(h) - LN(null_h))) with the LayerNorms and the combination in f32, rounded to bf16
    once (amk_cfg_layernorm_bf16), then one bf16 product whose f32 accumulators are the result (amk_gemm_bf16_f32out).
    null_h None: weight @ LN(h).  w16: a bf16 copy of weight the caller made once; else the optimizer's shadow if it is
    current, else a cast.  Inference only, no autograd; runs with autocast disabled inside."""
    if not (h.is_cuda and weight.is_cuda):
        raise RuntimeError("amk ops run only on MI355X (HIP) tensors; got a CPU tensor. There is no CPU fallback.")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (h, null_h, gamma, beta, weight)):
        raise RuntimeError("guided_logits is inference only: it has no backward; call it under torch.no_grad()")
    V, dim = weight.shape
    if h.shape[-1] != dim or dim % 8 or V % 8 or not _ln_supported(dim) or (null_h is not None and null_h.shape != h.shape):
        raise RuntimeError(f"guided_logits: hidden {tuple(h.shape)}, weight {tuple(weight.shape)}: dim and V must be multiples "
                           "of 8, dim at most 4096, and both hidden states of one shape")
    with torch.autocast("cuda", enabled=False):
        if w16 is None:
            w16 = _w16(weight.detach())
        if w16.dtype != torch.bfloat16 or tuple(w16.shape) != (V, dim):
            raise RuntimeError(f"guided_logits: w16 must be the bf16 copy of weight; got {w16.dtype} {tuple(w16.shape)}")
        w16 = _row_major_view(w16, 8)

        def rows(t):
            if t.dtype not in (torch.float32, torch.bfloat16):
                raise RuntimeError(f"guided_logits: hidden states in f32 or bf16; got {t.dtype}")
            t2 = t.detach().reshape(-1, dim)
            return t2 if t2.is_contiguous() and t2.data_ptr() % 16 == 0 else t2.contiguous().clone()

        hc = rows(h)
        hn = rows(null_h) if null_h is not None else None
        gm, bt = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        M = hc.shape[0]
        L = _lib.load()
        u = torch.empty((M, dim), device=h.device, dtype=torch.bfloat16)
        with _timed(f"cfg_layernorm_bf16 M{M} D{dim}"):
            rc = L.amk_cfg_layernorm_bf16(_ptr(hc), int(hc.dtype == torch.bfloat16), _ptr(hn),
                                          int(hn is not None and hn.dtype == torch.bfloat16), _ptr(gm), _ptr(bt),
                                          float(cfg_scale), M, dim, float(eps), _ptr(u), _stream())
        _lib.check(rc, "amk_cfg_layernorm_bf16")
        logits = torch.empty((M, V), device=h.device, dtype=torch.float32)
        with _timed(f"gemm_bf16_f32out N{V} K{dim}"):
            rc = L.amk_gemm_bf16_f32out(_ptr(u), dim, _ptr(w16), w16.stride(0), _NULL, _ptr(logits), V, M, V, dim, _stream())
        _lib.check(rc, "amk_gemm_bf16_f32out")
    return logits.view(*h.shape[:-1], V)


# ---------------------------------------------------------------------------- discriminator BatchNorm + LeakyReLU
# AMK_DISCR_NORM: "amk" (default) = the training-mode BatchNorm2d + LeakyReLU pairs of NLayerDiscriminator run on
# csrc/discr_norm.hip (forward, backward and the gradient penalty's double backward); "aten" = the modules as they are
# (MIOpen batch norm, ATen's leaky_relu and its composite double backward).  Read per call, so one build A/Bs.
def discr_norm_mode():
    return os.environ.get("AMK_DISCR_NORM", "amk")


def _bn_dims(x):
    N, C, H, W = x.shape
    return N, C, H * W


def _bn_ws(x):
    N, C, HW = _bn_dims(x)
    return torch.empty(int(_lib.load().amk_bnact_ws_floats(N, C, HW)), device=x.device, dtype=torch.float32)


def _bn_f32(t):
    return None if t is None else t.to(torch.float32).contiguous()


# The op's two element types: (dtype of the (N, C, HW) tensors, forward, backward, double backward).  The parameters, the
# statistics, the kept sums and the workspace (amk_bnact_ws_floats) are f32 in both.
_BN_F32 = (torch.float32, "amk_bnact_fwd", "amk_bnact_bwd", "amk_bnact_bwd_bwd")
_BN_BF16 = (torch.bfloat16, "amk_bnact_bf16_fwd", "amk_bnact_bf16_bwd", "amk_bnact_bf16_bwd_bwd")


class _BNActGrad(torch.autograd.Function):
    """(gx, dgamma, dbeta) of z = leaky_relu(batch_norm(x), slope) for a given gz; differentiable in gz, x and gamma
    (its backward is the double backward the gradient penalty takes).  Incoming gradients are brought to the element
    dtype (gg_gamma / gg_beta to f32); a subclass sets ELEM."""
    ELEM = _BN_F32

    @classmethod
    def forward(cls, ctx, gz, x, weight, bias, mean, rstd, slope):
        ctx.elem = cls.ELEM
        dtype, _, bwd, _ = cls.ELEM
        gz = _c16(gz.to(dtype))
        N, C, HW = _bn_dims(x)
        gx = torch.empty_like(x)
        sums = torch.empty((2, C), device=x.device, dtype=torch.float32)
        dw = torch.empty_like(weight)
        db = torch.empty_like(bias)
        _lib.check(getattr(_lib.load(), bwd)(
            _ptr(gz), _ptr(x), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(rstd), N, C, HW, float(slope), _ptr(gx), _ptr(sums),
            _ptr(dw), _ptr(db), _ptr(_bn_ws(x)), _stream()), bwd)
        ctx.save_for_backward(gz, x, weight, bias, mean, rstd, sums)
        ctx.slope = slope
        ctx.set_materialize_grads(False)   # absent gradients of dgamma / dbeta cost nothing
        return gx, dw, db

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx, ggw, ggb):
        gz, x, weight, bias, mean, rstd, sums = ctx.saved_tensors
        if ggx is None and ggw is None and ggb is None:
            return None, None, None, None, None, None, None
        dtype, _, _, bwd_bwd = ctx.elem
        ggx = torch.zeros_like(x) if ggx is None else _c16(ggx.to(dtype))
        N, C, HW = _bn_dims(x)
        g_gz = torch.empty_like(x)
        g_x = torch.empty_like(x)
        g_w = torch.empty_like(weight) if ctx.needs_input_grad[2] else None
        _lib.check(getattr(_lib.load(), bwd_bwd)(
            _ptr(ggx), _ptr(_bn_f32(ggw)), _ptr(_bn_f32(ggb)), _ptr(gz), _ptr(x), _ptr(weight), _ptr(bias), _ptr(mean),
            _ptr(rstd), _ptr(sums), N, C, HW, float(ctx.slope), _ptr(g_gz), _ptr(g_x), _ptr(g_w), _ptr(_bn_ws(x)),
            _stream()), bwd_bwd)
        return (g_gz if ctx.needs_input_grad[0] else None, g_x if ctx.needs_input_grad[1] else None, g_w,
                None, None, None, None)


class _BNAct(torch.autograd.Function):
    """z = leaky_relu(batch_norm(x, training=True), slope) with the running statistics updated in place; a subclass sets
    GRAD, whose ELEM names the forward too."""
    GRAD = _BNActGrad

    @classmethod
    def forward(cls, ctx, x, weight, bias, running_mean, running_var, eps, momentum, slope):
        fwd = cls.GRAD.ELEM[1]
        N, C, HW = _bn_dims(x)
        z = torch.empty_like(x)
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        rstd = torch.empty(C, device=x.device, dtype=torch.float32)
        _lib.check(getattr(_lib.load(), fwd)(
            _ptr(x), _ptr(weight), _ptr(bias), N, C, HW, float(eps), float(momentum), float(slope), _ptr(z), _ptr(mean),
            _ptr(rstd), _ptr(running_mean), _ptr(running_var), _ptr(_bn_ws(x)), _stream()), fwd)
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        ctx.slope = slope
        ctx.set_materialize_grads(False)
        return z

    @classmethod
    def backward(cls, ctx, gz):
        if gz is None:
            return (None,) * 8
        x, weight, bias, mean, rstd = ctx.saved_tensors
        from .models.discriminator import input_grad_only_active   # (lazy: the models package imports this module)

        gx, dw, db = cls.GRAD.apply(gz, x, weight, bias, mean, rstd, ctx.slope)
        if input_grad_only_active():
            dw = db = None
        return (gx if ctx.needs_input_grad[0] else None, dw if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None, None, None, None, None, None)


def bn_leaky_relu_ok(bn, x):
    """True when (bn, LeakyReLU) can run on amk_bnact_*: training-mode statistics with running averages and an affine
    transform, an f32 contiguous NCHW HIP tensor outside autocast.  Everything else (eval, CPU, bf16 autocast) keeps
    the modules."""
    return (bn.training and bn.track_running_stats and bn.affine and bn.momentum is not None
            and bn.running_mean is not None and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous() and x.numel() > 0 and x.shape[0] * x.shape[2] * x.shape[3] > 1
            and not torch.is_autocast_enabled() and bn.weight.dtype == torch.float32)


def bn_leaky_relu(x, bn, slope):
    """leaky_relu(bn(x), slope) for a training-mode nn.BatchNorm2d (see bn_leaky_relu_ok)."""
    _require_device(x, bn.weight, bn.bias)
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BNAct.apply(_c16(x), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum,
                        float(slope))


# AMK_DISCR_NORM_BF16: the same pairs under bf16 autocast, where the convolution in front hands over a bf16 tensor and the
# modules run MIOpen's batch norm on it, ATen's leaky_relu_ / leaky_relu_backward and, for the gradient penalty, ATen's
# composite double backward.  "1" = amk_bnact_bf16_* (csrc/discr_norm.hip on bf16 x, z, gz, gx, ggx, g_gz and g_x: the f32
# arithmetic of the f32 kernels, one rounding to bf16 on each store; the bf16 x and f32 mean / rstd / sums saved); "0" = the
# modules.  Measured at batch 32, the whole GAN step under bf16 autocast with one captured step per arm replayed in turn
# (tools/kbench_autocast.py --step --ab AMK_DISCR_NORM_BF16, profiles/kbench_autocast_discr_norm_bf16.log): 36.83 ms with the
# modules, 34.16 ms fused, the arms' spreads 0.08 ms; the op alone (tools/kbench_discr_norm.py --bf16,
# profiles/kbench_discr_norm_bf16.log) 3.91 -> 1.68 ms over a step's calls.  So the switch ships on.
# AMK_DISCR_NORM=aten disables both.  Read per call, so one build A/Bs.
def discr_norm_bf16_on():
    return os.environ.get("AMK_DISCR_NORM_BF16", "1") != "0"


class _BNActGradBF16(_BNActGrad):
    """_BNActGrad on bf16 gz and x: gx bf16, rounded once; dgamma, dbeta and the kept sums f32.  Its backward is the double
    backward on bf16 ggx with bf16 g_gz and g_x and an f32 g_gamma."""
    ELEM = _BN_BF16


class _BNActBF16(_BNAct):
    """_BNAct on a bf16 x with f32 parameters: z bf16, rounded once; mean, rstd and the running statistics f32."""
    GRAD = _BNActGradBF16


def bn_leaky_relu_bf16_ok(bn, x):
    """True when (bn, LeakyReLU) can run on amk_bnact_bf16_*: both switches on, training-mode statistics with running
    averages, a momentum and an affine transform in f32, and a contiguous NCHW bf16 HIP tensor with more than one element per
    channel (what the convolution in front returns under bf16 autocast).  Everything else (eval, CPU, bf16 parameters, f16,
    non-contiguous or channels-last inputs) keeps the modules."""
    return (discr_norm_mode() == "amk" and discr_norm_bf16_on() and isinstance(bn, torch.nn.BatchNorm2d)
            and bn.training and bn.track_running_stats and bn.affine and bn.momentum is not None
            and bn.running_mean is not None and bn.running_mean.dtype == torch.float32
            and bn.weight.dtype == torch.float32 and bn.bias.dtype == torch.float32 and bn.weight.is_cuda
            and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous() and x.numel() > 0
            and x.shape[0] * x.shape[2] * x.shape[3] > 1)


def bn_leaky_relu_bf16(x, bn, slope):
    """leaky_relu(bn(x), slope) in bf16 for a training-mode nn.BatchNorm2d and a bf16 x (see bn_leaky_relu_bf16_ok)."""
    _require_device(bn.weight, bn.bias)
    if not x.is_cuda or x.dtype != torch.bfloat16:
        raise RuntimeError(f"bn_leaky_relu_bf16 takes a bf16 HIP tensor; got {x.dtype} on {x.device}")
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BNActBF16.apply(_c16(x), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum,
                            float(slope))


# ---------------------------------------------------------------------------- conv VQGAN GroupNorm + Swish
# AMK_GN_ACT: "1" (default) = the GroupNorm (+ Swish) of amk.models.vqgan runs on csrc/gn_act.hip (x, mean and rstd saved; y
# and sigma recomputed in the backward); "0" = nn.GroupNorm and x * sigmoid(x) as they are.  Measured on VQGAN(256, 8192),
# batch 8 at 256 px, forward + backward, the switch alternated in one process (tools/kbench_vqgan.py,
# profiles/kbench_vqgan.log): 79.8 ms with the modules, 73.7 ms fused, the arms' spreads 0.13 / 0.45 ms, peak memory 10.9 -> 7.5 GiB.  So the switch ships on.  Read once per process.
GN_ACT = os.environ.get("AMK_GN_ACT", "1") != "0"


# The op's two element types: (dtype of x, z, gz and gx, forward, backward, workspace query); an entry point's name less
# its "amk_" is its event's.  mean, rstd, the parameters and their gradients are f32 in both.
_GN_F32 = (torch.float32, "amk_gnact_fwd", "amk_gnact_bwd", "amk_gnact_ws_floats")
_GN_BF16 = (torch.bfloat16, "amk_gnact_bf16_fwd", "amk_gnact_bf16_bwd", "amk_gnact_bf16_ws_floats")


def _gn_ws(x, G, ws_floats):
    N, C, HW = _bn_dims(x)
    return torch.empty(int(getattr(_lib.load(), ws_floats)(N, C, HW, G)), device=x.device, dtype=torch.float32)


class _GNAct(torch.autograd.Function):
    """z = act(group_norm(x)), act 0 identity, 1 swish.  Saves x, mean and rstd (N, G); y and sigma are recomputed.  A
    subclass sets ELEM."""
    ELEM = _GN_F32

    @classmethod
    def forward(cls, ctx, x, weight, bias, G, eps, act):
        ctx.elem = cls.ELEM
        _, fwd, _, ws_floats = cls.ELEM
        N, C, HW = _bn_dims(x)
        z = torch.empty_like(x)
        mean = torch.empty((N, G), device=x.device, dtype=torch.float32)
        rstd = torch.empty((N, G), device=x.device, dtype=torch.float32)
        ws = _gn_ws(x, G, ws_floats)
        with _timed(fwd[4:]):
            _lib.check(getattr(_lib.load(), fwd)(_ptr(x), _ptr(weight), _ptr(bias), N, C, HW, G, float(eps), act, _ptr(z),
                                                 _ptr(mean), _ptr(rstd), _ptr(ws), _stream()), fwd)
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        ctx.G, ctx.act = G, act
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        x, weight, bias, mean, rstd = ctx.saved_tensors
        dtype, _, bwd, ws_floats = ctx.elem
        gz = _c16(gz.to(dtype))
        N, C, HW = _bn_dims(x)
        gx = torch.empty_like(x)
        dw = torch.empty_like(weight)
        db = torch.empty_like(bias)
        ws = _gn_ws(x, ctx.G, ws_floats)
        with _timed(bwd[4:]):
            _lib.check(getattr(_lib.load(), bwd)(_ptr(gz), _ptr(x), _ptr(weight), _ptr(bias), _ptr(mean), _ptr(rstd), N, C, HW,
                                                 ctx.G, ctx.act, _ptr(gx), _ptr(dw), _ptr(db), _ptr(ws), _stream()), bwd)
        return (gx if ctx.needs_input_grad[0] else None, dw if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None, None, None, None)


# AMK_GN_ACT_BF16: the same pair under bf16 autocast, where the modules cast the convolution's bf16 output to f32
# (group_norm is on autocast's f32 list), normalise, run sigmoid and mul as two more f32 passes, keep three f32 tensors for
# the backward and leave the cast back to bf16 to the next convolution.  "1" = amk_gnact_bf16_fwd / _bwd (csrc/gn_act.hip
# on bf16 x, z, gz and gx: the f32 arithmetic of the f32 kernels, one rounding to bf16 on the store; bf16 x and f32 mean /
# rstd saved); "0" = the modules.  Measured on VQGAN(256, 8192), batch 8 at 256 px under bf16 autocast, forward + backward, the
# switch alternated in one process (tools/kbench_vqgan.py --autocast bf16, profiles/kbench_vqgan_bf16.log): 51.98 ms with the
# modules, 39.59 ms fused, the arms' spreads 0.09 / 0.32 ms, peak memory 9.65 -> 3.97 GiB.  So the switch ships on.
# AMK_GN_ACT=0 disables both.  Read once per process.
GN_ACT_BF16 = os.environ.get("AMK_GN_ACT_BF16", "1") != "0"


class _GNActBF16(_GNAct):
    """_GNAct on bf16 x under bf16 autocast: z and gx bf16, rounded once; mean, rstd (N, G), dgamma and dbeta f32.  Saves the
    bf16 x, mean and rstd."""
    ELEM = _GN_BF16


def group_norm_act_bf16_ok(gn, x):
    """True when (gn, act) can run on amk_gnact_bf16_*: both switches on, autocast enabled on the device with dtype bf16, an
    nn.GroupNorm with f32 affine parameters on the device and a contiguous 4-D bf16 HIP tensor with at least one element.
    An f32 x under autocast, autocast to f16 and everything group_norm_act_ok refuses keep the modules."""
    return (GN_ACT and GN_ACT_BF16 and isinstance(gn, torch.nn.GroupNorm) and gn.affine
            and gn.weight.dtype == torch.float32 and gn.weight.is_cuda and x.is_cuda and x.dtype == torch.bfloat16
            and x.dim() == 4 and x.is_contiguous() and x.numel() > 0 and torch.is_autocast_enabled()
            and torch.get_autocast_dtype("cuda") == torch.bfloat16)


def group_norm_act_ok(gn, x):
    """True when (gn, act) can run on amk_gnact_*: an nn.GroupNorm with f32 affine parameters and a contiguous 4-D f32 HIP
    tensor with at least one element, outside autocast and with the switch on.  Everything else (CPU, autocast,
    non-contiguous input, AMK_GN_ACT=0) keeps the modules."""
    return (GN_ACT and isinstance(gn, torch.nn.GroupNorm) and gn.affine and gn.weight.dtype == torch.float32
            and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.numel() > 0
            and gn.weight.is_cuda and not torch.is_autocast_enabled())


def group_norm_act(x, gn, act):
    """act(gn(x)) for an nn.GroupNorm; act 0 = identity, 1 = swish x * sigmoid(x).

    The result is f32, except for a bf16 x under bf16 autocast that group_norm_act_bf16_ok accepts: there it is bf16 (the
    modules would return f32, which the convolution that consumes it casts to bf16: the same values, rounded in the same
    place)."""
    if act not in (0, 1):
        raise ValueError(f"group_norm_act: act must be 0 (identity) or 1 (swish), got {act}")
    if group_norm_act_bf16_ok(gn, x):
        return _GNActBF16.apply(_c16(x), gn.weight, gn.bias, gn.num_groups, gn.eps, act)
    if not group_norm_act_ok(gn, x):
        y = gn(x)
        return y * torch.sigmoid(y) if act == 1 else y
    return _GNAct.apply(_c16(x), gn.weight, gn.bias, gn.num_groups, gn.eps, act)


# ---------------------------------------------------------------------------- LPIPS distance head
# AMK_LPIPS: "1" = the per-level distance head of amk.models.lpips.LPIPS (unit-normalise both feature tensors over the
# channels, weight the squared difference with the level's 1x1 convolution, average over the pixels) runs on
# csrc/lpips.hip, forward and the gradient for the first tensor: two reads of each feature tensor forward, two reads and
# one write backward, three f32 numbers per pixel saved; "0" (default) = the torch chain (about a dozen memory-bound ops
# per level, several feature-sized tensors kept for the backward).  f32 features outside autocast, bf16 features under bf16
# autocast (amk_lpips_bf16_*; there the fused head returns f32 where the chain returns bf16).  Read once per process.
# Measured per head, forward + backward, arms alternating in one process (tools/kbench_lpips.py, profiles/kbench_lpips*.log):
# at batch 32 the five levels of a 256 px step take 1.95 ms fused against 9.04 ms in f32 (536 against 2 576 MiB above the
# inputs at level 1) and 1.45 against 9.97 ms under bf16 autocast.  The GAN step with the term on is NOT MEASURED: the
# step benchmark has not yet completed a run with finite losses, and the rule for this switch is a
# win at the step level, so it ships off.
LPIPS = os.environ.get("AMK_LPIPS", "0") != "0"


def _lpips_chain(a, b, w, eps):
    """The head as lpips 0.1.4 runs it: normalize_tensor on both, the squared difference, the 1x1 lin convolution,
    spatial_average.  (N,) in the dtype torch gives it."""
    na = torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True))
    nb = torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True))
    diff = (a / (na + eps) - b / (nb + eps)) ** 2
    return torch.nn.functional.conv2d(diff, w.reshape(1, -1, 1, 1).to(diff.dtype)).mean([2, 3]).reshape(-1)


class _LpipsDist(torch.autograd.Function):
    """out_n of the head for f32 (outside autocast) or bf16 (under bf16 autocast) features; differentiates with respect to
    a only.  Saves a, b, w and the three f32 rows (N, HW) the forward writes; a zero-norm pixel of a gets a zero gradient."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, a, b, w, eps):
        N, C, HW = _bn_dims(a)
        L = _lib.load()
        bf = a.dtype == torch.bfloat16
        f32 = dict(device=a.device, dtype=torch.float32)
        out, rows = torch.empty(N, **f32), torch.empty((3, N, HW), **f32)
        ws = torch.empty(int((L.amk_lpips_bf16_ws_floats if bf else L.amk_lpips_ws_floats)(N, C, HW)), **f32)
        name = "amk_lpips_bf16_fwd" if bf else "amk_lpips_fwd"
        with _timed(name[4:]):
            _lib.check(getattr(L, name)(_ptr(a), _ptr(b), _ptr(w), N, C, HW, float(eps), _ptr(out), _ptr(rows), _ptr(ws),
                                        _stream()), name)
        ctx.save_for_backward(a, b, w, rows)
        ctx.eps = float(eps)
        return out

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        a, b, w, rows = ctx.saved_tensors
        N, C, HW = _bn_dims(a)
        L = _lib.load()
        g = g.to(torch.float32).contiguous()
        ga = torch.empty_like(a)
        name = "amk_lpips_bf16_bwd" if a.dtype == torch.bfloat16 else "amk_lpips_bwd"
        with _timed(name[4:]):
            _lib.check(getattr(L, name)(_ptr(g), _ptr(a), _ptr(b), _ptr(w), _ptr(rows), N, C, HW, ctx.eps, _ptr(ga),
                                        _stream()), name)
        return ga, None, None, None


def lpips_distance_ok(a, b, w):
    """True when the head can run on amk_lpips_*: the switch on; a and b contiguous 4-D HIP tensors of one shape and one
    dtype with at least one element, f32 outside autocast or bf16 inside bf16 autocast; w f32 on the device with C elements;
    neither b nor w requiring grad.  Everything else (CPU, f16, f32 under autocast, non-contiguous or channels-last features,
    a b or w that requires grad, AMK_LPIPS=0) keeps the torch chain."""
    if not (LPIPS and a.is_cuda and b.is_cuda and w.is_cuda and a.dim() == 4 and a.shape == b.shape and a.dtype == b.dtype
            and a.is_contiguous() and b.is_contiguous() and a.numel() > 0 and w.dtype == torch.float32
            and w.numel() == a.shape[1] and not b.requires_grad and not w.requires_grad):
        return False
    if a.dtype == torch.float32:
        return not torch.is_autocast_enabled()
    return a.dtype == torch.bfloat16 and _bf16_autocast()


def lpips_distance(a, b, w, eps=1e-10):
    """The LPIPS distance of one feature level, (N,): mean over the pixels of sum_c w_c (a_c / (|a| + eps) - b_c / (|b| + eps))^2,
    |.| the norm over the channels of a pixel.  a, b (N, C, H, W), w C elements (the level's 1x1 convolution).

    On the fused kernels (see lpips_distance_ok) the result is f32, also for bf16 features under bf16 autocast, where the
    torch chain returns bf16; the gradient flows to a only, and a pixel of a whose norm is 0 gets a zero gradient where
    autograd gives NaN.  Everything the kernels do not take runs the torch chain."""
    if not lpips_distance_ok(a, b, w):
        return _lpips_chain(a, b, w, eps)
    return _LpipsDist.apply(_c16(a), _c16(b), w.detach().reshape(-1).contiguous(), eps)


# ---------------------------------------------------------------------------- masked-token loss head
# Logits + cross-entropy on the valid rows only (csrc/ce_head.hip) in place of F.linear + F.cross_entropy at the end of
# the Muse / MaskGit train step: the (rows, vocabulary) logits, their log-softmax and their gradient are never written.
# Measured at the Muse head (8192 rows, 8192 words, dim 1024, cosine-schedule targets; tools/kbench_ce_head.py,
# profiles/kbench_ce_head.log): 3.89 ms against 22.45 ms forward + backward, 336 MB against 805 MB of peak memory above the
# inputs; bench.py --model muse 195.4 against 215.6 ms per step.  So the switch ships on.  Read once per process.
# With a bias (Parti's to_logits; amk_ce_head_bias_*): at Parti's head (8192 rows x 8192 words x 512, every row valid;
# tools/kbench_ce_head.py --bias, profiles/kbench_ce_head_bias.log) 3.32 ms against 21.07 ms in f32 and, under bf16
# autocast (profiles/kbench_ce_head_bias_bf16.log), 0.88 ms against 18.40 ms; the Parti step (tools/kbench_parti.py, arms
# alternating, profiles/kbench_parti_ce_head[_bf16].log) 21.8 against 40.3 ms in f32 and 12.5 against 29.3 ms under autocast.
CE_HEAD = os.environ.get("AMK_CE_HEAD", "1") != "0"


# AMK_CE_HEAD_BF16: the same head under bf16 autocast (csrc/ce_head_bf16.hip: bf16 operands on v_mfma_f32_32x32x16_bf16,
# the logits and every softmax quantity in f32) in place of the library's three GEMMs over all rows, the bf16 logits,
# their f32 copy, the log-softmax and the logits' gradient.  Measured at the Muse head (tools/kbench_ce_head.py --autocast
# bf16, profiles/kbench_ce_head_bf16.log): 0.75 ms against 18.70 ms forward + backward, 201 MB against 688 MB of peak memory
# above the inputs; bench.py --model muse --autocast bf16 63.3 against 81.7 ms per step on the parent commit
# (profiles/bench_muse_ce_head_bf16.log).  So the switch ships on.  AMK_CE_HEAD=0 disables both heads.  Read once per process.
CE_HEAD_BF16 = os.environ.get("AMK_CE_HEAD_BF16", "1") != "0"


def _bf16_autocast():
    return torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16


def ce_head_ok(x, weight, bias=None):
    """The models' gate.  Without autocast: the switch is on, f32 HIP tensors, K a multiple of 4.  Under bf16 autocast:
    both switches are on, HIP tensors, an f32 master weight, K a multiple of 8 (the bf16 head).  A bias must be an f32
    HIP tensor of shape (V,) (it stays f32 under autocast)."""
    if not (CE_HEAD and x.is_cuda and weight.dtype == torch.float32 and x.numel() > 0):
        return False
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.shape == (weight.shape[0],)):
        return False
    if torch.is_autocast_enabled():
        return (CE_HEAD_BF16 and _bf16_autocast() and x.dtype in (torch.float32, torch.bfloat16)
                and x.shape[-1] % 8 == 0)
    return x.dtype == torch.float32 and x.shape[-1] % 4 == 0


def _row_major_view(t2, mult=4):
    """t2 (rows, cols) as the kernels take it: unit column stride, row stride a multiple of mult, 16-byte aligned."""
    if t2.stride(1) != 1 or t2.stride(0) % mult or t2.stride(0) < t2.shape[1] or t2.data_ptr() % 16:
        t2 = t2.contiguous()
        if t2.data_ptr() % 16:
            t2 = t2.clone()
    return t2


def _bias_view(bias, V):
    """bias (V,) f32 as the kernels take it: contiguous and 16-byte aligned (copied when it is not)."""
    if bias.dtype != torch.float32 or bias.shape != (V,):
        raise RuntimeError(f"linear_cross_entropy: bias must be f32 of shape ({V},); got {bias.dtype} {tuple(bias.shape)}")
    b = bias.detach()
    if b.stride(0) != 1 or b.data_ptr() % 16:
        b = b.contiguous()
        if b.data_ptr() % 16:
            b = b.clone()
    return b


def _claim_vec(p, V):
    """_claim for a (V,) f32 gradient the kernels write directly: (reducer, view) or (None, None)."""
    r, v = _claim(p)
    if v is not None and (v.dtype != torch.float32 or v.shape != (V,) or v.stride(0) != 1 or v.data_ptr() % 16):
        return None, None   # (not reached with the reducer's views: ALIGN-ed, contiguous)
    return r, v


# The two precisions of the head, indexed by `bf16`: (cast of x, cast of the weight, the multiple K and the row strides
# must have, dtype of dx and of the backward workspace G, the entry points [2 * has_bias + is_backward], event prefix).
# x is cast to bf16 if it arrives in f32, the weight goes through _w16 (the optimizer's bf16 shadow when it is current).
_CE_HEADS = (
    (lambda x: x, lambda w: w, 4, torch.float32,
     ("amk_ce_head_fwd", "amk_ce_head_bwd", "amk_ce_head_bias_fwd", "amk_ce_head_bias_bwd"), ""),
    (lambda x: x.to(torch.bfloat16), _w16, 8, torch.bfloat16,
     ("amk_ce_head_bf16_fwd", "amk_ce_head_bf16_bwd", "amk_ce_head_bias_bf16_fwd", "amk_ce_head_bias_bf16_bwd"), "bf16_"),
)


class _LinearCrossEntropy(torch.autograd.Function):
    """mean over the rows with target != ignore_index of logsumexp(x W^T + b) - (x W^T + b)[target], b = 0 without a
    bias; f32 (csrc/ce_head.hip) or, with bf16, on bf16 operands (csrc/ce_head_bf16.hip).  loss and lse in f32, dx in x's
    dtype, dw and db in f32 -- into the reducer's bucket when they can be claimed.  Saves the prepared x and w, the bias,
    target, lse, the compacted row list and the device-side count only -- the number of valid rows is never read on the
    host."""

    @staticmethod
    def forward(ctx, x, weight, bias, target, ignore_index, bf16):
        cast_x, cast_w, mult, _, names, ev = _CE_HEADS[bf16]
        K = x.shape[-1]
        x2 = _row_major_view(cast_x(x.reshape(-1, K)), mult)
        w2 = _row_major_view(cast_w(weight), mult)
        t = target.reshape(-1).contiguous()
        M, V = x2.shape[0], w2.shape[0]
        if t.shape[0] != M or w2.shape[1] != K:
            raise RuntimeError(f"linear_cross_entropy: x {tuple(x.shape)}, weight {tuple(weight.shape)}, target "
                               f"{tuple(target.shape)} do not fit")
        b1 = () if bias is None else (_bias_view(bias, V),)
        L = _lib.load()
        dev = x2.device
        nbytes = getattr(L, names[0] + "_ws_bytes")(M, V, K)
        ws = torch.empty(max(nbytes // 4, 4), device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        lse = torch.empty(M, device=dev, dtype=torch.float32)
        rows = torch.empty(M, device=dev, dtype=torch.int32)
        count = torch.empty(1, device=dev, dtype=torch.int32)
        fn = names[2 * len(b1)]
        with _timed(f"{ev}ce_head{'_bias' if b1 else ''}_fwd M{M} V{V} K{K}"):
            _lib.check(getattr(L, fn)(_ptr(x2), x2.stride(0), _ptr(w2), w2.stride(0), *map(_ptr, b1), _ptr(t),
                                      int(ignore_index), M, V, K, _ptr(loss), _ptr(lse), _ptr(rows), _ptr(count), _ptr(ws),
                                      nbytes, _stream()), fn)
        ctx.save_for_backward(x2, w2, *b1, t, lse, rows, count)
        ctx.ignore_index, ctx.bf16 = int(ignore_index), bf16
        ctx.x_shape, ctx.x_dtype = x.shape, x.dtype
        ctx.weight, ctx.bias = weight, bias
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loss):
        x2, w2, *b1, t, lse, rows, count = ctx.saved_tensors
        _, _, mult, dtype, names, ev = _CE_HEADS[ctx.bf16]
        M, K = x2.shape
        V = w2.shape[0]
        L = _lib.load()
        dev = x2.device
        d = d_loss.reshape(1).to(torch.float32).contiguous()   # stays on the device
        dx = torch.empty(M, K, device=dev, dtype=dtype)
        wr, wv = _claim(ctx.weight) if ctx.needs_input_grad[1] else (None, None)
        if wv is not None and (wv.stride(-1) != 1 or wv.data_ptr() % 16 or wv.shape != w2.shape or wv.stride(0) % mult
                               or wv.dtype != torch.float32):
            wr, wv = None, None   # (not reached with the reducer's views: ALIGN-ed, contiguous)
        dw = wv if wv is not None else torch.empty(V, K, device=dev, dtype=torch.float32)
        br, bv, db = None, None, ()
        if b1:
            br, bv = _claim_vec(ctx.bias, V) if ctx.needs_input_grad[2] else (None, None)
            db = (bv if bv is not None else torch.empty(V, device=dev, dtype=torch.float32),)
        nbytes = getattr(L, names[1] + "_ws_bytes")(M, V, K)
        ws = torch.empty(max(nbytes, 16) // dx.element_size(), device=dev, dtype=dtype)
        fn = names[2 * len(b1) + 1]
        with _timed(f"{ev}ce_head{'_bias' if b1 else ''}_bwd M{M} V{V} K{K}"):
            _lib.check(getattr(L, fn)(_ptr(x2), x2.stride(0), _ptr(w2), w2.stride(0), *map(_ptr, b1), _ptr(t),
                                      ctx.ignore_index, M, V, K, _ptr(d), _ptr(lse), _ptr(rows), _ptr(count), _ptr(dx),
                                      dx.stride(0), _ptr(dw), dw.stride(0), *map(_ptr, db), _ptr(ws), nbytes, _stream()), fn)
        if wv is not None:
            wr.wrote(ctx.weight)
            dw = None
        if bv is not None:
            br.wrote(ctx.bias)
            db = ()
        return dx.view(ctx.x_shape).to(ctx.x_dtype), dw, db[0] if db else None, None, None, None


def linear_cross_entropy(x, weight, target, ignore_index=-100, bias=None):
    """F.cross_entropy(F.linear(x, weight, bias).flatten(0, -2), target.flatten(), ignore_index=ignore_index) as one op
    that never writes the logits: x (..., K) f32, weight (V, K), bias None or (V,) f32 (it stays f32 under autocast; its
    gradient is f32), target (...) int64 -> scalar f32 (mean over the rows whose
    target is not ignore_index; NaN when there is none).  Inside bf16 autocast: x f32 or bf16, weight the f32 master, the
    products on bf16 operands with the logits and the softmax in f32 (csrc/ce_head_bf16.hip).  A target outside [0, V) that is not ignore_index poisons the
    loss (NaN) instead of raising: raising would need the host to read device data.  Once differentiable."""
    bf16 = _bf16_autocast()
    _require_device(*((weight, target) if bf16 and x.is_cuda and x.dtype == torch.bfloat16 else (x, weight, target)))
    if bias is not None:
        _require_device(bias)
    if target.dtype != torch.int64:
        raise RuntimeError(f"linear_cross_entropy: target must be int64; got {target.dtype}")
    if bf16:   # bf16 operands (x cast, the weight's bf16 shadow), f32 loss, dx in x's dtype, dw in f32
        with torch.autocast("cuda", enabled=False):
            return _LinearCrossEntropy.apply(x, weight, bias, target, ignore_index, True)
    return _LinearCrossEntropy.apply(x, weight, bias, target, ignore_index, False)
