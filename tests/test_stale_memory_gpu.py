"""Every autograd entry point of amk.ops (and the plain entry points next to them) run twice from identical inputs: once
with every torch.empty / empty_like / empty_strided / new_empty of amk filled with NaN, once with a large finite value
(tests/poison.py).  A result that depends only on its inputs cannot change with the fill, so for every output and
gradient the test asserts

  * finite, wherever the family's own reference is finite (the documented exception: the loss head's NaN loss when no
    row is valid);
  * BITWISE equal between the two fills (torch.equal) -- the main assertion, no tolerance;
  * where the family has a reference module with a check that takes the op's own tensors (the ref= of a case), the
    "nan" run passes that check, bounds unchanged.  What is left out bounds single launches through the C ABI, on
    operands or outputs an op does not expose: gemm_x6, gemm_x6_tn, dense_f32 and the GEMMs of bf16_dense (one product of a
    Linear's three, with the kernel's own chunking in the bound), gemm_rows_bf16 (its own fixed operands), moe (the grouped
    GEMMs on routing lists), attn_x6 (the packed score tiles), attn_bwd_x6 (a figure relative to the f32 kernel, not a
    bound), and row_f32's Adam (one segment list, not a FlatAdam).

A case whose name says which kernel it forces (path= of a case) also asserts that this kernel's entry point was called
with the stage bits of the path.

A case may carry env= next to switches=: environment variables the library reads at every call (AMK_GEMM16_F32OUT of the
guided logits head), set and put back around the run; tests/test_redzone_gpu.py does the same.

The guard: while the cases run, every launcher of amk.lib.SIGNATURES (an entry point that takes a stream) is spied, and the
last test of the file asserts that each one was reached by a case or stands in NOT_SWEPT with an admissible reason -- so an
entry point added without a case fails here, by name (tests/sweep_guard.py, DESIGN.md "Stale memory").  The decode at model
level (prefill and sample steps of Parti and the Transformer, MUSE.generate) is in tests/test_stale_memory_decode_gpu.py.

Paths that accumulate with float atomics by design are listed in ATOMIC with the csrc line of the atomic: for the named
tensors of those cases bitwise equality is replaced by the family's existing bound, and the same case runs again in the
project's reproducible mode, where it must be bitwise equal.

Per family: a case where every tiled extent is a whole number of tiles, cases one past a tile boundary (taken from the
sweep tables of the family's own GPU test), and the smallest legal size.  Paths gated by size are forced with the module
switches, the cases stay tiny.  Nothing here is meant to make a kernel fault: integer and index buffers are never filled.
"""
import contextlib
import os

import pytest
import torch
from torch import nn

import sweep_guard
from poison import assert_fill_independent, run_both_fills
from util import assert_close, seeded

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16

# Float-atomic paths.  src: the atomic in the kernel source; tensors: the results it reaches; repro: how the case is run
# again without atomics (ops switches, or torch.use_deterministic_algorithms for "torch_det").
ATOMIC = {
    "attn_dq": dict(src="csrc/attn_bwd_fused.hip:443", tensors=("dq",),
                    repro=dict(DETERMINISTIC_ATTENTION_BACKWARD=True)),
    "attn_dq_x6": dict(src="csrc/attn_bwd_fused_x6.hip:311", tensors=("dq",),
                       repro=dict(DETERMINISTIC_ATTENTION_BACKWARD=True)),
    "vq_dcodebook": dict(src="csrc/vq.hip:354", tensors=("dcodebook",), repro="torch_det"),
}
# (the routed experts' weight gradient cut in two, csrc/moe.hip:1157, adds two halves into a zeroed dW: 0 + a + b is the same
# in either order, so that path is held to bitwise equality like everything else -- case moe_routed/wgrad_split.  The sums
# inside the expert GEMM, csrc/moe.hip:563, are off by default (ops.MOE_SUM_IN_GEMM) and not covered here.)


@contextlib.contextmanager
def _switches(**kw):
    from amk import ops

    old = {k: getattr(ops, k) for k in kw}
    for k, v in kw.items():
        setattr(ops, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


@contextlib.contextmanager
def _env(env):
    """Environment variables that the library reads at every call (env= of a case): value None = unset.  Put back on exit."""
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _autocast(on):
    return torch.autocast("cuda", dtype=BF16, enabled=bool(on))


KINDS = ("whole", "edge", "smallest")      # every tiled extent whole tiles / one past a tile boundary / the smallest legal size


class Case:
    def __init__(self, family, name, fn, kind, atomic=None, ref=None, allow_nan=(), switches=None, path=None, env=None):
        assert kind in KINDS, kind
        self.family, self.name, self.fn, self.kind, self.atomic, self.ref = family, name, fn, kind, atomic, ref
        self.allow_nan, self.switches, self.path, self.env = allow_nan, dict(switches or {}), path, dict(env or {})

    @property
    def id(self):
        return f"{self.family}/{self.name}"


CASES = []


def _add(family, name, fn, kind, **kw):
    CASES.append(Case(family, name, fn, kind, **kw))


def _kinds(shapes):
    """whole, edge, ..., edge, smallest: how the shape lists below are ordered unless a list says otherwise."""
    return zip(shapes, ("whole",) + ("edge",) * (len(shapes) - 2) + ("smallest",))


@contextlib.contextmanager
def _library_calls(names, reached=None):
    """Records (entry point, its `stages` argument) of every call of the named libamk entry points made inside the block;
    reached: a set that collects the names called instead (the guard's spy on every launcher).  Blocks nest: the inner one
    wraps what the outer one installed and puts that back.  amk binds no entry point at import time -- ops.py, dense.py and
    optim.py look every one up on the loaded library when they call it (by attribute or by getattr on a name) -- so the
    library object is the one place to spy."""
    from amk import lib

    L, seen, old = lib.load(), [], {}

    def spy(name, fn):
        def call(*args):
            if reached is not None:
                reached.add(name)
            else:
                seen.append((name, args[-2] if "bwd" in name else None))     # (..., scale, stages, stream)
            return fn(*args)
        return call

    for n in names:
        old[n] = getattr(L, n)
        setattr(L, n, spy(n, old[n]))
    try:
        yield seen
    finally:
        for n, fn in old.items():
            setattr(L, n, fn)


# ---------------------------------------------------------------------------------------------- attention
def _attn_inputs(B, H, I, J, D, mask):
    q, k, v, cot = seeded((B, H, I, D), 1), seeded((B, H, J, D), 2), seeded((B, H, J, D), 3), seeded((B, H, I, D), 4)
    km = None
    if mask == "key":
        km = torch.ones(B, J, dtype=torch.bool)
        km[B - 1, J - max(1, J // 3):] = False
    return q, k, v, cot, km


def _attn_fn(entry, B, H, I, J, D, mask, dtype=F32):
    def fn(device):
        from amk import ops

        q, k, v, cot, km = _attn_inputs(B, H, I, J, D, mask)
        kmd = km.to(device) if km is not None else None
        cm = ops.causal_mask(I, J, device) if mask == "causal" else None
        scale = D ** -0.5
        if entry == "core":
            qd, kd, vd = (t.to(device).requires_grad_() for t in (q, k, v))
            o = ops.attention(qd, kd, vd, scale, key_mask=kmd, causal_mask=cm)
            dq, dk, dv = torch.autograd.grad(o, (qd, kd, vd), cot.to(device))
            return dict(o=o, dq=dq, dk=dk, dv=dv)
        pack = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], H * D)   # noqa: E731
        q2 = pack(q).to(device=device, dtype=dtype).requires_grad_()
        kv2 = torch.cat([pack(k), pack(v)], -1).to(device=device, dtype=dtype).requires_grad_()
        o2 = ops.attention_fused_kv(q2, kv2, H, D, scale, key_mask=kmd, causal_mask=cm)
        assert type(o2.grad_fn).__name__ == ("_AttnFusedKVBF16Backward" if dtype == BF16 else "_AttnFusedKVBackward")
        dq2, dkv2 = torch.autograd.grad(o2, (q2, kv2), pack(cot).to(device=device, dtype=dtype))
        unpack = lambda t, T: t.reshape(B, T, H, D).permute(0, 2, 1, 3)   # noqa: E731
        return dict(o=unpack(o2, I), dq=unpack(dq2, I), dk=unpack(dkv2[..., :H * D], J), dv=unpack(dkv2[..., H * D:], J))
    return fn


def _attn_ref(B, H, I, J, D, mask):
    """The bound tests/test_attention_gpu.py holds the f32 core to: 2e-5 against the CPU oracle (util.assert_close).  Not at
    one key: the softmax over one key is 1 whatever q and k are, so dq and dk are identically zero there and a bound
    relative to the reference's largest element says nothing (the kernels give ~1e-7, the rounding of dp - delta); o and dv
    are held there too."""
    names = ("o", "dv") if J == 1 else ("o", "dq", "dk", "dv")

    def ref(got, device):
        from amk import ops
        from oracle import ref_cpu

        q, k, v, cot, km = _attn_inputs(B, H, I, J, D, mask)
        cm = ops.causal_mask(I, J, device).cpu() if mask == "causal" else None
        qs, ks, vs = (t.clone().requires_grad_() for t in (q, k, v))
        want = ref_cpu.attention_core(qs, ks, vs, D ** -0.5, km, cm)
        wq, wk, wv = torch.autograd.grad((want * cot).sum(), (qs, ks, vs))
        for name, w in (("o", want), ("dq", wq), ("dk", wk), ("dv", wv)):
            if name in names:
                assert_close(got[name].cpu(), w, 2e-5, f"{name} against the oracle")
    return ref


def _attn_bf16_ref(B, H, I, J, mask, D=64):
    """tests/bf16_attention_ref.py (head dim 64) and tests/bf16_attention_hd_ref.py (32, 128): o, dq, dk and dv of the bf16
    core element by element within its bound of the fp64 reference on the bf16 values."""
    def ref(got, device):
        import bf16_attention_hd_ref
        import bf16_attention_ref
        from amk import ops

        mod = bf16_attention_ref if D == 64 else bf16_attention_hd_ref
        q, k, v, cot, km = (None if t is None else t.to(BF16).float() if t.is_floating_point() else t
                            for t in _attn_inputs(B, H, I, J, D, mask))
        cm = ops.causal_mask(I, J, device).cpu() if mask == "causal" else None
        R = mod.reference(q, k, v, cot, D ** -0.5, km, cm)
        mod.assert_within(got, R, "stale-memory case")
    return ref


# The library entry points and the `stages` bits (amk.h, ops.ATTN_BWD_*) a forced path must show.  The host code does not
# clamp them at small sizes: fused_keys_per_wg (csrc/attn_bwd_fused.hip:501) returns a forced 128 / 256 whatever J is, and
# AMK_ATTN_BWD_X6 has one geometry and no fallback (csrc/attn_bwd.hip:77-89: it launches the split-bf16 kernel or fails).
_FUSED, _K128, _K256, _X6 = 8, 16, 32, 128
_ATTN_ENTRIES = ("amk_attn_fwd", "amk_attn_fwd_keep", "amk_attn_fwd_x6", "amk_attn_fwd_x6_keep", "amk_attn_bwd", "amk_attn_bwd_kept")


def _attn_path(fwd, bwd, bits=_FUSED, stages=None):
    """fwd / bwd: the entry points called; bits: of KEYS128 | KEYS256 | X6 | FUSED exactly these are set; stages: the whole word."""
    def check(seen):
        assert [n for n, _ in seen] == [fwd, bwd] * 2, seen              # one forward and one backward per fill
        for n, st in seen:
            if n == bwd and stages is not None:
                assert st == stages, seen
            elif n == bwd:
                assert st & (_FUSED | _K128 | _K256 | _X6) == bits, seen
    return dict(entries=_ATTN_ENTRIES, check=check)


def _attn_pair_bound(name, a, b):
    assert_close(a, b, 2e-5, f"{name}: atomic arrival order, the two fills")


_OFF = dict(ATTENTION_FORWARD="f32", ATTENTION_BACKWARD_X6="0", ATTENTION_KEEP_SCORES=True,
            ATTENTION_BACKWARD_TWO_KERNEL=False, ATTENTION_BACKWARD_KEYS=0, DETERMINISTIC_ATTENTION_BACKWARD=False)
# (B, H, I, J, mask): whole tiles; one past a boundary with each mask and I != J; the smallest
_ATTN_SHAPES = [(1, 2, 64, 64, None), (1, 2, 33, 65, "key"), (1, 2, 65, 77, "causal"), (2, 2, 129, 257, "key"),
                (1, 2, 257, 129, None), (1, 1, 1, 1, None)]
for (_B, _H, _I, _J, _m), _kd in _kinds(_ATTN_SHAPES):
    _s = f"{_B}x{_H}x{_I}x{_J}_{_m or 'nomask'}"
    for _entry in ("core", "fused"):
        _fn, _rf = _attn_fn(_entry, _B, _H, _I, _J, 64, _m), _attn_ref(_B, _H, _I, _J, 64, _m)
        # f32 forward, scores kept, one-pass backward with dq atomics
        _add("attention", f"{_entry}_f32_keep_{_s}", _fn, _kd, atomic="attn_dq", ref=_rf, switches=_OFF,
             path=_attn_path("amk_attn_fwd_keep", "amk_attn_bwd_kept"))
        # split-bf16 forward (forced), scores kept
        _add("attention", f"{_entry}_x6fwd_keep_{_s}", _fn, _kd, atomic="attn_dq", ref=_rf,
             switches=dict(_OFF, ATTENTION_FORWARD="bf16x6"), path=_attn_path("amk_attn_fwd_x6_keep", "amk_attn_bwd_kept"))
    _fn, _rf = _attn_fn("fused", _B, _H, _I, _J, 64, _m), _attn_ref(_B, _H, _I, _J, 64, _m)
    # scores recomputed: one-pass and two-kernel backward, f32 and split-bf16 forward
    _add("attention", f"fused_f32_recompute_{_s}", _fn, _kd, atomic="attn_dq", ref=_rf,
         switches=dict(_OFF, ATTENTION_KEEP_SCORES=False), path=_attn_path("amk_attn_fwd", "amk_attn_bwd"))
    _add("attention", f"fused_x6fwd_recompute_{_s}", _fn, _kd, atomic="attn_dq", ref=_rf,
         switches=dict(_OFF, ATTENTION_FORWARD="bf16x6", ATTENTION_KEEP_SCORES=False),
         path=_attn_path("amk_attn_fwd_x6", "amk_attn_bwd"))
    _add("attention", f"fused_two_kernel_{_s}", _fn, _kd, ref=_rf, switches=dict(_OFF, ATTENTION_BACKWARD_TWO_KERNEL=True),
         path=_attn_path("amk_attn_fwd", "amk_attn_bwd", stages=7))         # delta + dK/dV + dQ
    # the kept-scores backward at 128 and at 256 keys per workgroup, and its split-bf16 form (256 keys, forced)
    _add("attention", f"fused_keys128_{_s}", _fn, _kd, atomic="attn_dq", ref=_rf, switches=dict(_OFF, ATTENTION_BACKWARD_KEYS=128),
         path=_attn_path("amk_attn_fwd_keep", "amk_attn_bwd_kept", _FUSED | _K128))
    _add("attention", f"fused_keys256_{_s}", _fn, _kd, atomic="attn_dq", ref=_rf, switches=dict(_OFF, ATTENTION_BACKWARD_KEYS=256),
         path=_attn_path("amk_attn_fwd_keep", "amk_attn_bwd_kept", _FUSED | _K256))
    _add("attention", f"fused_x6bwd_{_s}", _fn, _kd, atomic="attn_dq_x6", ref=_rf,
         switches=dict(_OFF, ATTENTION_FORWARD="bf16x6", ATTENTION_BACKWARD_X6="1", ATTENTION_BACKWARD_KEYS=256),
         path=_attn_path("amk_attn_fwd_x6_keep", "amk_attn_bwd_kept", _FUSED | _K256 | _X6))
    # the bf16 core (bf16 projections in, head dim 64)
    _add("attention_bf16", f"fused_bf16_{_s}", _attn_fn("fused", _B, _H, _I, _J, 64, _m, BF16), _kd,
         ref=_attn_bf16_ref(_B, _H, _I, _J, _m))
# the bf16 core at head dims 32 and 128 (csrc/attn_bf16_hd.hip, amk_attn_bf16_hd_fwd / _bwd: opt-in through
# ops.ATTENTION_BF16_DIMS), which the entry-point guard found without a case
for _D in (32, 128):
    for (_B, _H, _I, _J, _m), _kd in _kinds([(1, 2, 128, 128, None), (1, 2, 65, 77, "causal"), (2, 2, 33, 129, "key"), (1, 1, 1, 1, None)]):
        _add("attention_bf16_head_dims", f"d{_D}_{_B}x{_H}x{_I}x{_J}_{_m or 'nomask'}", _attn_fn("fused", _B, _H, _I, _J, _D, _m, BF16), _kd,
             ref=_attn_bf16_ref(_B, _H, _I, _J, _m, _D), switches=dict(ATTENTION_BF16_DIMS=frozenset((32, 64, 128))))
# every head-dim template: 32 and 128 have the one-pass backward (atomics), the others recompute in three launches
for _D in (32, 96, 128, 160, 192, 224, 256):
    for (_B, _H, _I, _J, _m), _kd in _kinds([(1, 2, 64, 64, None), (1, 2, 65, 77, "causal"), (1, 2, 33, 65, "key"), (1, 1, 1, 1, None)]):
        _s = f"d{_D}_{_B}x{_H}x{_I}x{_J}_{_m or 'nomask'}"
        _add("attention_head_dims", _s, _attn_fn("core", _B, _H, _I, _J, _D, _m), _kd,
             atomic="attn_dq" if _D in (32, 128) else None, ref=_attn_ref(_B, _H, _I, _J, _D, _m), switches=_OFF)


# ---------------------------------------------------------------------------------------------- decode
def _decode_fn(B, H, D, cap, n, dtype, masked):
    def fn(device):
        from amk import ops

        hd = H * D
        q = seeded((B, 1, hd), 1).to(device=device, dtype=dtype)
        new = seeded((B, 1, 2 * hd), 2).to(device=device, dtype=dtype)
        cache = seeded((B, cap, 2 * hd), 3).to(device=device, dtype=dtype)
        n_dev = torch.tensor([n], device=device, dtype=torch.int32)
        km = None
        if masked:
            km = torch.ones(B, cap, dtype=torch.bool, device=device)
            km[B - 1, : n // 2] = False
        with torch.no_grad():
            o = ops.attention_decode(q, new, cache, n_dev, H, D, D ** -0.5, key_mask=km)       # append mode
            # read mode over the n + 1 rows now valid (n_dev = 0 there is out of range: the kernels then write nothing)
            o2 = ops.attention_decode(q, None, cache, n_dev + 1, H, D, D ** -0.5, key_mask=km)
        return dict(o_append=o, o_read=o2, cache=cache)
    return fn


def _decode_ref(B, H, D, cap, n, masked, dtype):
    """tests/attn_decode_ref.py: the f32 kernel's output within the per-element bound of the float64 reference, in append
    mode and in read mode over the same n + 1 rows.  tests/attn_decode_bf16_ref.py for bf16 caches: the same reference on
    the bf16 values, every stored element between the roundings of the bound's two ends."""
    def ref(got, device):
        import attn_decode_bf16_ref
        import attn_decode_ref

        hd = H * D
        q, new, cache = (t.to(dtype).float() for t in (seeded((B, 1, hd), 1), seeded((B, 1, 2 * hd), 2), seeded((B, cap, 2 * hd), 3)))
        cache[:, n] = new[:, 0]
        assert torch.equal(got["cache"].cpu().float(), cache), "the cache after the append"
        heads = lambda t: t.reshape(B, -1, H, D).permute(0, 2, 1, 3)   # noqa: E731
        k, v = heads(cache[:, : n + 1, :hd]), heads(cache[:, : n + 1, hd:])
        km = None
        if masked:
            km = torch.ones(B, n + 1, dtype=torch.bool)
            km[B - 1, : n // 2] = False
        if dtype == BF16:
            _, _, lo, hi, _ = attn_decode_bf16_ref.reference(q.reshape(B, H, D), k, v, D ** -0.5, km)
            for name in ("o_append", "o_read"):
                n_bad = attn_decode_bf16_ref.count_outside(got[name].cpu().reshape(B, H, D), lo, hi)
                assert n_bad == 0, f"{name}: {n_bad} elements outside [rne(ref - b), rne(ref + b)]"
            return
        want, bound, _ = attn_decode_ref.reference(q.reshape(B, H, D), k, v, D ** -0.5, km)
        for name in ("o_append", "o_read"):
            n_bad, worst = attn_decode_ref.worst_ratio(got[name].cpu().reshape(B, H, D), want, bound)
            assert n_bad == 0, f"{name}: {n_bad} elements outside the bound (worst {worst:.2f}x)"
    return ref


for _dt, _tag in ((F32, "f32"), (BF16, "bf16")):
    for (_B, _H, _D, _cap, _n, _mk), _kd in _kinds([(2, 2, 64, 128, 64, False), (2, 3, 64, 300, 129, True), (1, 2, 32, 77, 65, True),
                                                    (1, 1, 64, 1, 0, False)]):
        _add("attention_decode", f"{_tag}_B{_B}_h{_H}_d{_D}_cap{_cap}_n{_n}", _decode_fn(_B, _H, _D, _cap, _n, _dt, _mk), _kd,
             ref=_decode_ref(_B, _H, _D, _cap, _n, _mk, _dt))


# ---------------------------------------------------------------------------------------------- prefill
def _prefill_inputs(B, H, D, cap, p0, n, bf16):
    """q, k, v (B, H, cap, D) by absolute position (tests/attn_prefill_ref.py); the cache before the call (B, cap, 2*h*d):
    rows 0 .. p0 - 1 hold k | v, the rows from p0 on what an earlier sequence left there; the key mask of the read call."""
    import attn_prefill_ref as P

    q, k, v = P.make_inputs(B, H, D, cap, seed=6000 + D + p0, bf16=bf16)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B, cap, H * D)   # noqa: E731
    rows = torch.cat((flat(k), flat(v)), dim=2)
    cache = rows.clone()
    left = seeded((B, cap - p0, 2 * H * D), 7, 3.0)
    cache[:, p0:] = left.to(BF16).float() if bf16 else left
    km = torch.ones(B, cap, dtype=torch.bool)
    km[B - 1, : (p0 + n) // 2] = False
    return q, k, v, flat(q), rows, cache, km


def _prefill_fn(B, H, D, cap, p0, n, dtype):
    def fn(device):
        from amk import ops

        _, _, _, q2, rows, cache, km = _prefill_inputs(B, H, D, cap, p0, n, dtype == BF16)
        q2 = q2[:, p0:p0 + n].to(device=device, dtype=dtype)
        kv_new = rows[:, p0:p0 + n].to(device=device, dtype=dtype)
        cache = cache.to(device=device, dtype=dtype)
        n_dev = torch.tensor([p0], device=device, dtype=torch.int32)
        with torch.no_grad():
            o = ops.attention_prefill(q2, kv_new, cache, n_dev, H, D, D ** -0.5)                        # append mode
            # read mode: every row over the p0 + n rows now valid, under a key mask
            o2 = ops.attention_prefill(q2, None, cache, n_dev + n, H, D, D ** -0.5, key_mask=km.to(device))
        return dict(o_append=o, o_read=o2, cache=cache)
    return fn


def _prefill_ref(B, H, D, cap, p0, n, dtype):
    """tests/attn_prefill_ref.py: the cache is its input with rows p0 .. p0 + n - 1 replaced, bitwise; row i of the append call
    within the per-row bound of the float64 reference over keys 0 .. p0 + i, row i of the read call within that of the masked
    reference over keys 0 .. p0 + n - 1.  bf16 caches: every stored element between the roundings of the bound's two ends,
    the interval check of tests/test_attn_prefill_bf16_gpu.py."""
    def ref(got, device):
        import attn_prefill_ref as P

        bf16 = dtype == BF16
        q, k, v, _, rows, cache, km = _prefill_inputs(B, H, D, cap, p0, n, bf16)
        cache[:, p0:p0 + n] = rows[:, p0:p0 + n]
        assert torch.equal(got["cache"].cpu().float(), cache), "the cache after the append"
        for name, J, mask in (("o_append", None, None), ("o_read", p0 + n, km)):
            assert got[name].dtype == dtype and tuple(got[name].shape) == (B, n, H * D), name
            rows_got = got[name].cpu().float().view(B, n, H, D).permute(0, 2, 1, 3)
            for i in range(n):
                R = P.row_reference(q, k, v, p0 + i, J=J, mask=mask, bf16=bf16)
                n_bad = P.outside(rows_got[:, :, i], R, bf16=bf16)
                assert n_bad == 0, f"{name}: row {i}: {n_bad} elements outside the row's bound"
    return ref


for _dt, _tag in ((F32, "f32"), (BF16, "bf16")):
    # two chunks of 64 keys per row (the partials workspace and the combine launch); a call that ends at the capacity with
    # D % 64 == 32 and a partial row block and chunk; rows that stop short of a chunk beside rows that cross it; the smallest
    for (_B, _H, _D, _cap, _p0, _n), _kd in _kinds([(2, 2, 64, 128, 64, 64), (2, 3, 96, 200, 130, 70), (1, 2, 32, 200, 6, 64),
                                                    (1, 1, 32, 1, 0, 1)]):
        _add("attention_prefill", f"{_tag}_B{_B}_h{_H}_d{_D}_cap{_cap}_p{_p0}_n{_n}", _prefill_fn(_B, _H, _D, _cap, _p0, _n, _dt), _kd,
             ref=_prefill_ref(_B, _H, _D, _cap, _p0, _n, _dt))


# ---------------------------------------------------------------------------------------------- guided logits head
def _guided_inputs(M, dim, V, second, bf16_rows):
    import guided_head_ref

    hc, hn, gamma, beta = guided_head_ref.make_cfg_ln("unit", M, dim, 60 + dim, bf16=bf16_rows)
    w = torch.randn(V, dim, generator=torch.Generator().manual_seed(61 + V)) * 0.05
    return hc, (hn if second else None), gamma, beta, w


def _guided_fn(M, dim, V, second, bf16_rows):
    def fn(device):
        from amk import ops

        hc, hn, gamma, beta, w = _guided_inputs(M, dim, V, second, bf16_rows)
        dt = BF16 if bf16_rows else F32
        hcd = hc.to(device=device, dtype=dt)
        hnd = hn.to(device=device, dtype=dt) if second else None
        with torch.no_grad(), _autocast(True):
            assert ops.guided_logits_ok(hcd, w.to(device))
            logits = ops.guided_logits(hcd, gamma.to(device), beta.to(device), w.to(device), null_h=hnd, cfg_scale=3.0)
        return dict(logits=logits)
    return fn


def _guided_ref(M, dim, V, second, bf16_rows):
    """The check of tests/test_guided_head_gpu.py's test_guided_logits_op against tests/guided_head_ref.py: the LayerNorm's
    bf16 rows through the C ABI inside their intervals, the op's logits bitwise the C GEMM's on those rows, and every logit
    inside the GEMM's bound.  Runs inside the case's env, so the C GEMM uses the store the op used."""
    def ref(got, device):
        import guided_head_ref
        from test_guided_head_gpu import _cfg_ln, _gemm      # the names only: no test function is imported

        hc, hn, gamma, beta, w = _guided_inputs(M, dim, V, second, bf16_rows)
        u = _cfg_ln(device, hc, hn, gamma, beta, 3.0, bf16_rows)
        assert guided_head_ref.inside(u, guided_head_ref.ref_cfg_ln(hc, hn, gamma, beta, 3.0)).all()
        u32, w32 = u.float().cpu(), w.to(device).bfloat16().float().cpu()
        c = _gemm(device, u32, w32, None)[:M]
        assert got["logits"].dtype == F32 and torch.equal(got["logits"], c)
        assert guided_head_ref.outside_gemm(c, guided_head_ref.ref_gemm_f32(u32, w32)) == 0
    return ref


# a whole 128-row tile; one row past it with V no multiple of 64; few rows of a long K without the second hidden state; the
# smallest.  Each under both stores of the GEMM (csrc/gemm_bf16.hip:574-599, read at every call).
for (_M, _dim, _V, _second, _b16), _kd in _kinds([(128, 128, 256, True, False), (129, 72, 136, True, True), (5, 264, 8, False, False),
                                                  (1, 8, 8, True, False)]):
    for _store in (None, "direct"):
        _add("guided_logits", f"{_M}x{_dim}x{_V}_{'two' if _second else 'one'}_{'bf16' if _b16 else 'f32'}rows_{_store or 'lds'}_store",
             _guided_fn(_M, _dim, _V, _second, _b16), _kd, ref=_guided_ref(_M, _dim, _V, _second, _b16),
             env=dict(AMK_GEMM16_F32OUT=_store))


# ---------------------------------------------------------------------------------------------- agent attention
def _agent_inputs(B, H, T, D, P, bf16=False):
    import agent_bf16_ref
    import agent_ref

    # q, k, v, d_o (B, H, T, D), conv_w, conv_b; for the bf16 path q, k, v and d_o are bf16 values
    return (agent_bf16_ref if bf16 else agent_ref).make_inputs("diffuse", B, H, T, D, P, D ** -0.5, 77)


def _agent_fn(B, H, T, D, P, bf16):
    def fn(device):
        from amk import ops

        dt = BF16 if bf16 else F32
        q, k, v, g, cw, cb = (x.to(device) for x in _agent_inputs(B, H, T, D, P, bf16))
        bthd = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, H * D)   # noqa: E731
        qkv = torch.cat([bthd(q), bthd(k), bthd(v)], -1).contiguous().to(dt).requires_grad_()
        cw, cb = cw.clone().requires_grad_(), cb.clone().requires_grad_()
        with _autocast(bf16):
            o = ops.agent_attention(qkv, cw, cb, H, D, P, D ** -0.5)
        assert type(o.grad_fn).__name__ == ("_AgentAttnBF16Backward" if bf16 else "_AgentAttnBackward")
        dqkv, dcw, dcb = torch.autograd.grad(o, (qkv, cw, cb), bthd(g).contiguous().to(dt))
        back = lambda x: x.reshape(B, T, H, D).permute(0, 2, 1, 3)   # noqa: E731
        dq, dk, dv = (back(t) for t in dqkv.view(B, T, 3, H * D).unbind(2))
        return dict(o=back(o), dq=dq, dk=dk, dv=dv, dconv_w=dcw, dconv_b=dcb)
    return fn


def _agent_ref_check(B, H, T, D, P, bf16):
    """tests/agent_ref.py: both tiers of its per-element bounds on the op's outputs and gradients.  tests/agent_bf16_ref.py
    for the bf16 path: the bf16 outputs inside the rounded interval, the f32 ones (the convolution's gradients) as before."""
    def ref(got, device):
        import agent_bf16_ref
        import agent_ref

        R = agent_ref.reference(*(x.to(device) for x in _agent_inputs(B, H, T, D, P, bf16)), P, D ** -0.5)
        for name in ("o", "dq", "dk", "dv", "dconv_w", "dconv_b"):
            if bf16 and name in agent_bf16_ref.ROUNDED:
                agent_bf16_ref.assert_rounded_within(got[name], R, name, "stale-memory case")
            else:
                agent_ref.assert_within(got[name], R, name, "stale-memory case", key=("stale_bf16_" if bf16 else "stale_") + name)
    return ref


import agent_ref as _agent_ref  # noqa: E402

for _bf in (False, True):
    # after tests/test_agent_bounds_gpu.py's grid: a whole chunk, one past one and two chunks, P == T, the smallest
    for (_B, _H, _T, _D, _P), _kd in _kinds([(1, 2, _agent_ref.chunk_len(64), 64, 8), (2, 2, _agent_ref.chunk_len(64) + 1, 64, 6),
                                             (2, 3, 2 * _agent_ref.chunk_len(32) + 1, 32, 7),
                                             (1, 1, _agent_ref.chunk_len(128) + 1, 128, 16), (2, 2, 5, 64, 5), (2, 1, 1, 64, 1)]):
        _add("agent_bf16" if _bf else "agent", f"B{_B}_h{_H}_T{_T}_d{_D}_P{_P}", _agent_fn(_B, _H, _T, _D, _P, _bf), _kd,
             ref=_agent_ref_check(_B, _H, _T, _D, _P, _bf))


# ---------------------------------------------------------------------------------------------- VQ
def _vq_fn(N, K, C):
    def fn(device):
        from amk import ops

        z = seeded((N, C), 1).to(device).requires_grad_()
        cb = seeded((K, C), 2).to(device).requires_grad_()
        out, idx, loss = ops.vq_lookup(z, cb, 0.25)
        dz, dcb = torch.autograd.grad((out * seeded((N, C), 3).to(device)).sum() + 0.7 * loss, (z, cb))
        emb = ops.vq_gather(idx, cb)
        return dict(out=out, idx=idx, loss=loss, dz=dz, dcodebook=dcb, gather=emb)
    return fn


def _vq_pair_bound(name, a, b):
    assert_close(a, b, 2e-5, f"{name}: atomic arrival order, the two fills")


for (_N, _K, _C), _kd in zip([(128, 256, 32), (129, 65, 32), (300, 1000, 64), (257, 8192, 32), (5, 1, 32), (1, 1, 32)],
                             ("whole", "edge", "edge", "edge", "smallest", "smallest")):      # (K = 1 is the smallest codebook)
    _add("vq", f"N{_N}_K{_K}_C{_C}", _vq_fn(_N, _K, _C), _kd, atomic="vq_dcodebook")


# ---------------------------------------------------------------------------------------------- sampling
def _sample_fn(B, T, V, mode):
    def fn(device):
        from amk import ops

        logits = seeded((B, T, V), 1, 2.0).to(device)
        null = seeded((B, T, V), 2, 2.0).to(device)
        ids = torch.zeros(B, T, dtype=torch.int64, device=device)
        mask = (torch.arange(B * T).view(B, T) % 3 != 0).to(device)
        if mode == "gumbel":
            u = torch.rand(B, T, V, generator=torch.Generator().manual_seed(3)).clamp_(1e-6, 1 - 1e-6)
            scores = ops.sample_step(logits, ids, mask, null, gumbel=(-torch.log(-torch.log(u))).to(device))
        else:
            # an explicit seed takes the module's call counter as the stream offset (the test puts the counter back)
            ops._SAMPLE_CALLS = 0
            scores = ops.sample_step(logits, ids, mask, null, seed=1234, unmasked_score=2.0)
        return dict(scores=scores, ids=ids)
    return fn


for (_B, _T, _V), _kd in _kinds([(2, 8, 256), (2, 5, 1000), (1, 3, 8196), (1, 1, 4)]):
    for _mode in ("gumbel", "seed"):
        _add("sample_step", f"{_mode}_{_B}x{_T}x{_V}", _sample_fn(_B, _T, _V, _mode), _kd)


# ---------------------------------------------------------------------------------------------- routed experts
def _route_fn(U, E, k):
    def fn(device):
        from amk import ops

        return dict(ops.moe_route(seeded((U, E), 1).to(device), k))
    return fn


for (_U, _E, _k), _kd in _kinds([(256, 8, 2), (257, 5, 2), (1000, 32, 2), (1, 1, 1)]):
    _add("moe_route", f"U{_U}_E{_E}_k{_k}", _route_fn(_U, _E, _k), _kd)


def _routed_fn(U, E, k, N, Kd, bias, bf16, weighted=True, outer=1):
    def fn(device):
        from amk import ops

        x_div = k                             # a unit's k pairs read its row (MoELayer; SwitchHead's moe_out with outer = h)
        x = seeded((U * k // x_div, Kd), 1).to(device).requires_grad_()
        logits = seeded((U, E), 2).to(device).requires_grad_()
        W = seeded((E, N, Kd), 3, Kd ** -0.5).to(device).requires_grad_()
        b = seeded((E, N), 4, 0.1).to(device).requires_grad_() if bias else None
        with _autocast(bf16):
            out, ids = ops.routed_linear(x, logits, W, b, k, x_div, weighted, outer)
        assert type(out.grad_fn).__name__ == ("_RoutedLinearBF16Backward" if bf16 else "_RoutedLinearBackward")
        wrt = [t for t in (x, logits if weighted else None, W, b) if t is not None]
        grads = torch.autograd.grad(out, wrt, seeded(tuple(out.shape), 5).to(device))
        res = dict(out=out, ids=ids)
        res.update({f"grad{i}": g for i, g in enumerate(grads)})
        return res
    return fn


def _routed_bf16_ref(U, E, k, N, Kd, bias):
    """tests/moe_bf16_ref.py (ref_op): out, dx, dlogits, dw and db of ops.routed_linear under bf16 autocast within the
    composed per-element bounds."""
    def ref(got, device):
        import moe_bf16_ref
        from amk import ops

        x, logits = seeded((U, Kd), 1).to(device), seeded((U, E), 2).to(device)
        W = seeded((E, N, Kd), 3, Kd ** -0.5).to(device)
        b = seeded((E, N), 4, 0.1).to(device) if bias else None
        d_out = seeded((U, N), 5).to(device)
        route = ops.moe_route(logits, k)
        assert torch.equal(route["ids"], got["ids"])
        R = moe_bf16_ref.ref_op(x, logits, W, b, d_out, route, k)
        names = [("out", "out"), ("dx", "grad0"), ("dlogits", "grad1"), ("dw", "grad2")] + ([("db", "grad3")] if bias else [])
        for name, key in names:
            moe_bf16_ref.assert_bounded(got[key], R, name, "stale-memory case")
    return ref


def _wgrad_split_path():
    """The routed weight gradient in two halves (rsplit == 2 of csrc/moe.hip:1552): what tests/moe_ref.py's model of the host
    code, held to a table by tests/test_moe_bounds.py, gives for this launch on this GPU."""
    def check(seen):
        import moe_ref

        slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
        name = moe_ref.expected_path("wgrad", 1024, 2, 128, 64, 0, [512, 512], slots)
        assert name == "wgrad_wide<128,64,scale> rsplit 2", name
        assert [n for n, _ in seen] == ["amk_grouped_gemm_wgrad"] * 2, seen
    return dict(entries=("amk_grouped_gemm_wgrad",), check=check)


for _bf in (False, True):
    _f = "moe_routed_bf16" if _bf else "moe_routed"
    # the 128-wide tiles, whole; one past, five experts (one may be empty); under 64 either way: the narrow kernels; one row,
    # one expert
    for _nm, _kd, (_U, _E, _k, _N, _Kd, _bias) in [("whole_wide", "whole", (128, 4, 2, 128, 64, True)),
                                                    ("edge_wide", "edge", (129, 5, 2, 136, 72, True)),
                                                    ("narrow", "edge", (65, 3, 2, 40, 24, False)),
                                                    ("smallest", "smallest", (1, 1, 1, 8, 8, True))]:
        _add(_f, _nm, _routed_fn(_U, _E, _k, _N, _Kd, _bias, _bf), _kd,
             ref=_routed_bf16_ref(_U, _E, _k, _N, _Kd, _bias) if _bf else None)
_add("moe_routed", "unweighted_outer2", _routed_fn(66, 4, 2, 40, 24, False, False, weighted=False, outer=2), "edge")
# 512 pairs per expert: dW in two halves
_add("moe_routed", "wgrad_split", _routed_fn(512, 2, 2, 128, 64, True, False), "whole", path=_wgrad_split_path())


def _switchhead_fn(which, G, H, E, k, dim, d, bf16):
    def fn(device):
        from amk import ops

        U = G * H
        logits = seeded((U, E), 2).to(device).requires_grad_()
        with _autocast(bf16):
            if which == "shared":            # V experts: (G, dim) -> (U, d)
                a = seeded((G, dim), 1).to(device).requires_grad_()
                W = seeded((E, d, dim), 3, dim ** -0.5).to(device).requires_grad_()
                out, ids = ops.shared_row_experts(a, logits, W, k, H)
                wrt = (a, logits, W)
            else:                            # output experts + head sum: (U, d) -> (G, dim)
                a = seeded((U, d), 1).to(device).requires_grad_()
                W = seeded((E, dim, d), 3, d ** -0.5).to(device).requires_grad_()
                out, ids = ops.summed_experts(a, logits, W, k, H)
                wrt = (a, W)
        want = {"shared": "_SharedRowExperts", "summed": "_SummedExperts"}[which] + ("BF16" if bf16 else "") + "Backward"
        assert type(out.grad_fn).__name__ == want
        grads = torch.autograd.grad(out, wrt, seeded(tuple(out.shape), 5).to(device=device, dtype=out.dtype))
        res = dict(out=out, ids=ids)
        res.update({f"grad{i}": g for i, g in enumerate(grads)})
        return res
    return fn


def _switchhead_bf16_ref(which, G, H, E, k, dim, d):
    """tests/switchhead_bf16_ref.py (ref_shared_row / ref_summed): the op's outputs and gradients under bf16 autocast within
    the composed per-element bounds."""
    def ref(got, device):
        import switchhead_bf16_ref as sref
        from amk import ops

        U = G * H
        logits = seeded((U, E), 2).to(device)
        ids, gate = ops._topk(logits, k)
        assert torch.equal(ids, got["ids"])
        if which == "shared":
            a, W = seeded((G, dim), 1).to(device), seeded((E, d, dim), 3, dim ** -0.5).to(device)
            R = sref.ref_shared_row(a, logits, W, seeded((U, d), 5).to(device), ids, gate, k, H)
            names = (("out", "out"), ("dx", "grad0"), ("dlogits", "grad1"), ("dw", "grad2"))
        else:
            a, W = seeded((U, d), 1).to(device), seeded((E, dim, d), 3, d ** -0.5).to(device)
            R = sref.ref_summed(a, logits, W, seeded((G, dim), 5).to(device=device, dtype=BF16), ids, k, H)
            names = (("out", "out"), ("da", "grad0"), ("dw", "grad1"))
        for name, key in names:
            sref.assert_bounded(got[key], R, name, "stale-memory case")
    return ref


for _bf in (False, True):
    for _which in ("shared", "summed"):
        _f = f"switchhead_{_which}" + ("_bf16" if _bf else "")
        # (G, H, E, k, dim, d) after switchhead_bf16_ref.OP_SHAPES: whole, one past, odd, smallest
        for (_G, _H, _E, _k, _dim, _d), _kd in _kinds([(128, 4, 4, 2, 256, 64), (130, 4, 4, 2, 256, 64), (65, 4, 5, 3, 264, 64),
                                                       (97, 8, 8, 2, 256, 32), (1, 1, 1, 1, 8, 8)]):
            _add(_f, f"G{_G}_H{_H}_E{_E}_k{_k}_dim{_dim}_d{_d}", _switchhead_fn(_which, _G, _H, _E, _k, _dim, _d, _bf), _kd,
                 ref=_switchhead_bf16_ref(_which, _G, _H, _E, _k, _dim, _d) if _bf else None)


# ---------------------------------------------------------------------------------------------- row kernels
def _gate_fn(kind, M, H, bf16):
    def fn(device):
        from amk import ops

        ab = seeded((M, 2 * H), 1, 2.0).to(device=device, dtype=BF16 if bf16 else F32).requires_grad_()
        out = (ops.swiglu if kind == "swiglu" else ops.geglu)(ab)
        want = {"swiglu": "_SwiGLUBF16Backward" if bf16 else "_SwiGLUBackward", "geglu": "_GEGLUBackward"}[kind]
        assert type(out.grad_fn).__name__ == want
        (d_ab,) = torch.autograd.grad(out, ab, seeded((M, H), 2).to(device=device, dtype=out.dtype))
        return dict(out=out, d_ab=d_ab)
    return fn


def _gate_ref(kind, M, H, bf16):
    """tests/row_f32_ref.py (ref_swiglu, ref_geglu): out, da and db of the f32 gates within their per-element bounds;
    tests/bf16_dense_ref.py (ref_swiglu_mixed) for the bf16 SwiGLU."""
    def ref(got, device):
        import bf16_dense_ref
        import row_f32_ref

        ab, cot = seeded((M, 2 * H), 1, 2.0), seeded((M, H), 2)
        if bf16:
            R = bf16_dense_ref.ref_swiglu_mixed(ab.to(BF16), cot.to(BF16))
            bf16_dense_ref.assert_within({"g": got["out"], "dab": got["d_ab"]}, R, ("g", "dab"), "stale-memory case")
        else:
            view = {"out": got["out"], "da": got["d_ab"][:, :H], "db": got["d_ab"][:, H:]}
            bf16_dense_ref.assert_within(view, row_f32_ref.REF_GATE[kind](ab, cot), row_f32_ref.GATE_OUT, "stale-memory case")
    return ref


_ROW_KINDS = ("whole", "smallest", "edge", "edge", "edge", "edge", "edge")       # the row lists start whole, then the smallest
for (_M, _H), _kd in zip([(64, 64), (1, 4), (7, 20), (33, 96), (5, 1368), (257, 8)], _ROW_KINDS):   # row_f32_ref.GATE_SHAPES and whole / one past
    _add("swiglu", f"f32_{_M}x{_H}", _gate_fn("swiglu", _M, _H, False), _kd, ref=_gate_ref("swiglu", _M, _H, False))
    _add("geglu", f"f32_{_M}x{_H}", _gate_fn("geglu", _M, _H, False), _kd, ref=_gate_ref("geglu", _M, _H, False))
    _add("swiglu_bf16", f"bf16_{_M}x{_H}", _gate_fn("swiglu", _M, _H, True), _kd, ref=_gate_ref("swiglu", _M, _H, True))


def _ln_inputs(M, D):
    import row_f32_ref

    return row_f32_ref.make_ln("unit", M, D, 1)      # x, res, gamma, beta, the cotangents of y and of h


def _ln_ref(kind, M, D):
    """tests/row_f32_ref.py (ref_ln): the f32 LayerNorm's outputs and gradients within their per-element bounds."""
    def ref(got, device):
        import bf16_dense_ref
        import row_f32_ref

        x, r, w, b, cy, ch = _ln_inputs(M, D)
        if kind in ("add_ln_mixed", "ln_mixed", "ln_to_bf16"):
            # tests/bf16_dense_ref.py (ref_ln), as tests/test_mixed_gpu.py holds the mixed LayerNorm: y in bf16 on a bf16
            # cotangent; with a residual h and its gradient in f32, and the bf16 gradient of a bf16 x
            if kind == "ln_mixed":
                R = bf16_dense_ref.ref_ln(x, None, w, b, cy.to(BF16), None)
                view = dict(y=got["y"], dgamma=got["dw"], dbeta=got["db"])
            else:
                R = bf16_dense_ref.ref_ln(x.to(BF16) if kind == "add_ln_mixed" else x, r, w, b, cy.to(BF16), ch)
                view = dict(y=got["y"], dgamma=got["dw"], dbeta=got["db"], h=got["h"], dh=got["dres"])
                if kind == "add_ln_mixed":
                    view["dh16"] = got["dx"]
            bf16_dense_ref.assert_within(view, R, tuple(view), "stale-memory case")
            return
        if kind == "ln":
            R = row_f32_ref.ref_ln(x, None, w, b, cy, None)
            view = dict(y=got["y"], dh=got["dx"], dgamma=got["dw"], dbeta=got["db"])
        else:
            R = row_f32_ref.ref_ln(x, r, w, b, cy, ch)
            assert torch.equal(got["dx"], got["dres"])
            view = dict(h=got["h"], y=got["y"], dh=got["dx"], dgamma=got["dw"], dbeta=got["db"])
        res = bf16_dense_ref.ratios(view, R, list(view))
        assert all(nbad == 0 for nbad, _ in res.values()), res
    return ref


def _ln_fn(kind, M, D):
    def fn(device):
        from amk import ops

        x, r, w, b, cy, ch = (t.to(device) for t in _ln_inputs(M, D))
        x, r, w, b = (t.requires_grad_() for t in (x, r, w, b))
        if kind == "ln":
            y = ops.layer_norm(x, w, b)
            g = torch.autograd.grad(y, (x, w, b), cy)
            return dict(y=y, dx=g[0], dw=g[1], db=g[2])
        if kind == "add_ln":
            h, y = ops.add_layer_norm(x, r, w, b)
            g = torch.autograd.grad((h, y), (x, r, w, b), (ch, cy))
            return dict(h=h, y=y, dx=g[0], dres=g[1], dw=g[2], db=g[3])
        if kind == "add_ln_mixed":           # under autocast, the branch's input in bf16
            xb = x.detach().to(BF16).requires_grad_()
            with _autocast(True):
                h, y = ops.add_layer_norm(xb, r, w, b, branch=True)
            assert y.dtype == BF16 and type(y.grad_fn).__name__ == "_AddLayerNormMixedBackward"
            g = torch.autograd.grad((h, y), (xb, r, w, b), (ch, cy.to(BF16)))
            return dict(h=h, y=y, dx=g[0], dres=g[1], dw=g[2], db=g[3])
        if kind == "ln_mixed":               # f32 x, no residual: no h is written
            with _autocast(True):
                y = ops.layer_norm(x, w, b, branch=True)
            assert y.dtype == BF16
            g = torch.autograd.grad(y, (x, w, b), cy.to(BF16))
            return dict(y=y, dx=g[0], dw=g[1], db=g[2])
        h, y = ops.layer_norm_to_bf16(x, r, w, b)       # the plain entry point, autocast disabled by the caller
        g = torch.autograd.grad((h, y), (x, r, w, b), (ch, cy))
        return dict(h=h, y=y, dx=g[0], dres=g[1], dw=g[2], db=g[3])
    return fn


for (_M, _D), _kd in zip([(64, 256), (1, 4), (5, 4), (37, 260), (9, 1028), (5, 4096), (257, 8)], _ROW_KINDS):      # after row_f32_ref.LN_SHAPES
    for _kind in ("ln", "add_ln", "add_ln_mixed", "ln_mixed", "ln_to_bf16"):
        _add({"ln": "layer_norm", "add_ln": "add_layer_norm", "add_ln_mixed": "add_layer_norm_mixed",
              "ln_mixed": "add_layer_norm_mixed", "ln_to_bf16": "layer_norm_to_bf16"}[_kind], f"{_kind}_{_M}x{_D}",
             _ln_fn(_kind, _M, _D), _kd, ref=_ln_ref(_kind, _M, _D))


def _colsum_fn(M, N):
    def fn(device):
        from amk import ops

        return dict(colsum=ops.colsum(seeded((M, N), 1).to(device)))
    return fn


def _colsum_ref(M, N):
    """tests/row_f32_ref.py (ref_colsum): every column sum within its bound."""
    def ref(got, device):
        import bf16_dense_ref
        import row_f32_ref

        bf16_dense_ref.assert_within(got, row_f32_ref.ref_colsum(seeded((M, N), 1)), ("colsum",), "stale-memory case")
    return ref


for (_M, _N), _kd in zip([(256, 256), (1, 4), (3, 260), (8195, 256), (70, 1024), (257, 8)], _ROW_KINDS):            # row_f32_ref.COL_SHAPES
    _add("colsum", f"{_M}x{_N}", _colsum_fn(_M, _N), _kd, ref=_colsum_ref(_M, _N))


def _row_stats_fn(M, D):
    def fn(device):
        from amk import dense

        mean, rstd = dense.row_stats(seeded((M, D), 1).to(device))
        return dict(mean=mean, rstd=rstd)
    return fn


def _row_stats_ref(M, D):
    """tests/dense_f32_ref.py (ref_row_stats): mean and rstd of every row within their bounds, as
    tests/test_dense_f32_bounds_gpu.py holds dense.row_stats."""
    def ref(got, device):
        import dense_f32_ref

        R = dense_f32_ref.ref_row_stats(seeded((M, D), 1))
        dense_f32_ref.assert_within(got["mean"], R, "mean", "row_stats_mean", "stale-memory case")
        dense_f32_ref.assert_within(got["rstd"], R, "rstd", "row_stats_rstd", "stale-memory case")
    return ref


# amk_row_stats (dense.row_stats; found without a case by the entry-point guard): the widths at which row_stats_kernel's
# NCH changes (dense_f32_ref.stats_nch: 256 | 1024), one past each, the smallest
for (_M, _D), _kd in zip([(64, 256), (1, 4), (37, 260), (5, 1028), (257, 8)], _ROW_KINDS):
    _add("row_stats", f"{_M}x{_D}", _row_stats_fn(_M, _D), _kd, ref=_row_stats_ref(_M, _D))


# ---------------------------------------------------------------------------------------------- Linear layers, f32
def _lin(fn_out, params, x, cot_seed=9):
    out = fn_out()
    outs = out if isinstance(out, tuple) else (out,)
    cots = tuple(seeded(tuple(o.shape), cot_seed + i).to(device=o.device, dtype=o.dtype) for i, o in enumerate(outs))
    grads = torch.autograd.grad(outs, [x] + params, cots)
    res = {f"out{i}": o for i, o in enumerate(outs)}
    res.update({f"grad{i}": g for i, g in enumerate(grads)})
    return res


def _linear_fn(M, N, K, want, bias=True):
    def fn(device):
        from amk import ops

        x = seeded((M, K), 1).to(device).requires_grad_()
        w = seeded((N, K), 2, K ** -0.5).to(device).requires_grad_()
        b = seeded((N,), 3, 0.1).to(device).requires_grad_() if bias else None
        res = _lin(lambda: ops.linear(x, w, b), [w] + ([b] if bias else []), x)
        assert type(res["out0"].grad_fn).__name__ == want + "Backward"
        return res
    return fn


def _linear2_fn(M, Na, Nb, K):
    def fn(device):
        from amk import ops

        x = seeded((M, K), 1).to(device).requires_grad_()
        wa = seeded((Na, K), 2, K ** -0.5).to(device).requires_grad_()
        wb = seeded((Nb, K), 3, K ** -0.5).to(device).requires_grad_()
        return _lin(lambda: ops.linear2(x, wa, wb), [wa, wb], x)
    return fn


def _ffn_fn(M, K, H, N):
    def fn(device):
        from amk import ops

        x = seeded((M, K), 1).to(device).requires_grad_()
        w12 = seeded((2 * H, K), 2, K ** -0.5).to(device).requires_grad_()
        b12 = seeded((2 * H,), 3, 0.1).to(device).requires_grad_()
        w3 = seeded((N, H), 4, H ** -0.5).to(device).requires_grad_()
        b3 = seeded((N,), 5, 0.1).to(device).requires_grad_()
        return _lin(lambda: ops.swiglu_ffn(x, w12, b12, w3, b3), [w12, b12, w3, b3], x)
    return fn


_AMK = dict(DENSE_MODE="amk", GEMM_MODE="f32")
# the f32 tiles are 128 wide (csrc/gemm_f32.hip): whole, +-4 around one and two tiles, the smallest the gate lets through
for (_M, _N, _K), _kd in _kinds([(128, 128, 128), (132, 124 + 8, 132), (124, 260, 260), (1, 128, 128)]):
    _add("dense_linear", f"{_M}x{_N}x{_K}", _linear_fn(_M, _N, _K, "_DenseLinear"), _kd, switches=_AMK)
    _add("dense_linear", f"auto_{_M}x{_N}x{_K}", _linear_fn(_M, _N, _K, "_DenseLinear"), _kd,
         switches=dict(DENSE_MODE="auto", GEMM_MODE="f32"))
    _add("dense_linear2", f"{_M}x128+{_N}x{_K}", _linear2_fn(_M, 128, _N, _K), _kd, switches=_AMK)
    _add("swiglu_ffn", f"{_M}x{_K}x{_N}", _ffn_fn(_M, _K, _N, 128 if _N == 128 else 132), _kd, switches=_AMK)
    _add("linear_x6", f"{_M}x{_N}x{_K}", _linear_fn(_M, _N, _K, "_LinearX6"), _kd, switches=dict(GEMM_MODE="bf16x6"))
_add("linear_x6", "1x4x4", _linear_fn(1, 4, 4, "_LinearX6"), "smallest", switches=dict(GEMM_MODE="bf16x6"))
_add("linear_x6", "33x6x36_mm_dx", _linear_fn(33, 6, 36, "_LinearX6"), "edge", switches=dict(GEMM_MODE="bf16x6"))   # N % 4: dX by mm
# K < 128: the library's GEMMs with the bias gradient by amk_colsum
for (_M, _N, _K), _kd in zip([(64, 64, 64), (65, 20, 36), (257, 1024, 8), (1, 4, 4), (9, 1028, 12)],
                             ("whole", "edge", "edge", "smallest", "edge")):
    _add("bias_linear", f"{_M}x{_N}x{_K}", _linear_fn(_M, _N, _K, "_BiasLinear"), _kd, switches=dict(GEMM_MODE="f32"))


class _PlaneNet(nn.Module):
    """One Linear, one q / kv pair and one SwiGLU FFN whose weights carry the optimizer's split-bf16 planes."""

    def __init__(self, K, N, H):
        super().__init__()
        self.lin = nn.Linear(K, N)
        self.q, self.kv = nn.Linear(K, 128, bias=False), nn.Linear(K, N, bias=False)
        self.w12, self.w3 = nn.Linear(K, 2 * H), nn.Linear(H, N)


def _planes_fn(M, K, N, H, forms):
    def fn(device):
        from amk import ops
        from amk.dp import GradReducer
        from amk.optim import FlatAdam

        torch.manual_seed(0)
        net = _PlaneNet(K, N, H).to(device)
        opt = FlatAdam(GradReducer(net.parameters(), bucket_bytes=64 << 10), lr=1e-3)
        opt.enable_planes(gate=[net.w12.weight], transposed="dx" in forms)
        x = seeded((M, K), 1).to(device).requires_grad_()
        res = {}
        with _switches(X6_AUTO_FORMS=frozenset(forms)):
            y = ops.linear(x, net.lin.weight, net.lin.bias)
            a, b = ops.linear2(x, net.q.weight, net.kv.weight)
            f = ops.swiglu_ffn(x, net.w12.weight, net.w12.bias, net.w3.weight, net.w3.bias)
            names = [type(t.grad_fn).__name__ for t in (y, a, f)]
            assert names == ["_X6LinearBackward", "_X6Linear2Backward", "_X6SwiGLUFFNBackward"], names
            params = [p for p in net.parameters()]
            cots = [seeded(tuple(t.shape), 7 + i).to(device) for i, t in enumerate((y, a, b, f))]
            grads = torch.autograd.grad((y, a, b, f), [x] + params, cots)
        res.update(y=y, a=a, b=b, f=f)
        res.update({f"grad{i}": g for i, g in enumerate(grads)})
        return res
    return fn


for _forms in (("fwd", "dw"), ("fwd", "dx", "dw"), ("fwd",)):
    for (_M, _K, _N, _H), _kd in _kinds([(128, 128, 128, 128), (132, 132, 260, 132), (124, 260, 132, 164), (1, 128, 128, 128)]):
        _add("x6_linear_planes", f"{'+'.join(_forms)}_{_M}x{_K}x{_N}x{_H}", _planes_fn(_M, _K, _N, _H, _forms), _kd,
             switches=dict(GEMM_MODE="auto", X6_LINEAR=True))


# ---------------------------------------------------------------------------------------------- Linear layers, bf16 autocast
def _mixed_fn(kind, M, K, N, H=0):
    def fn(device):
        from amk import ops

        x = seeded((M, K), 1).to(device).requires_grad_()
        with _autocast(True):
            if kind == "linear":
                w = seeded((N, K), 2, K ** -0.5).to(device).requires_grad_()
                b = seeded((N,), 3, 0.1).to(device).requires_grad_()
                res = _lin(lambda: ops.linear(x, w, b), [w, b], x)
                want = "_LinearMixedBackward"
            elif kind == "swiglu_ffn":
                w12 = seeded((2 * H, K), 2, K ** -0.5).to(device).requires_grad_()
                b12 = seeded((2 * H,), 3, 0.1).to(device).requires_grad_()
                w3 = seeded((N, H), 4, H ** -0.5).to(device).requires_grad_()
                b3 = seeded((N,), 5, 0.1).to(device).requires_grad_()
                res = _lin(lambda: ops.swiglu_ffn(x, w12, b12, w3, b3), [w12, b12, w3, b3], x)
                want = "_SwiGLUFFNMixedBackward"
            else:
                w1 = seeded((2 * H, K), 2, K ** -0.5).to(device).requires_grad_()
                gamma = (1.0 + seeded((H,), 3, 0.1)).to(device).requires_grad_()
                beta = seeded((H,), 4, 0.1).to(device).requires_grad_()
                w2 = seeded((N, H), 5, H ** -0.5).to(device).requires_grad_()
                res = _lin(lambda: ops.geglu_ffn(x, w1, gamma, beta, w2), [w1, gamma, beta, w2], x)
                want = "_GEGLUFFNMixedBackward"
        assert type(res["out0"].grad_fn).__name__ == want
        return res
    return fn


# csrc/gemm_bf16.hip: 128-row tiles, gradient tiles of 128 x 128
for (_M, _K, _N), _kd in _kinds([(128, 128, 128), (132, 136, 264), (124, 24, 136), (1, 8, 8)]):
    _add("linear_mixed", f"{_M}x{_K}x{_N}", _mixed_fn("linear", _M, _K, _N), _kd)
for (_M, _K, _N, _H), _kd in _kinds([(128, 128, 128, 512), (132, 136, 264, 520), (1, 8, 8, 512)]):      # (the fused form from 2 H = 1024 on)
    _add("swiglu_ffn_mixed", f"{_M}x{_K}x{_N}x{_H}", _mixed_fn("swiglu_ffn", _M, _K, _N, _H), _kd)
for (_M, _K, _N, _H), _kd in _kinds([(128, 128, 128, 256), (132, 136, 136, 264), (37, 24, 24, 4096), (1, 8, 8, 8)]):      # (dim -> inner -> dim)
    _add("geglu_ffn_mixed", f"{_M}x{_K}x{_N}x{_H}", _mixed_fn("geglu_ffn", _M, _K, _N, _H), _kd)


def _geglu_identity_fn(M, H):
    """_GEGLUFFNMixed with dim = 2H, w1 = I and w2 = (I | 0)^T, the construction of tests/test_geglu_ln_bf16_gpu.py: x = ab
    passes through w1 exactly and y through w2 into the first H output columns, so the Function's output and gradients are
    the fused kernels' y, d_ab, dgamma and dbeta, which tests/geglu_ln_bf16_ref.py bounds."""
    def fn(device):
        import geglu_ln_bf16_ref
        from amk import ops

        ab, dy, gamma, beta = geglu_ln_bf16_ref.make_inputs("diffuse", M, H)
        x = ab.to(device).requires_grad_()
        w1 = torch.eye(2 * H, device=device).requires_grad_()
        w2 = torch.eye(2 * H, H, device=device).requires_grad_()
        gm, bt = gamma.to(device).requires_grad_(), beta.to(device).requires_grad_()
        with _autocast(True):
            assert ops.geglu_ffn_ok(x, w1, gm, bt, w2)
            out = ops.geglu_ffn(x, w1, gm, bt, w2, geglu_ln_bf16_ref.EPS)
        assert type(out.grad_fn).__name__ == "_GEGLUFFNMixedBackward"
        d_ab, dgm, dbt, dw1, dw2 = torch.autograd.grad(out, (x, gm, bt, w1, w2),
                                                       torch.cat([dy, torch.zeros_like(dy)], dim=1).to(device))
        return dict(y=out[:, :H], rest=out[:, H:], d_ab=d_ab, dgamma=dgm, dbeta=dbt, dw1=dw1, dw2=dw2)
    return fn


def _geglu_identity_ref(M, H):
    def ref(got, device):
        import geglu_ln_bf16_ref

        R = geglu_ln_bf16_ref.reference(*geglu_ln_bf16_ref.make_inputs("diffuse", M, H))
        assert not bool(got["rest"].any())
        names = ("y", "d_ab", "dgamma", "dbeta")
        q = geglu_ln_bf16_ref.ratios({k: got[k].cpu() for k in names}, R, names=names, record=False)
        assert all(v <= 1.0 for v in q.values()), q
    return ref


# widths of tests/test_geglu_ln_bf16_gpu.py: whole vectors, a tail past 256 and past 1024, the smallest
for (_M, _H), _kd in _kinds([(64, 256), (67, 264), (5, 1032), (1, 8)]):
    _add("geglu_ffn_mixed", f"identity_{_M}x{_H}", _geglu_identity_fn(_M, _H), _kd, ref=_geglu_identity_ref(_M, _H),
         switches=dict(GEGLU_FFN_BF16=True))


def _rows_fn(M, N, K, out_dtype, bias):
    def fn(device):
        from amk import ops

        x = seeded((M, K), 1).to(device=device, dtype=BF16)
        w = seeded((N, K), 2, K ** -0.5).to(device=device, dtype=BF16)
        b = seeded((N,), 3, 0.1).to(device) if bias else None
        with torch.no_grad():
            return dict(rows_bf16=ops.linear_rows_bf16(x, w, b, out_dtype), rows=ops.linear_rows(x, w, b, out_dtype))
    return fn


for (_M, _N, _K), _kd in zip([(8, 64, 64), (17, 65, 72), (1, 1, 8), (64, 300, 1030), (5, 7, 20)],      # (K not a multiple of 8: padded copies)
                             ("whole", "edge", "smallest", "edge", "edge")):
    _add("linear_rows", f"{_M}x{_N}x{_K}", _rows_fn(_M, _N, _K, BF16 if _N % 2 else F32, _M != 1), _kd)


# ---------------------------------------------------------------------------------------------- norms of the conv models
def _bn_inputs(shape, bf16=False):
    import discr_norm_bf16_ref
    import discr_norm_ref

    # (for the bf16 kernels x, gz and ggx are bf16 values)
    return (discr_norm_bf16_ref if bf16 else discr_norm_ref).make_inputs("diffuse", shape)


def _bn_fn(shape, bf16):
    def fn(device):
        from amk import ops

        import discr_norm_ref

        inp, slope = _bn_inputs(shape, bf16), discr_norm_ref.SLOPE
        bn = nn.BatchNorm2d(shape[1])
        with torch.no_grad():
            bn.weight.copy_(inp["gamma"])
            bn.bias.copy_(inp["beta"])
            bn.running_mean.copy_(inp["run_mean"])
            bn.running_var.copy_(inp["run_var"])
        bn = bn.to(device)
        dt = BF16 if bf16 else F32
        x = inp["x"].to(device=device, dtype=dt).requires_grad_()
        gz = inp["gz"].to(device=device, dtype=dt).requires_grad_()
        ggx = inp["ggx"].to(device=device, dtype=dt)
        if bf16:
            assert ops.bn_leaky_relu_bf16_ok(bn, x)
            z = ops.bn_leaky_relu_bf16(x, bn, slope)
        else:
            assert ops.bn_leaky_relu_ok(bn, x)
            z = ops.bn_leaky_relu(x, bn, slope)
        gx, gw, gb = torch.autograd.grad(z, (x, bn.weight, bn.bias), gz, create_graph=True)
        # the double backward, every second-order input given
        g_x, g_w, g_gz = torch.autograd.grad((gx, gw, gb), (x, bn.weight, gz),
                                             (ggx, inp["gg_gamma"].to(device), inp["gg_beta"].to(device)))
        return dict(z=z, run_mean=bn.running_mean, run_var=bn.running_var, gx=gx, dgamma=gw, dbeta=gb, g_x=g_x, g_gamma=g_w,
                    g_gz=g_gz)
    return fn


def _bn_ref(shape, bf16):
    """tests/discr_norm_ref.py: every tensor of forward, backward and double backward within its per-element bound;
    tests/discr_norm_bf16_ref.py for the bf16 kernels (the bf16 outputs inside RNE's image of their bound)."""
    def ref(got, device):
        import discr_norm_bf16_ref
        import discr_norm_ref

        mod = discr_norm_bf16_ref if bf16 else discr_norm_ref
        R = mod.reference(_bn_inputs(shape, bf16), "diffuse")
        q = mod.ratios({k: v.cpu() for k, v in got.items()}, R, names=list(got), record=False, family="diffuse")
        assert all(v <= 1.0 for v in q.values()), q
    return ref


# discr_norm_ref.CPU_SHAPES / GPU_SHAPES: HW 1, 2, 961, 4225 (odd), 4096 (== the segment), 4160 (just over), 196, 4097
for _shape, _kd in zip([(2, 4, 8, 8), (2, 3, 1, 1), (1, 2, 1, 2), (5, 4, 31, 31), (2, 3, 65, 65), (2, 5, 64, 64), (2, 3, 64, 65),
                        (3, 2, 14, 14), (1, 2, 4097, 1)],
                       ("whole", "smallest", "edge", "edge", "edge", "whole", "edge", "edge", "edge")):
    _s = "x".join(map(str, _shape))
    _add("bn_act", _s, _bn_fn(_shape, False), _kd, ref=_bn_ref(_shape, False))
    _add("bn_act_bf16", _s, _bn_fn(_shape, True), _kd, ref=_bn_ref(_shape, True))


def _gn_inputs(shape, G, bf16=False):
    import gn_act_bf16_ref
    import gn_act_ref

    # (for the bf16 kernels x and gz are bf16 values)
    return (gn_act_bf16_ref if bf16 else gn_act_ref).make_inputs("diffuse", tuple(shape) + (G,), seed=3)


def _gn_fn(shape, G, act, bf16):
    def fn(device):
        from amk import ops

        inp = _gn_inputs(shape, G, bf16)
        gn = nn.GroupNorm(G, shape[1], eps=1e-6)
        with torch.no_grad():
            gn.weight.copy_(inp["gamma"])
            gn.bias.copy_(inp["beta"])
        gn = gn.to(device)
        dt = BF16 if bf16 else F32
        x = inp["x"].to(device=device, dtype=dt).requires_grad_()
        with _autocast(bf16), _switches(GN_ACT=True, GN_ACT_BF16=True):
            z = ops.group_norm_act(x, gn, act)
        assert type(z.grad_fn).__name__ == ("_GNActBF16Backward" if bf16 else "_GNActBackward")
        gx, gw, gb = torch.autograd.grad(z, (x, gn.weight, gn.bias), inp["gz"].to(device=device, dtype=z.dtype))
        return dict(z=z, gx=gx, dgamma=gw, dbeta=gb)
    return fn


def _gn_ref(shape, G, act, bf16):
    """tests/gn_act_ref.py: every element of z, gx, dgamma and dbeta within its bound of the float64 reference;
    tests/gn_act_bf16_ref.py for the bf16 kernels (z and gx inside RNE's image of their bound)."""
    def ref(got, device):
        import gn_act_bf16_ref
        import gn_act_ref

        mod = gn_act_bf16_ref if bf16 else gn_act_ref
        R = mod.reference(_gn_inputs(shape, G, bf16), G, act)
        q = mod.ratios({k: v.cpu() for k, v in got.items()}, R, names=("z", "gx", "dgamma", "dbeta"), record=False)
        assert all(v <= 1.0 for v in q.values()), q
    return ref


# gn_act_ref.CASES (cpg 1 with runs of 9, HW = 1, odd HW, a run of 1024, a run past a segment edge, G = 1 and G = C), and
# HW = 14^2 and 4097
for (_shape, _G), _kd in zip([((2, 128, 16, 16), 32), ((2, 32, 3, 3), 32), ((1, 64, 1, 1), 32), ((3, 64, 5, 7), 32),
                              ((1, 256, 33, 31), 32), ((2, 48, 6, 6), 1), ((2, 48, 6, 6), 48), ((1, 32, 14, 14), 32),
                              ((1, 32, 4097, 1), 32)],
                             ("whole", "edge", "smallest", "edge", "edge", "edge", "edge", "edge", "edge")):
    for _act in (0, 1):
        _s = "x".join(map(str, _shape)) + f"_G{_G}_act{_act}"
        _add("gn_act", _s, _gn_fn(_shape, _G, _act, False), _kd, ref=_gn_ref(_shape, _G, _act, False))
        _add("gn_act_bf16", _s, _gn_fn(_shape, _G, _act, True), _kd, ref=_gn_ref(_shape, _G, _act, True))


def _lpips_inputs(shape, bf16):
    import lpips_ref

    return lpips_ref.make_inputs("relu", shape, "pos", seed=2, bf16=bf16)


def _lpips_fn(shape, bf16):
    def fn(device):
        from amk import ops

        inp = _lpips_inputs(shape, bf16)
        dt = BF16 if bf16 else F32
        a = inp["a"].to(device=device, dtype=dt).requires_grad_()
        b, w = inp["b"].to(device=device, dtype=dt), inp["w"].to(device)
        with _autocast(bf16), _switches(LPIPS=True):
            assert ops.lpips_distance_ok(a, b, w)
            out = ops.lpips_distance(a, b, w)
        assert type(out.grad_fn).__name__ == "_LpipsDistBackward"
        (ga,) = torch.autograd.grad(out, a, inp["g"].to(device))
        return dict(out=out, ga=ga)
    return fn


def _lpips_ref(shape, bf16):
    """tests/lpips_ref.py: every element within its bound of the float64 reference (ratios <= 1)."""
    def ref(got, device):
        import lpips_ref

        R = lpips_ref.reference(_lpips_inputs(shape, bf16), bf16=bf16)
        q = lpips_ref.ratios(got, R)
        assert q["out"] <= 1.0 and q["ga"] <= 1.0, q
    return ref


for _bf in (False, True):
    for _shape, _kd in zip([(2, 64, 8, 8), (2, 64, 14, 14), (1, 3, 1, 1), (2, 5, 4097, 1), (3, 130, 5, 7)],
                           ("whole", "edge", "smallest", "edge", "edge")):
        _add("lpips_bf16" if _bf else "lpips", "x".join(map(str, _shape)), _lpips_fn(_shape, _bf), _kd, ref=_lpips_ref(_shape, _bf))


# ---------------------------------------------------------------------------------------------- loss head
def _ce_inputs(M, V, K, pattern, bias, bf16):
    """x, w, b (None without a bias), target on the CPU as the four heads' own tests make them: under bf16 x is bf16 and w
    holds bf16 values (an f32 master weight in the op)."""
    import ce_head_bias_ref
    import ce_head_ref

    target = ce_head_ref.make_target(M, V, pattern, seed=M + V)
    x, w = ce_head_bias_ref.make_inputs("unit", M, V, K, target, seed=M + V + K, bf16=bf16)
    b = ce_head_bias_ref.make_bias("unit", x, w, target, seed=M + V) if bias else None
    return x, w, b, target


def _ce_fn(M, V, K, pattern, bias, bf16):
    def fn(device):
        from amk import ops

        x, w, b, t = _ce_inputs(M, V, K, pattern, bias, bf16)
        xg, wg = x.to(device).requires_grad_(), w.float().to(device).requires_grad_()
        bg = b.to(device).requires_grad_() if bias else None
        with _autocast(bf16):
            loss = ops.linear_cross_entropy(xg, wg, t.to(device), -1, bias=bg)
        grads = torch.autograd.grad(loss * 0.7, [xg, wg] + ([bg] if bias else []))
        res = dict(loss=loss, dx=grads[0], dw=grads[1])
        if bias:
            res["db"] = grads[2]
        return res
    return fn


def _ce_ref(M, V, K, pattern, bias, bf16):
    """tests/ce_head_ref.py, ce_head_bf16_ref.py and ce_head_bias_ref.py, each for its head: no element outside the hard bound,
    and the worst q within TIGHT_FACTOR x the emulation's (the two tiers of the heads' own tests)."""
    def ref(got, device):
        import ce_head_bf16_ref
        import ce_head_bias_ref
        import ce_head_ref

        x, w, b, t = (None if v is None else v.to(device) for v in _ce_inputs(M, V, K, pattern, bias, bf16))
        if bias:
            mod, q_emu = ce_head_bias_ref, ce_head_bias_ref.Q_EMU[bf16]
            R = mod.reference(x, w, b, t, -1, 0.7, bf16=bf16)
        else:
            mod = ce_head_bf16_ref if bf16 else ce_head_ref
            q_emu, R = mod.Q_EMU, mod.reference(x, w, t, -1, 0.7)
        for name in ("loss", "dx", "dw") + (("db",) if bias else ()):
            nbad, ratio, q = mod.measures(got[name], R, name)
            assert nbad == 0, f"{name}: {nbad} elements outside the hard bound (worst {ratio:.3f} x)"
            assert q <= mod.TIGHT_FACTOR * q_emu[name], f"{name}: q {q:.3f} above {mod.TIGHT_FACTOR} x Q_EMU = {q_emu[name]}"
    return ref


# tests/test_ce_head_gpu.py's tile-edge lists: M 1 / 128 / 129 / 300, V 1 / 4 / 128 / 129 / 1000, K 4 / 36 / 64 / 260 (8 / 40 under bf16)
for _bf in (False, True):
    for _bias in (False, True):
        _f = "ce_head" + ("_bias" if _bias else "") + ("_bf16" if _bf else "")
        for (_M, _V, _K, _pat), _kd in zip([(128, 128, 64, "all"), (129, 129, 40 if _bf else 36, "random64"),
                                            (300, 1000, 264 if _bf else 260, "edges"), (1, 1, 8 if _bf else 4, "all"),
                                            (127, 4, 64, "last_tile")], ("whole", "edge", "edge", "smallest", "edge")):
            _add(_f, f"{_M}x{_V}x{_K}_{_pat}", _ce_fn(_M, _V, _K, _pat, _bias, _bf), _kd, ref=_ce_ref(_M, _V, _K, _pat, _bias, _bf))


def _ce_none_valid_fn(bias, bf16):
    def fn(device):
        from amk import ops

        xg = seeded((37, 64), 1).to(device).requires_grad_()
        wg = seeded((50, 64), 2).to(device).requires_grad_()
        bg = seeded((50,), 3).to(device).requires_grad_() if bias else None
        with _autocast(bf16):
            loss = ops.linear_cross_entropy(xg, wg, torch.full((37,), -1, dtype=torch.int64, device=device), -1, bias=bg)
        return dict(loss=loss)
    return fn


for _bf in (False, True):
    for _bias in (False, True):
        _add("ce_head" + ("_bias" if _bias else "") + ("_bf16" if _bf else ""), "no_valid_row", _ce_none_valid_fn(_bias, _bf),
             "edge", allow_nan=("loss",))


# ---------------------------------------------------------------------------------------------- the optimizer
def _adam_fn(sizes, shadow, planes, capturable):
    def fn(device):
        from amk.dp import GradReducer
        from amk.optim import FlatAdam

        torch.manual_seed(0)
        net = nn.Sequential(*[m for a, b in zip(sizes, sizes[1:]) for m in (nn.Linear(a, b), nn.Tanh())]).to(device)
        red = GradReducer(net.parameters(), bucket_bytes=32 << 10)
        opt = FlatAdam(red, lr=3e-3, betas=(0.9, 0.96), weight_decay=0.1, decoupled=True, capturable=capturable,
                       bf16_shadow=shadow)
        if planes:
            opt.enable_planes()
        x = seeded((16, sizes[0]), 1).to(device)
        for _ in range(2):
            red.begin(True)
            net(x).pow(2).mean().backward()
            red.finish()
            norm = opt.step(max_norm=0.7)
        res = dict(norm=norm)
        for i, (fp, m, v) in enumerate(zip(opt.flat_p, opt.m, opt.v)):
            res.update({f"p{i}": fp, f"m{i}": m, f"v{i}": v})
        for i, f16 in enumerate(opt.flat_p16):
            res[f"shadow{i}"] = f16
        for i, pl in enumerate(opt.planes):
            if pl is not None:
                res[f"planes{i}"] = pl[0]
        return res
    return fn


for _sizes, _kd in zip([(64, 128, 64), (37, 53, 300, 7), (1, 1), (4, 4)], ("whole", "edge", "smallest", "edge")):
    for _shadow, _planes, _cap in [(False, False, False), (True, False, False), (False, True, False), (True, True, True)]:
        _add("flat_adam", f"{'-'.join(map(str, _sizes))}_shadow{int(_shadow)}_planes{int(_planes)}_cap{int(_cap)}",
             _adam_fn(_sizes, _shadow, _planes, _cap), _kd)


# ---------------------------------------------------------------------------------------------- the test
_PAIR_BOUND = {"attn_dq": _attn_pair_bound, "attn_dq_x6": _attn_pair_bound, "vq_dcodebook": _vq_pair_bound}


# The guard: every launcher of the C ABI is reached by a case, or stands here with its reason.  Admissible reasons: no Python
# code of amk calls the entry point (C ABI only: single launches through it are bounded by the family's own GPU test), or the
# path is off by default and documented as not covered.  tests/sweep_guard.py holds the verdict.
NOT_SWEPT = {
    "amk_adam_flat_step": "C ABI only: no Python code of amk calls it -- FlatAdam.step always calls amk_adam_flat_step_shadow, with a "
                          "null shadow where there is none (amk/optim.py:232)",
    "amk_grouped_gemm_nt_acc": "off by default and documented as not covered: the sums inside the expert GEMM, ops.MOE_SUM_IN_GEMM "
                               "(csrc/moe.hip:563; the note under ATOMIC above)",
    "amk_grouped_gemm_nn_acc": "off by default and documented as not covered: the sums inside the expert GEMM, ops.MOE_SUM_IN_GEMM "
                               "(csrc/moe.hip:563; the note under ATOMIC above)",
}
REACHED, RAN = set(), set()      # launchers called / cases run by test_result_does_not_depend_on_stale_memory in this process


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_result_does_not_depend_on_stale_memory(device, case, monkeypatch):
    from amk import lib, ops

    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    monkeypatch.setattr(ops, "_SAMPLE_CALLS", ops._SAMPLE_CALLS)      # (the seeded sampling cases set it: put back afterwards)
    RAN.add(case.id)
    with _switches(**case.switches), _env(case.env), _library_calls(sweep_guard.launchers(lib.SIGNATURES), reached=REACHED):
        if case.path is not None:      # the forced path is the one that ran
            with _library_calls(case.path["entries"]) as seen:
                nan_run, big_run = run_both_fills(lambda: case.fn(device))
            case.path["check"](seen)
        else:
            nan_run, big_run = run_both_fills(lambda: case.fn(device))
        torch.cuda.synchronize()
        row = ATOMIC[case.atomic] if case.atomic else None
        assert_fill_independent(nan_run, big_run, case.id, tolerant=row["tensors"] if row else (),
                                bound=_PAIR_BOUND.get(case.atomic), allow_nan=case.allow_nan)
        if case.ref is not None:
            case.ref(nan_run, device)
        if row is not None:      # the same case without atomics: bitwise, every tensor
            if row["repro"] == "torch_det":
                old = torch.are_deterministic_algorithms_enabled()
                torch.use_deterministic_algorithms(True)
                try:
                    a, b = run_both_fills(lambda: case.fn(device))
                finally:
                    torch.use_deterministic_algorithms(old)
            else:
                with _switches(**row["repro"]):
                    a, b = run_both_fills(lambda: case.fn(device))
            assert_fill_independent(a, b, case.id + " (reproducible mode)", allow_nan=case.allow_nan)


def test_atomic_rows_name_a_float_atomic_in_the_source():
    """A path may be in ATOMIC only if its kernel source has a float atomic on the line the row gives."""
    import os

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "attention-models_amd")
    for name, row in ATOMIC.items():
        path, line = row["src"].split(":")
        with open(os.path.join(root, path)) as f:
            text = f.read().splitlines()[int(line) - 1]
        assert "atomic_fadd_f32" in text or "atomicAdd(" in text, (name, text)
    used = {c.atomic for c in CASES if c.atomic}
    assert used == set(ATOMIC), "every ATOMIC row is used by a case, and no case names a row that is not there"


def test_every_family_has_its_case_kinds():
    """Every family has a case of whole tiles, a case one past a tile boundary and a case of the smallest legal size."""
    fams = {}
    for c in CASES:
        fams.setdefault(c.family, set()).add(c.kind)
    assert len(fams) >= 48, sorted(fams)
    missing = {f: sorted(set(KINDS) - kinds) for f, kinds in fams.items() if kinds != set(KINDS)}
    assert not missing, missing
    assert len({c.id for c in CASES}) == len(CASES)


def test_every_launcher_is_swept():
    """Last in the file: the launchers the cases above called, against NOT_SWEPT.  A new entry point of amk.lib.SIGNATURES
    without a case fails here and is named.  Skips unless every case ran in this process (a -k selection)."""
    from amk import lib

    if len(RAN) < len(CASES):
        pytest.skip(f"{len(RAN)} of {len(CASES)} cases of the sweep ran in this process: the guard needs all of them")
    problems = sweep_guard.verdict(REACHED, lib.SIGNATURES, NOT_SWEPT)
    assert not problems, "\n".join(problems)
