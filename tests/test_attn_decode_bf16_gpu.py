"""amk_attn_decode_bf16 on the GPU (csrc/attn_decode.hip) against the fp64 reference and the RNE interval of
tests/attn_decode_bf16_ref.py: append and read mode at every chunk boundary, the fused bitwise cache append, masks,
poisoned rows beyond the valid range, reproducibility, q / kv_new as slices of one projection output, and the refusals."""
import ctypes
import functools

import pytest
import torch

import attn_decode_bf16_ref as R16

pytestmark = pytest.mark.gpu

B, H, CAP = 2, 3, 200
# every instance of the bf16 chunk kernel (csrc/attn_decode.hip:421-432, launch_chunks_bf16 over D / 32): 1 .. 8
HEAD_DIMS = [32, 64, 96, 128, 160, 192, 224, 256]
APPEND_N = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 199]
READ_N = [1, 7, 77, 200]
BF16 = torch.bfloat16
POISON = float(torch.tensor(3e38).to(BF16))   # the bf16 value nearest 3e38


@functools.lru_cache(maxsize=None)
def _inputs(D):
    """q (B, H, D), k / v (B, H, CAP + 1, D), bf16 values as f32 on the CPU: rows 0 .. CAP - 1 fill the cache, row n is
    also the new row."""
    return R16.make_inputs(B, H, D, CAP + 1, seed=2000 + D)


def _mask(key):
    if key is None:
        return None
    m = torch.ones(B, CAP, dtype=torch.bool)
    m[0, 5::3] = False
    m[1] = False
    return m


@functools.lru_cache(maxsize=None)
def _reference(D, J, mask_key=None):
    q, k, v = _inputs(D)
    mask = _mask(mask_key)
    return R16.reference(q, k[:, :, :J], v[:, :, :J], D ** -0.5, None if mask is None else mask[:, :J])[:4]


def _device_tensors(D, device, batch=slice(None)):
    """q2 (B, 1, h*d), rows (B, CAP + 1, 2*h*d) in the '(kv h d)' layout, bf16."""
    q, k, v = (t[batch] for t in _inputs(D))
    b = q.shape[0]
    q2 = q.reshape(b, 1, H * D)
    rows = torch.cat((k.permute(0, 2, 1, 3).reshape(b, CAP + 1, H * D), v.permute(0, 2, 1, 3).reshape(b, CAP + 1, H * D)), dim=2)
    return q2.to(device, BF16), rows.to(device, BF16)


def _cache(rows, valid):
    cache = rows[:, :CAP].clone()
    cache[:, valid:] = POISON
    return cache


def _n(n, device):
    return torch.tensor([n], dtype=torch.int32, device=device)


def _bits(t):
    return t.view(torch.int16)


def _check(o, D, J, what, mask_key=None):
    ref, b32, lo, hi = _reference(D, J, mask_key)
    assert o.dtype == BF16
    got = o.view(B, H, D).float().cpu()
    assert bool(torch.isfinite(got).all()), what
    n_bad = R16.count_outside(got, lo, hi)
    off = int((got.double() != R16.bf16_rne(ref)).sum())
    print(f"{what}: {n_bad} outside, {off} of {got.numel()} differ from RNE(ref)")
    assert n_bad == 0, f"{what}: {n_bad} elements outside [RNE(ref - b32), RNE(ref + b32)]"


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_append_mode(device, D):
    from amk import ops

    q2, rows = _device_tensors(D, device)
    for n in APPEND_N:
        cache = _cache(rows, n)                     # row n itself is poisoned: it must come from kv_new
        before = cache.clone()
        kv_new = rows[:, n:n + 1].clone()
        n_dev = _n(n, device)
        o = ops.attention_decode(q2, kv_new, cache, n_dev, H, D, D ** -0.5)
        _check(o, D, n + 1, f"append D {D} n {n}")
        assert torch.equal(_bits(cache[:, n]), _bits(kv_new[:, 0])), n         # the appended row, bitwise
        before[:, n] = kv_new[:, 0]
        assert torch.equal(_bits(cache), _bits(before)), n                     # every other row and the poison untouched
        assert int(n_dev.item()) == n
        if n == 0:
            assert torch.equal(_bits(o.view(B, H * D)), _bits(kv_new[:, 0, H * D:]))   # one key: v_new's bits


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_read_mode(device, D):
    from amk import ops

    q2, rows = _device_tensors(D, device)
    for n in READ_N:
        cache = _cache(rows, n)
        before = cache.clone()
        o = ops.attention_decode(q2, None, cache, _n(n, device), H, D, D ** -0.5)
        _check(o, D, n, f"read D {D} n {n}")
        assert torch.equal(_bits(cache), _bits(before)), n
    cache = _cache(rows, CAP)
    o = ops.attention_decode(q2, None, cache, None, H, D, D ** -0.5)            # n_dev NULL: all capacity rows
    _check(o, D, CAP, f"read D {D} n_dev NULL")


@pytest.mark.parametrize("D", [64, 96])
def test_read_mode_with_key_mask(device, D):
    from amk import ops

    q2, rows = _device_tensors(D, device)
    mask = _mask("m").to(device)
    cache = _cache(rows, CAP)
    o = ops.attention_decode(q2, None, cache, None, H, D, D ** -0.5, key_mask=mask)
    _check(o, D, CAP, f"masked read D {D}", mask_key="m")
    # the fully masked batch: the mean of all capacity values, as amk.h's contract has it, held to the same interval
    mean = _inputs(D)[2][1, :, :CAP].double().mean(dim=1)
    b32 = _reference(D, CAP, "m")[1][1]
    got = o.view(B, H, D)[1].float().cpu()
    assert R16.count_outside(got, R16.bf16_rne(mean - b32), R16.bf16_rne(mean + b32)) == 0
    # a partly valid cache under the same mask: keys past n stay unread whatever the mask says
    cache = _cache(rows, 77)
    o = ops.attention_decode(q2, None, cache, _n(77, device), H, D, D ** -0.5, key_mask=mask)
    _check(o, D, 77, f"masked read D {D} n 77", mask_key="m")


@pytest.mark.parametrize("D", [64, 96])
def test_reproducible_and_independent_of_the_batch(device, D):
    from amk import ops

    n = 199
    q2, rows = _device_tensors(D, device)
    kv_new = rows[:, n:n + 1].clone()
    outs = [ops.attention_decode(q2, kv_new, _cache(rows, n), _n(n, device), H, D, D ** -0.5) for _ in range(2)]
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    qb, rb = _device_tensors(D, device, batch=slice(0, 1))   # batch 0 alone = batch 0 of two
    ob = ops.attention_decode(qb, rb[:, n:n + 1].clone(), _cache(rb, n), _n(n, device), H, D, D ** -0.5)
    assert torch.equal(_bits(ob[0]), _bits(outs[0][0]))


@pytest.mark.parametrize("D", [64, 96])
def test_slices_of_one_projection_output_equal_the_contiguous_call(device, D):
    from amk import ops

    n, hd = 130, H * D
    q2, rows = _device_tensors(D, device)
    kv_new = rows[:, n:n + 1].clone()
    qkv = torch.cat((q2, kv_new), dim=2)                      # (B, 1, 3hd): q | k | v as one projection leaves them
    cache_a, cache_b = _cache(rows, n), _cache(rows, n)
    o_a = ops.attention_decode(q2, kv_new, cache_a, _n(n, device), H, D, D ** -0.5)
    q_s, kv_s = qkv[:, :, :hd], qkv[:, :, hd:]
    assert not q_s.is_contiguous() and not kv_s.is_contiguous()
    o_b = ops.attention_decode(q_s, kv_s, cache_b, _n(n, device), H, D, D ** -0.5)
    assert torch.equal(_bits(o_a), _bits(o_b))
    assert torch.equal(_bits(cache_a), _bits(cache_b))
    _check(o_b, D, n + 1, f"sliced D {D}")


def _raw_call(L, q2, kv_new, cache, o, ws, n_dev, D, heads=H):
    hd = heads * D
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    return L.amk_attn_decode_bf16(ptr(q2), ptr(kv_new), ptr(kv_new, 2 * hd), ptr(cache), ptr(cache, 2 * hd), ptr(o), ptr(ws),
                                  ptr(n_dev), ctypes.c_void_p(0), q2.shape[0], heads, D, cache.shape[1],
                                  hd, D, 2 * hd, D, cache.shape[1] * 2 * hd, 2 * hd, D, hd, D, D ** -0.5,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_out_of_range_and_refusals(device):
    from amk import lib, ops

    L = lib.load()
    D = 64
    q2, rows = _device_tensors(D, device)
    cache = _cache(rows, 150)
    before = cache.clone()
    kv_new = rows[:, 150:151].clone()
    o = torch.full((B, 1, H * D), 7.0, device=device, dtype=BF16)
    ws = torch.empty(L.amk_attn_decode_ws_floats(B, H, D, CAP), device=device)
    for n in (CAP, CAP + 5, -1):   # append mode with no room (or a corrupt length): nothing is touched
        assert _raw_call(L, q2, kv_new, cache, o, ws, _n(n, device), D) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(cache), _bits(before)) and bool((o == 7.0).all()), n
    for n in (0, CAP + 1):         # read mode: no keys, or more than the cache holds
        assert _raw_call(L, q2, None, cache, o, ws, _n(n, device), D) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(cache), _bits(before)) and bool((o == 7.0).all()), n
    # head dim 48 (4 heads of 48 span the same 192 columns) is refused before any device work
    assert _raw_call(L, q2, kv_new, cache, o, ws, _n(1, device), 48, heads=4) == -2
    assert b"head dim 48" in L.amk_last_error()
    assert _raw_call(L, q2, kv_new, cache, None, ws, _n(1, device), D) == -1
    assert _raw_call(L, q2, kv_new, cache, o, ws, None, D) == -1          # append mode needs n_dev
    assert torch.equal(_bits(cache), _bits(before)) and bool((o == 7.0).all())
    # the op: a dtype mix and f16 are refused, and say so
    with pytest.raises(RuntimeError, match="must have the cache's dtype"):
        ops.attention_decode(q2.float(), kv_new, cache, _n(1, device), H, D, D ** -0.5)
    with pytest.raises(RuntimeError, match="must have the cache's dtype"):
        ops.attention_decode(q2, kv_new, cache.float(), _n(1, device), H, D, D ** -0.5)
    with pytest.raises(RuntimeError, match="float32 or a bfloat16 cache"):
        ops.attention_decode(q2.half(), kv_new.half(), cache.half(), _n(1, device), H, D, D ** -0.5)
    with pytest.raises(RuntimeError, match="head dim 48"):
        ops.attention_decode(q2, kv_new, cache, _n(1, device), 4, 48, 48 ** -0.5)
