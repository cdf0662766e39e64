"""amk_attn_decode on the GPU (csrc/attn_decode.hip) against the fp64 reference and per-element bound of
tests/attn_decode_ref.py: append and read mode at every chunk boundary, the fused cache append, masks, poisoned rows
beyond the valid range, reproducibility, and the refusals."""
import ctypes
import functools

import pytest
import torch

import attn_decode_ref as R

pytestmark = pytest.mark.gpu

B, H, CAP = 2, 3, 200
# every instance of launch_chunks (csrc/attn_decode.hip:218-229, D / 32 float4 per lane): 1 .. 8
HEAD_DIMS = [32, 64, 96, 128, 160, 192, 224, 256]
# the ends, the 32-key passes of a workgroup (31 / 32 / 33) and every boundary of the 64-key chunks below the capacity
# (63 / 64 / 65, 127 / 128 / 129, 191 / 192 / 193): n = 64 c is the first position whose new row opens chunk c
APPEND_N = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 199]
READ_N = [1, 7, 77, 200]
POISON = 3e38   # rows beyond the valid range: any read of one shows as inf / nan or a value far outside the bound


@functools.lru_cache(maxsize=None)
def _inputs(D):
    """q (B, H, D), k / v (B, H, CAP + 1, D) on the CPU: rows 0 .. CAP - 1 fill the cache, row n is also the new row."""
    return R.make_inputs(B, H, D, CAP + 1, seed=2000 + D)


@functools.lru_cache(maxsize=None)
def _reference(D, J, mask_key=None):
    q, k, v = _inputs(D)
    mask = _mask(mask_key)
    return R.reference(q, k[:, :, :J], v[:, :, :J], D ** -0.5, None if mask is None else mask[:, :J])[:2]


def _mask(key):
    if key is None:
        return None
    m = torch.ones(B, CAP, dtype=torch.bool)
    m[0, 5::3] = False      # batch 0: partly masked
    m[1] = False            # batch 1: fully masked -> uniform weights over the keys
    return m


def _device_tensors(D, device, batch=slice(None)):
    """q2 (B, 1, h*d), rows (B, CAP + 1, 2*h*d) in the '(kv h d)' layout."""
    q, k, v = (t[batch] for t in _inputs(D))
    b = q.shape[0]
    q2 = q.reshape(b, 1, H * D).to(device)
    rows = torch.cat((k.permute(0, 2, 1, 3).reshape(b, CAP + 1, H * D), v.permute(0, 2, 1, 3).reshape(b, CAP + 1, H * D)), dim=2)
    return q2, rows.to(device)


def _cache(rows, valid):
    cache = rows[:, :CAP].clone()
    cache[:, valid:] = POISON
    return cache


def _n(n, device):
    return torch.tensor([n], dtype=torch.int32, device=device)


def _check(o, D, J, what, mask_key=None):
    ref, bound = _reference(D, J, mask_key)
    got = o.view(B, H, D).cpu()
    assert bool(torch.isfinite(got).all()), what
    n_bad, worst = R.worst_ratio(got, ref, bound)
    print(f"{what}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{what}: {n_bad} elements outside the bound (worst {worst:.2f}x)"


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
        assert torch.equal(cache[:, n], kv_new[:, 0]), n                       # the appended row, bitwise
        before[:, n] = kv_new[:, 0]
        assert torch.equal(cache, before), n                                   # every other row and the poison untouched
        assert int(n_dev.item()) == n                                          # the kernel never writes the length
        if n == 0:
            assert torch.equal(o.view(B, H, D), kv_new[:, 0, H * D:].view(B, H, D))   # one key: v_new exactly


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_read_mode(device, D):
    from amk import ops

    q2, rows = _device_tensors(D, device)
    for n in READ_N:
        cache = _cache(rows, n)
        before = cache.clone()
        o = ops.attention_decode(q2, None, cache, _n(n, device), H, D, D ** -0.5)
        _check(o, D, n, f"read D {D} n {n}")
        assert torch.equal(cache, before), n
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
    # the fully masked batch: the mean of all capacity values, as amk.h's contract has it
    mean = _inputs(D)[2][1, :, :CAP].double().mean(dim=1)
    assert float((o.view(B, H, D)[1].cpu().double() - mean).abs().max()) <= float(_reference(D, CAP, "m")[1][1].max())
    # a partly valid cache under the same mask: keys past n stay unread whatever the mask says
    cache = _cache(rows, 77)
    o = ops.attention_decode(q2, None, cache, _n(77, device), H, D, D ** -0.5, key_mask=mask)
    _check(o, D, 77, f"masked read D {D} n 77", mask_key="m")


def test_reproducible_and_independent_of_the_batch(device):
    from amk import ops

    D, n = 64, 199
    q2, rows = _device_tensors(D, device)
    kv_new = rows[:, n:n + 1].clone()
    outs = [ops.attention_decode(q2, kv_new, _cache(rows, n), _n(n, device), H, D, D ** -0.5) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    for b in range(B):   # batch 2 = batch 1 run twice
        qb, rb = _device_tensors(D, device, batch=slice(b, b + 1))
        ob = ops.attention_decode(qb, rb[:, n:n + 1].clone(), _cache(rb, n), _n(n, device), H, D, D ** -0.5)
        assert torch.equal(ob[0], outs[0][b]), b


def _raw_call(L, q2, kv_new, cache, o, ws, n_dev, D, heads=H):
    hd = heads * D
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    return L.amk_attn_decode(ptr(q2), ptr(kv_new), ptr(kv_new, 4 * hd), ptr(cache), ptr(cache, 4 * hd), ptr(o), ptr(ws),
                             ptr(n_dev), ctypes.c_void_p(0), q2.shape[0], heads, D, cache.shape[1],
                             hd, D, 2 * hd, D, cache.shape[1] * 2 * hd, 2 * hd, D, hd, D, D ** -0.5,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_out_of_range_and_refusals(device):
    from amk import lib

    L = lib.load()
    D = 64
    q2, rows = _device_tensors(D, device)
    cache = _cache(rows, 150)
    before = cache.clone()
    kv_new = rows[:, 150:151].clone()
    o = torch.full((B, 1, H * D), 7.0, device=device)
    ws = torch.empty(L.amk_attn_decode_ws_floats(B, H, D, CAP), device=device)
    for n in (CAP, CAP + 5, -1):   # append mode with no room (or a corrupt length): nothing is touched
        assert _raw_call(L, q2, kv_new, cache, o, ws, _n(n, device), D) == 0
        torch.cuda.synchronize()
        assert torch.equal(cache, before) and bool((o == 7.0).all()), n
    for n in (0, CAP + 1):         # read mode: no keys, or more than the cache holds
        assert _raw_call(L, q2, None, cache, o, ws, _n(n, device), D) == 0
        torch.cuda.synchronize()
        assert torch.equal(cache, before) and bool((o == 7.0).all()), n
    # an unsupported head dim (4 heads of 48 span the same 192 columns) is refused before any device work
    assert _raw_call(L, q2, kv_new, cache, o, ws, _n(1, device), 48, heads=4) == -2
    assert b"head dim 48" in L.amk_last_error()
    assert _raw_call(L, q2, kv_new, cache, None, ws, _n(1, device), D) == -1
    assert _raw_call(L, q2, kv_new, cache, o, None, _n(1, device), D) == -1
    assert _raw_call(L, q2, kv_new, cache, o, ws, None, D) == -1          # append mode needs n_dev
    assert torch.equal(cache, before) and bool((o == 7.0).all())

