"""amk_attn_prefill on the GPU (csrc/attn_prefill.hip) against the per-row fp64 reference and bound of
tests/attn_decode_ref.py (tests/attn_prefill_ref.py: row i of a call at p0 is the single-token row at J = p0 + i + 1):
append mode across the chunk and row-block boundaries, the bitwise cache append, read mode with a key mask, poisoned
rows beyond the valid range, reproducibility, independence of the batch and of the split into calls, slices of one
projection output, out-of-range positions and the op's refusals."""
import ctypes
import functools

import pytest
import torch

import attn_prefill_ref as P

pytestmark = pytest.mark.gpu

B, H, CAP = 2, 2, 200
# every instance of the prefill kernel (csrc/attn_prefill.hip:293-305, launch_chunks over D / 32): 1 .. 8
HEAD_DIMS = [32, 64, 96, 128, 160, 192, 224, 256]
# (p0, n): one row; one and two passes of 32 keys; rows and positions on either side of the 64-key chunks and the
# 16-row blocks; a call that ends at the capacity; and two calls, (6, 64) and (70, 64), in which a group of rows that is
# NOT the last of its 16-row block has rows that stop short of a 64-key chunk beside rows that cross it, so that some
# waves of a workgroup skip the chunk's sums while others leave a partial for the second launch and the block goes on
CASES = [(0, 1), (0, 33), (0, 65), (1, 31), (63, 2), (64, 64), (65, 65), (130, 70), (199, 1), (6, 64), (70, 64)]
POISON = 3e38   # rows beyond the valid range: any read of one shows as inf / nan or a value far outside the bound


@functools.lru_cache(maxsize=None)
def _inputs(D):
    return P.make_inputs(B, H, D, CAP, seed=4000 + D)


@functools.lru_cache(maxsize=None)
def _reference(D, t, J=None, masked=False):
    q, k, v = _inputs(D)
    return P.row_reference(q, k, v, t, J=J, mask=_mask() if masked else None)


def _mask():
    m = torch.ones(B, CAP, dtype=torch.bool)
    m[0, 5::3] = False      # batch 0: partly masked
    m[1] = False            # batch 1: fully masked -> uniform weights over the keys
    return m


@functools.lru_cache(maxsize=None)
def _device_tensors(D, device):
    """q2 (B, CAP, h*d) and rows (B, CAP, 2*h*d) in the '(kv h d)' layout, by absolute position.  Read only."""
    q, k, v = _inputs(D)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B, CAP, H * D)  # noqa: E731
    return flat(q).to(device), torch.cat((flat(k), flat(v)), dim=2).to(device)


def _cache(rows, valid):
    cache = rows.clone()
    cache[:, valid:] = POISON
    return cache


def _n(n, device):
    return torch.tensor([n], dtype=torch.int32, device=device)


def _check_rows(o, D, p0, what, J=None, masked=False):
    """Every element of every row inside the bound of its own reference."""
    n = o.shape[1]
    got = o.view(B, n, H, D).permute(0, 2, 1, 3).cpu()
    assert bool(torch.isfinite(got).all()), what
    worst = 0.0
    for i in range(n):
        ref, bound = _reference(D, p0 + i, J, masked)
        err = (got[:, :, i].double() - ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert int((err > bound).sum()) == 0, f"{what}: row {i} outside the bound (worst {float((err / bound).max()):.2f}x)"
    print(f"{what}: worst |err| / bound {worst:.3f}")


def _equal_to_decode(ops, q2, o, cache, p0, D):
    """Rows of o that are bitwise what amk_attn_decode gives for the same query on the same cache.  Reported only."""
    same = 0
    for i in range(o.shape[1]):
        od = ops.attention_decode(q2[:, p0 + i:p0 + i + 1].contiguous(), None, cache, _n(p0 + i + 1, o.device), H, D, D ** -0.5)
        same += int(torch.equal(od[:, 0], o[:, i]))
    return same


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_append_mode(device, D):
    from amk import ops

    q2, rows = _device_tensors(D, device)
    for p0, n in CASES:
        cache = _cache(rows, p0)                    # rows p0 .. are poisoned: the new rows must come from kv_new
        want = cache.clone()
        kv_new = rows[:, p0:p0 + n].clone()
        n_dev = _n(p0, device)
        o = ops.attention_prefill(q2[:, p0:p0 + n], kv_new, cache, n_dev, H, D, D ** -0.5)
        assert tuple(o.shape) == (B, n, H * D) and o.dtype == torch.float32
        _check_rows(o, D, p0, f"append D {D} p0 {p0} n {n}")
        assert torch.equal(cache[:, p0:p0 + n], kv_new), (p0, n)               # the appended rows, bitwise
        want[:, p0:p0 + n] = kv_new
        assert torch.equal(cache, want), (p0, n)                               # every other row and the poison untouched
        assert int(n_dev.item()) == p0                                         # the kernel never writes the position
        if p0 == 0:
            assert torch.equal(o[:, 0], kv_new[:, 0, H * D:])                  # one key: v_new exactly
        same = _equal_to_decode(ops, q2, o, cache, p0, D)
        print(f"append D {D} p0 {p0} n {n}: {same} of {n} rows bitwise equal to amk_attn_decode on the same cache")


@pytest.mark.parametrize("D", [64, 96])
@pytest.mark.parametrize("n", [1, 33])
def test_read_mode_with_key_mask(device, D, n):
    from amk import ops

    q2, rows = _device_tensors(D, device)
    mask = _mask().to(device)
    cache = _cache(rows, CAP)
    before = cache.clone()
    o = ops.attention_prefill(q2[:, :n], None, cache, None, H, D, D ** -0.5, key_mask=mask)   # n_dev NULL: all rows
    _check_rows(o, D, 0, f"masked read D {D} n {n}", J=CAP, masked=True)
    # the fully masked batch: the mean of all capacity values, as amk.h's contract has it
    mean = _inputs(D)[2][1].double().mean(dim=1)
    for i in range(n):
        err = (o.view(B, n, H, D)[1, i].cpu().double() - mean).abs()
        assert float(err.max()) <= float(_reference(D, i, CAP, True)[1][1].max()), i
    o = ops.attention_prefill(q2[:, :n], None, cache, None, H, D, D ** -0.5)                    # and without the mask
    _check_rows(o, D, 0, f"read D {D} n {n}", J=CAP)
    # a partly valid cache under the same mask: keys past p0 stay unread whatever the mask says
    cache77 = _cache(rows, 77)
    o = ops.attention_prefill(q2[:, :n], None, cache77, _n(77, device), H, D, D ** -0.5, key_mask=mask)
    _check_rows(o, D, 0, f"masked read D {D} n {n} p0 77", J=77, masked=True)
    assert torch.equal(cache, before) and torch.equal(cache77, _cache(rows, 77))                # read mode writes no cache


@pytest.mark.parametrize("D", [64, 96])
def test_reproducible_and_independent_of_batch_and_split(device, D):
    from amk import ops

    p0, n = 65, 65
    q2, rows = _device_tensors(D, device)
    run = lambda q, r, a, m: ops.attention_prefill(q[:, a:a + m], r[:, a:a + m].clone(), _cache(r, a), _n(a, device),  # noqa: E731
                                                   H, D, D ** -0.5)
    outs = [run(q2, rows, p0, n) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    for b in range(B):                                   # a batch alone = that batch of two
        ob = run(q2[b:b + 1], rows[b:b + 1], p0, n)
        assert torch.equal(ob[0], outs[0][b]), b
    # the same rows in two calls, split inside a 16-row block and inside a chunk: a row does not depend on its block
    cache = _cache(rows, p0)
    n_dev = _n(p0, device)
    first = ops.attention_prefill(q2[:, p0:p0 + 23], rows[:, p0:p0 + 23].clone(), cache, n_dev, H, D, D ** -0.5)
    n_dev.add_(23)
    second = ops.attention_prefill(q2[:, p0 + 23:p0 + n], rows[:, p0 + 23:p0 + n].clone(), cache, n_dev, H, D, D ** -0.5)
    assert torch.equal(torch.cat((first, second), dim=1), outs[0])
    assert torch.equal(cache[:, :p0 + n], rows[:, :p0 + n])


@pytest.mark.parametrize("D", [64, 96])
def test_slices_of_one_projection_output_equal_the_contiguous_call(device, D):
    from amk import ops

    p0, n, hd = 130, 70, H * D
    q2, rows = _device_tensors(D, device)
    kv_new = rows[:, p0:p0 + n].clone()
    qkv = torch.cat((q2[:, p0:p0 + n], kv_new), dim=2)          # (B, n, 3hd): q | k | v as one projection leaves them
    cache_a, cache_b = _cache(rows, p0), _cache(rows, p0)
    o_a = ops.attention_prefill(q2[:, p0:p0 + n].contiguous(), kv_new, cache_a, _n(p0, device), H, D, D ** -0.5)
    q_s, kv_s = qkv[:, :, :hd], qkv[:, :, hd:]
    assert not q_s.is_contiguous() and not kv_s.is_contiguous()
    o_b = ops.attention_prefill(q_s, kv_s, cache_b, _n(p0, device), H, D, D ** -0.5)
    assert torch.equal(o_a, o_b) and torch.equal(cache_a, cache_b)


def _raw_call(L, q2, kv_new, cache, o, ws, n_dev, D, heads=H):
    hd, n, cap = heads * D, q2.shape[1], cache.shape[1]
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    return L.amk_attn_prefill(ptr(q2), ptr(kv_new), ptr(kv_new, 4 * hd), ptr(cache), ptr(cache, 4 * hd), ptr(o), ptr(ws),
                              ptr(n_dev), ctypes.c_void_p(0), q2.shape[0], heads, D, cap, n,
                              n * hd, hd, D, n * 2 * hd, 2 * hd, D, cap * 2 * hd, 2 * hd, D, n * hd, hd, D, D ** -0.5,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_out_of_range_and_refusals(device):
    from amk import lib, ops

    L = lib.load()
    D, n = 64, 65
    q2, rows = _device_tensors(D, device)
    q = q2[:, :n].contiguous()
    kv_new = rows[:, :n].clone()
    cache = _cache(rows, 136)
    before = cache.clone()
    o = torch.full((B, n, H * D), 7.0, device=device)
    ws = torch.empty(L.amk_attn_prefill_ws_floats(B, H, D, CAP, n), device=device)
    for p0 in (136, CAP, CAP + 5, -1):   # p0 + n = 201 and beyond, or a corrupt position: nothing is touched
        assert _raw_call(L, q, kv_new, cache, o, ws, _n(p0, device), D) == 0
        torch.cuda.synchronize()
        assert torch.equal(cache, before) and bool((o == 7.0).all()), p0
    for p0 in (0, CAP + 1):               # read mode: no keys, or more than the cache holds
        assert _raw_call(L, q, None, cache, o, ws, _n(p0, device), D) == 0
        torch.cuda.synchronize()
        assert torch.equal(cache, before) and bool((o == 7.0).all()), p0
    assert _raw_call(L, q, kv_new, cache, o, ws, _n(1, device), 16, heads=8) == -2   # refused before any device work
    assert b"amk_attn_prefill: head dim 16" in L.amk_last_error()
    assert _raw_call(L, q, kv_new, cache, None, ws, _n(1, device), D) == -1
    assert _raw_call(L, q, kv_new, cache, o, None, _n(1, device), D) == -1
    assert _raw_call(L, q, kv_new, cache, o, ws, None, D) == -1                      # append mode needs n_dev
    assert torch.equal(cache, before) and bool((o == 7.0).all())
    # the op's own refusals
    with pytest.raises(RuntimeError, match="inference only"):
        ops.attention_prefill(q.clone().requires_grad_(), kv_new, cache, _n(1, device), H, D, D ** -0.5)
    with pytest.raises(RuntimeError, match="must have the cache's dtype"):
        ops.attention_prefill(q.bfloat16(), kv_new, cache, _n(1, device), H, D, D ** -0.5)
    with pytest.raises(RuntimeError, match="append mode needs n_dev"):
        ops.attention_prefill(q, kv_new, cache, None, H, D, D ** -0.5)
    with pytest.raises(RuntimeError, match="ws must be"):
        ops.attention_prefill(q, kv_new, cache, _n(1, device), H, D, D ** -0.5, ws=ws[:8])
    with pytest.raises(RuntimeError, match="head dim 16"):
        ops.attention_prefill(q, kv_new, cache, _n(1, device), 8, 16, 16 ** -0.5)
    assert torch.equal(cache, before)
