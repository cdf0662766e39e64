"""amk_attn_prefill_bf16 on the GPU (csrc/attn_prefill.hip) against the per-row fp64 reference and the RNE interval of
tests/attn_decode_bf16_ref.py (tests/attn_prefill_ref.py: row i of a call at p0 is the single-token row at
J = p0 + i + 1): the cases of tests/test_attn_prefill_gpu.py on a bf16 cache, every comparison of stored values bitwise."""
import ctypes
import functools

import pytest
import torch

import attn_decode_bf16_ref as R16
import attn_prefill_ref as P

pytestmark = pytest.mark.gpu

B, H, CAP = 2, 2, 200
# every instance of the prefill kernel (csrc/attn_prefill.hip:293-305, launch_chunks over D / 32): 1 .. 8
HEAD_DIMS = [32, 64, 96, 128, 160, 192, 224, 256]
# the cases of tests/test_attn_prefill_gpu.py (see there for the last two)
CASES = [(0, 1), (0, 33), (0, 65), (1, 31), (63, 2), (64, 64), (65, 65), (130, 70), (199, 1), (6, 64), (70, 64)]
BF16 = torch.bfloat16
POISON = float(torch.tensor(3e38).to(BF16))   # the bf16 value nearest 3e38


@functools.lru_cache(maxsize=None)
def _inputs(D):
    return P.make_inputs(B, H, D, CAP, seed=5000 + D, bf16=True)


@functools.lru_cache(maxsize=None)
def _reference(D, t, J=None, masked=False):
    q, k, v = _inputs(D)
    return P.row_reference(q, k, v, t, J=J, mask=_mask() if masked else None, bf16=True)


def _mask():
    m = torch.ones(B, CAP, dtype=torch.bool)
    m[0, 5::3] = False
    m[1] = False
    return m


@functools.lru_cache(maxsize=None)
def _device_tensors(D, device):
    """q2 (B, CAP, h*d) and rows (B, CAP, 2*h*d) in the '(kv h d)' layout, bf16, by absolute position.  Read only."""
    q, k, v = _inputs(D)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B, CAP, H * D)  # noqa: E731
    return flat(q).to(device, BF16), torch.cat((flat(k), flat(v)), dim=2).to(device, BF16)


def _cache(rows, valid):
    cache = rows.clone()
    cache[:, valid:] = POISON
    return cache


def _n(n, device):
    return torch.tensor([n], dtype=torch.int32, device=device)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_rows(o, D, p0, what, J=None, masked=False):
    """Every element of every row inside [RNE(ref - b32), RNE(ref + b32)] of its own reference."""
    assert o.dtype == BF16
    n = o.shape[1]
    got = o.view(B, n, H, D).permute(0, 2, 1, 3).float().cpu()
    assert bool(torch.isfinite(got).all()), what
    off = 0
    for i in range(n):
        ref, b32, lo, hi = _reference(D, p0 + i, J, masked)
        n_bad = R16.count_outside(got[:, :, i], lo, hi)
        off += int((got[:, :, i].double() != R16.bf16_rne(ref)).sum())
        assert n_bad == 0, f"{what}: row {i}: {n_bad} elements outside [RNE(ref - b32), RNE(ref + b32)]"
    print(f"{what}: 0 outside, {off} of {got.numel()} differ from RNE(ref)")


def _equal_to_decode(ops, q2, o, cache, p0, D):
    """Rows of o that are bitwise what amk_attn_decode_bf16 gives for the same query on the same cache.  Reported only."""
    same = 0
    for i in range(o.shape[1]):
        od = ops.attention_decode(q2[:, p0 + i:p0 + i + 1].contiguous(), None, cache, _n(p0 + i + 1, o.device), H, D, D ** -0.5)
        same += int(torch.equal(_bits(od[:, 0]), _bits(o[:, i])))
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
        assert tuple(o.shape) == (B, n, H * D)
        _check_rows(o, D, p0, f"append D {D} p0 {p0} n {n}")
        assert torch.equal(_bits(cache[:, p0:p0 + n]), _bits(kv_new)), (p0, n)    # the appended rows, bitwise
        want[:, p0:p0 + n] = kv_new
        assert torch.equal(_bits(cache), _bits(want)), (p0, n)                    # every other row and the poison untouched
        assert int(n_dev.item()) == p0
        if p0 == 0:
            assert torch.equal(_bits(o[:, 0]), _bits(kv_new[:, 0, H * D:]))       # one key: v_new's bits
        same = _equal_to_decode(ops, q2, o, cache, p0, D)
        print(f"append D {D} p0 {p0} n {n}: {same} of {n} rows bitwise equal to amk_attn_decode_bf16 on the same cache")


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
    # the fully masked batch: the mean of all capacity values, as amk.h's contract has it, held to the same interval
    mean = _inputs(D)[2][1].double().mean(dim=1)
    for i in range(n):
        b32 = _reference(D, i, CAP, True)[1][1]
        got = o.view(B, n, H, D)[1, i].float().cpu()
        assert R16.count_outside(got, R16.bf16_rne(mean - b32), R16.bf16_rne(mean + b32)) == 0, i
    o = ops.attention_prefill(q2[:, :n], None, cache, None, H, D, D ** -0.5)                    # and without the mask
    _check_rows(o, D, 0, f"read D {D} n {n}", J=CAP)
    cache77 = _cache(rows, 77)   # a partly valid cache under the same mask: keys past p0 stay unread
    o = ops.attention_prefill(q2[:, :n], None, cache77, _n(77, device), H, D, D ** -0.5, key_mask=mask)
    _check_rows(o, D, 0, f"masked read D {D} n {n} p0 77", J=77, masked=True)
    assert torch.equal(_bits(cache), _bits(before)) and torch.equal(_bits(cache77), _bits(_cache(rows, 77)))


@pytest.mark.parametrize("D", [64, 96])
def test_reproducible_and_independent_of_batch_and_split(device, D):
    from amk import ops

    p0, n = 65, 65
    q2, rows = _device_tensors(D, device)
    run = lambda q, r, a, m: ops.attention_prefill(q[:, a:a + m], r[:, a:a + m].clone(), _cache(r, a), _n(a, device),  # noqa: E731
                                                   H, D, D ** -0.5)
    outs = [run(q2, rows, p0, n) for _ in range(2)]
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    for b in range(B):                                   # a batch alone = that batch of two
        ob = run(q2[b:b + 1], rows[b:b + 1], p0, n)
        assert torch.equal(_bits(ob[0]), _bits(outs[0][b])), b
    # the same rows in two calls, split inside a 16-row block and inside a chunk: a row does not depend on its block
    cache = _cache(rows, p0)
    n_dev = _n(p0, device)
    first = ops.attention_prefill(q2[:, p0:p0 + 23], rows[:, p0:p0 + 23].clone(), cache, n_dev, H, D, D ** -0.5)
    n_dev.add_(23)
    second = ops.attention_prefill(q2[:, p0 + 23:p0 + n], rows[:, p0 + 23:p0 + n].clone(), cache, n_dev, H, D, D ** -0.5)
    assert torch.equal(_bits(torch.cat((first, second), dim=1)), _bits(outs[0]))
    assert torch.equal(_bits(cache[:, :p0 + n]), _bits(rows[:, :p0 + n]))


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
    assert torch.equal(_bits(o_a), _bits(o_b)) and torch.equal(_bits(cache_a), _bits(cache_b))


def _raw_call(L, q2, kv_new, cache, o, ws, n_dev, D, heads=H):
    hd, n, cap = heads * D, q2.shape[1], cache.shape[1]
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    return L.amk_attn_prefill_bf16(ptr(q2), ptr(kv_new), ptr(kv_new, 2 * hd), ptr(cache), ptr(cache, 2 * hd), ptr(o), ptr(ws),
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
    o = torch.full((B, n, H * D), 7.0, device=device, dtype=BF16)
    ws = torch.empty(L.amk_attn_prefill_ws_floats(B, H, D, CAP, n), device=device)
    for p0 in (136, CAP, CAP + 5, -1):   # p0 + n = 201 and beyond, or a corrupt position: nothing is touched
        assert _raw_call(L, q, kv_new, cache, o, ws, _n(p0, device), D) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(cache), _bits(before)) and bool((o == 7.0).all()), p0
    for p0 in (0, CAP + 1):               # read mode: no keys, or more than the cache holds
        assert _raw_call(L, q, None, cache, o, ws, _n(p0, device), D) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(cache), _bits(before)) and bool((o == 7.0).all()), p0
    assert _raw_call(L, q, kv_new, cache, o, ws, _n(1, device), 16, heads=8) == -2   # refused before any device work
    assert b"amk_attn_prefill_bf16: head dim 16" in L.amk_last_error()
    assert _raw_call(L, q, kv_new, cache, None, ws, _n(1, device), D) == -1
    assert _raw_call(L, q, kv_new, cache, o, ws, None, D) == -1                      # append mode needs n_dev
    assert torch.equal(_bits(cache), _bits(before)) and bool((o == 7.0).all())
    with pytest.raises(RuntimeError, match="must have the cache's dtype"):
        ops.attention_prefill(q.float(), kv_new, cache, _n(1, device), H, D, D ** -0.5)
    with pytest.raises(RuntimeError, match="float32 or a bfloat16 cache"):
        ops.attention_prefill(q.half(), kv_new.half(), cache.half(), _n(1, device), H, D, D ** -0.5)
    q5 = torch.zeros((B, n, H * D + 4), device=device, dtype=BF16)[:, :, 4:]         # rows at a stride off a multiple of 8
    with pytest.raises(RuntimeError, match="consumes q in place"):
        ops.attention_prefill(q5, kv_new, cache, _n(1, device), H, D, D ** -0.5)
