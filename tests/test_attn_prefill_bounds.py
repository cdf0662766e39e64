"""The many-row decode attention (csrc/attn_prefill.hip) on the CPU: the ABI's refusals before any device work, the
workspace size against a restatement, the per-row emulations of tests/attn_decode_ref.py and attn_decode_bf16_ref.py
inside their bounds at the rows the GPU tests use, and planted defects of the launch as a whole -- a key too many, a key
too few, a new row read from the stale cache, an append one row off -- each of which must leave a row's bound or fail
the bitwise cache check (tests/attn_prefill_ref.py)."""
import ctypes
import functools

import pytest
import torch

import attn_decode_bf16_ref as R16
import attn_decode_ref as R
import attn_prefill_ref as P
from amk import lib as amk_lib

AMK_EINVAL, AMK_EUNSUPPORTED = -1, -2
B, H, CAP = 2, 2, 200
# (p0, n) of tests/test_attn_prefill_gpu.py
CASES = [(0, 1), (0, 33), (0, 65), (1, 31), (63, 2), (64, 64), (65, 65), (130, 70), (199, 1), (6, 64), (70, 64)]
ENTRIES = ["amk_attn_prefill", "amk_attn_prefill_bf16"]


def _dummy():
    """(buffer, a non-null host pointer on a 16-byte boundary, the same 4 bytes further): they pass the null checks;
    the second fails the alignment check, which comes after every size and head-dim check and before any HIP call."""
    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    return buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 4)


def _call(L, entry, ptrs, D, n=4, heads=2, cap=16):
    hd = heads * D
    null = ctypes.c_void_p(0)
    strides = [n * hd, hd, D, n * 2 * hd, 2 * hd, D, cap * 2 * hd, 2 * hd, D, n * hd, hd, D]
    return getattr(L, entry)(*ptrs, null, 1, heads, D, cap, n, *strides, 1.0, null)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_come_before_any_device_work(entry):
    L = amk_lib.load()
    buf, ok, off = _dummy()
    name = entry.encode()
    for d in (48, 288):
        assert _call(L, entry, [off] * 8, d) == AMK_EUNSUPPORTED
        msg = L.amk_last_error()
        assert msg.startswith(name + b":") and str(d).encode() in msg and b"multiple of 32" in msg, msg
    assert _call(L, entry, [off] * 8, 64, n=0) == AMK_EINVAL
    assert L.amk_last_error().startswith(name + b": bad sizes"), L.amk_last_error()
    assert _call(L, entry, [off] * 8, 64, n=-3) == AMK_EINVAL
    null = ctypes.c_void_p(0)
    for missing in (0, 3, 4, 5, 6):          # q, k_cache, v_cache, o, ws
        ptrs = [ok] * 8
        ptrs[missing] = null
        assert _call(L, entry, ptrs, 64) == AMK_EINVAL, missing
        assert L.amk_last_error().startswith(name + b": null pointer"), L.amk_last_error()
    ptrs = [ok] * 8
    ptrs[2] = null                              # k_new without v_new
    assert _call(L, entry, ptrs, 64) == AMK_EINVAL and b"go together" in L.amk_last_error()
    ptrs = [ok] * 8
    ptrs[7] = null                              # append mode without n_dev
    assert _call(L, entry, ptrs, 64) == AMK_EINVAL and b"n_dev" in L.amk_last_error()
    for d in (32, 64, 96, 128, 160, 192, 224, 256):   # every taken head dim reaches the alignment check
        for bad in range(7):
            ptrs = [ok] * 8
            ptrs[bad] = off
            assert _call(L, entry, ptrs, d) == AMK_EINVAL, (d, bad)
            msg = L.amk_last_error()
            assert msg.startswith(name + b":") and b"aligned" in msg, msg
    assert _call(L, entry, [ok] * 8, 64, heads=70000) == AMK_EUNSUPPORTED and b"beyond the grid" in L.amk_last_error()
    assert L.amk_version() == 140


def test_workspace_size_matches_its_restatement():
    L = amk_lib.load()

    def floats(b, h, d, cap, n):
        if min(b, h, d, cap, n) <= 0:
            return 0
        slots = b * h * n * ((cap + 63) // 64)          # (M, l) and o[D] per (batch, head, row, chunk of 64 keys)
        return (2 * slots + 3) // 4 * 4 + slots * d

    for args in [(2, 2, 64, 200, 65), (1, 1, 32, 1, 1), (8, 8, 64, 1024, 1023), (3, 5, 96, 65, 7), (2, 3, 256, 64, 64),
                 (8, 8, 64, 1024, 0), (0, 8, 64, 1024, 4), (64, 16, 256, 8192, 8192)]:
        assert L.amk_attn_prefill_ws_floats(*args) == floats(*args), args


@functools.lru_cache(maxsize=None)
def _inputs(D, bf16):
    return P.make_inputs(B, H, D, CAP, seed=3000 + D, bf16=bf16)


def _rows_to_emulate():
    """Absolute positions t = p0 + i of the GPU cases: each case's first and last row and every row that closes or
    opens a chunk of 64 keys or a pass of 32."""
    edges = {31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193}
    ts = set()
    for p0, n in CASES:
        ts |= {p0, p0 + n - 1} | {t for t in edges if p0 <= t < p0 + n}
    return sorted(ts)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [32, 64, 96, 128, 256])
def test_row_emulations_are_inside_the_existing_bounds(D, bf16):
    q, k, v = _inputs(D, bf16)
    rows = _rows_to_emulate()
    assert max(rows) == CAP - 1 and min(rows) == 0
    for t in rows:
        ref = P.row_reference(q, k, v, t, bf16=bf16)
        n_bad = P.outside(P.row_emulation(q, k, v, t, bf16=bf16), ref, bf16)
        assert n_bad == 0, (D, t, n_bad)


def test_masked_read_rows_are_inside_the_existing_bound():
    q, k, v = _inputs(64, False)
    mask = torch.ones(B, CAP, dtype=torch.bool)
    mask[0, 5::3] = False
    mask[1] = False
    for t, J in [(0, 200), (32, 200), (5, 77)]:
        ref = P.row_reference(q, k, v, t, J=J, mask=mask)
        assert P.outside(P.row_emulation(q, k, v, t, J=J, mask=mask), ref) == 0, (t, J)


def _planted(D, p0, n, bf16, defect):
    """(rows with an element outside their bound, rows, cache bitwise as the contract has it) of the model with a defect."""
    q, k, v = _inputs(D, bf16)
    g = torch.Generator().manual_seed(77)
    stale_k, stale_v = torch.randn(B, H, CAP, D, generator=g), torch.randn(B, H, CAP, D, generator=g)
    k_cache = torch.cat((k[:, :, :p0], stale_k[:, :, p0:]), dim=2)     # rows from p0 on: what an earlier decode left
    v_cache = torch.cat((v[:, :, :p0], stale_v[:, :, p0:]), dim=2)
    sl = slice(p0, p0 + n)

    def attend(qr, kk, vv):    # the exact row (bf16: stored as the kernel stores it): a defect must show on its own
        o = R.reference(qr, kk, vv, D ** -0.5)[0]
        return R16.bf16_rne(o) if bf16 else o

    o, kc, vc = P.model(q[:, :, sl], k[:, :, sl], v[:, :, sl], k_cache, v_cache, p0, attend, defect)
    want_k, want_v = k_cache.clone(), v_cache.clone()
    want_k[:, :, sl], want_v[:, :, sl] = k[:, :, sl], v[:, :, sl]
    cache_ok = torch.equal(kc, want_k) and torch.equal(vc, want_v)
    bad = [i for i in range(n) if P.outside(o[:, :, i], P.row_reference(q, k, v, p0 + i, bf16=bf16), bf16)]
    return bad, cache_ok


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D,p0,n", [(32, 0, 33), (64, 63, 2), (64, 65, 65), (96, 1, 31), (128, 130, 70), (256, 64, 64)])
def test_planted_defects_leave_the_bound_or_fail_the_cache_check(D, p0, n, bf16):
    bad, cache_ok = _planted(D, p0, n, bf16, None)
    assert bad == [] and cache_ok                       # the model without a defect is the contract
    # one key too many: every row sees the next row's key (the last row: a stale cache row, or nothing at the capacity)
    bad, cache_ok = _planted(D, p0, n, bf16, "extra_key")
    assert bad == [i for i in range(n) if p0 + i + 1 < CAP] and cache_ok, ("extra_key", bad)
    # one key too few: every row that has more than one key loses its own
    bad, cache_ok = _planted(D, p0, n, bf16, "missing_key")
    assert bad == [i for i in range(n) if p0 + i > 0] and cache_ok, ("missing_key", bad)
    # the new rows read from the stale cache: every row (each attends at least its own new row)
    bad, cache_ok = _planted(D, p0, n, bf16, "stale_new_row")
    assert bad == list(range(n)) and cache_ok, ("stale_new_row", bad)
    # the append one row off: the outputs are right (new keys never come from the cache) and the cache check fails
    bad, cache_ok = _planted(D, p0, n, bf16, "append_off_by_one")
    assert bad == [] and not cache_ok, "append_off_by_one"


def test_out_of_range_is_a_no_op_in_the_model():
    q, k, v = _inputs(32, False)
    o, kc, vc = P.model(q[:, :, :65], k[:, :, :65], v[:, :, :65], k, v, 136, None)   # p0 + n = 201
    assert o is None and torch.equal(kc, k) and torch.equal(vc, v)
