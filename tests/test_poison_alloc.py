"""tests/poison.py on CPU tensors (devices="all"): every signature variant amk uses, both fills down to the bit patterns,
integer tensors untouched, the allocators restored, and the method itself -- a toy op that sums a buffer it wrote only
partly is caught by the comparison of the two fills, a correct one passes."""
import struct

import pytest
import torch

import poison
from poison import assert_fill_independent, poisoned_empty, run_both_fills

F32_BITS = {"nan": 0xFFFFFFFF - (1 << 32), "big": 0x7F7F7F7F}     # as int32
BF16_BITS = {"nan": 0xFFFF - (1 << 16), "big": 0x7F7F}            # as int16
BIG32 = struct.unpack("<f", b"\x7f\x7f\x7f\x7f")[0]


def _all_bytes(t, byte):
    raw = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())
    return bool((raw == byte).all())


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_signature_variants(fill):
    byte = poison.FILL_BYTE[fill]
    like = torch.zeros(3, 5)
    with poisoned_empty(fill, devices="all"):
        made = [
            torch.empty((4, 6), dtype=torch.float32),                              # size as a tuple
            torch.empty(4, 6, dtype=torch.float32),                                # size as varargs
            torch.empty(7, device="cpu", dtype=torch.bfloat16),                    # dtype= and device=
            torch.empty((2, 3), device=torch.device("cpu"), dtype=torch.float64),
            torch.empty(5),                                                        # an int size, default dtype
            torch.empty((2, 3, 4, 5), dtype=torch.float32, memory_format=torch.channels_last),
            torch.empty((3,), dtype=torch.float32, pin_memory=False),
            torch.empty(size=(2, 2), dtype=torch.float32),
            torch.empty_like(like),
            torch.empty_like(like, dtype=torch.bfloat16),
            torch.empty_like(like.t()),                                            # a non-contiguous prototype
            torch.empty_like(like, memory_format=torch.contiguous_format),
            torch.empty_strided((3, 4), (8, 1), dtype=torch.float32),              # padded rows: the gaps are filled too
            like.new_empty((2, 7)),
            like.new_empty(2, 7),
            like.new_empty((6,), dtype=torch.bfloat16),
            like.new_empty((6,), dtype=torch.float64, device="cpu"),
        ]
    for i, t in enumerate(made):
        assert _all_bytes(t, byte), f"variant {i}: {t.dtype} {tuple(t.shape)} not filled"
    assert made[0].shape == made[1].shape == (4, 6)
    assert made[5].is_contiguous(memory_format=torch.channels_last)
    assert made[10].stride() == like.t().stride()
    assert made[12].stride() == (8, 1)


def test_bit_patterns():
    with poisoned_empty("nan", devices="all"):
        n32, n16, n64 = torch.empty(9), torch.empty(9, dtype=torch.bfloat16), torch.empty(9, dtype=torch.float64)
    with poisoned_empty("big", devices="all"):
        b32, b16, b64 = torch.empty(9), torch.empty(9, dtype=torch.bfloat16), torch.empty(9, dtype=torch.float64)
    assert torch.isnan(n32).all() and torch.isnan(n16).all() and torch.isnan(n64).all()
    assert (n32.view(torch.int32) == F32_BITS["nan"]).all() and (n16.view(torch.int16) == BF16_BITS["nan"]).all()
    assert (b32.view(torch.int32) == F32_BITS["big"]).all() and (b16.view(torch.int16) == BF16_BITS["big"]).all()
    assert (b64.view(torch.int64) == 0x7F7F7F7F7F7F7F7F).all()
    assert torch.isfinite(b32).all() and torch.isfinite(b16).all() and torch.isfinite(b64).all()
    assert float(b32[0]) == BIG32 and 3.38e38 < BIG32 < 3.40e38
    assert 3.38e38 < float(b16[0]) < 3.40e38          # bf16 0x7F7F reads the same
    assert float(b64[0]) > 1e300


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_integer_bool_and_unlisted_uint8_untouched(fill):
    """An allocator that hands back known bytes stands in for torch.empty: the wrapper must leave them alone."""
    real = torch.empty

    def marked(*a, **k):
        return real(*a, **k).zero_()

    torch.empty = marked
    try:
        with poisoned_empty(fill, devices="all"):
            made = [torch.empty(8, dtype=dt) for dt in (torch.int32, torch.int64, torch.int16, torch.int8, torch.bool,
                                                        torch.uint8)]
            f = torch.empty(8, dtype=torch.float32)
        assert torch.empty is marked
    finally:
        torch.empty = real
    for t in made:
        assert not t.any(), t.dtype            # this call site is not on the uint8 allow-list
    assert _all_bytes(f, poison.FILL_BYTE[fill])


def test_uint8_allow_list_is_by_call_site(monkeypatch):
    def _attn_forward():                          # (same function name; the file name is what differs)
        return torch.empty(16, dtype=torch.uint8)

    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real(*a, **k).zero_())
    with poisoned_empty("nan", devices="all"):
        off = _attn_forward()
    assert not off.any()
    monkeypatch.setitem(poison.UINT8_FLOAT_SITES, ("test_poison_alloc.py", "_attn_forward"), "this test")
    for fill, byte in poison.FILL_BYTE.items():
        with poisoned_empty(fill, devices="all"):
            on = _attn_forward()
        assert (on == byte).all()
    for site, src in poison.UINT8_FLOAT_SITES.items():
        if src != "this test":
            assert src.startswith("csrc/") and ":" in src, site      # every entry names its source line


def test_gpu_mode_leaves_cpu_tensors_alone():
    real = torch.empty
    torch.empty = lambda *a, **k: real(*a, **k).zero_()
    try:
        with poisoned_empty("nan"):
            t = torch.empty(8)
    finally:
        torch.empty = real
    assert not t.any()


def test_restored_after_exit_and_after_exception():
    names = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with poisoned_empty("big", devices="all"):
        assert torch.empty is not names[0] and torch.Tensor.new_empty is not names[3]
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == names
    with pytest.raises(ZeroDivisionError):
        with poisoned_empty("nan", devices="all"):
            1 / 0
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == names
    with pytest.raises(ValueError):
        with poisoned_empty("zero"):
            pass
    with poisoned_empty("nan", devices="all"):      # nests: the inner block restores the outer wrappers, the outer the originals
        outer = torch.empty
        with poisoned_empty("big", devices="all"):
            assert float(torch.empty(1)[0]) == BIG32
        assert torch.empty is outer
    assert torch.empty is names[0]


def _toy(x, rows_written):
    """Column sums over a padded scratch buffer of 8 rows: a correct op writes all 8 (zeros below the data), a wrong one
    only the rows it has data for -- and then sums the stale rest."""
    buf = torch.empty((8, x.shape[1]), dtype=torch.float32)
    buf[: x.shape[0]] = x
    buf[x.shape[0]:rows_written] = 0.0
    return {"colsum": buf.sum(0)}


def test_partly_written_buffer_is_caught():
    x = torch.arange(15, dtype=torch.float32).view(5, 3)
    good = run_both_fills(lambda: _toy(x, 8), devices="all")
    assert_fill_independent(*good, "toy, all rows written")
    assert torch.equal(good[0]["colsum"], x.sum(0))
    bad = run_both_fills(lambda: _toy(x, 7), devices="all")      # one pad row left as allocated
    with pytest.raises(AssertionError, match="non-finite"):
        assert_fill_independent(*bad, "toy, one row stale")
    # ... and where the stale element does not reach the result as NaN / inf, the bitwise comparison catches it
    masked = [{"y": torch.tensor([1.0, 2.0])}, {"y": torch.tensor([1.0, 2.0000002])}]
    with pytest.raises(AssertionError, match="differs between the fills"):
        assert_fill_independent(*masked, "toy, last bit")
    # the float-atomic rows: equality replaced by the family's bound for the named tensors only
    seen = []
    assert_fill_independent(*masked, "toy, tolerant", tolerant=("y",), bound=lambda n, a, b: seen.append(n))
    assert seen == ["y"]
    nan = [{"loss": torch.tensor(float("nan"))}] * 2
    assert_fill_independent(*nan, "documented NaN", allow_nan=("loss",))
