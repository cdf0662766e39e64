"""tests/redzone.py on CPU tensors (devices="all"): every layout and signature variant keeps what the unpatched allocator
chose, the margins have the documented size, alignment and value, the patched names are restored, and the method itself --
plain torch indexing stands in for a bad kernel, every write stays inside the backing buffer the test owns.  MUTATIONS is
the table of DESIGN.md ("Red zones"): what each stand-in damages, and under which fill check() sees it."""
import re

import pytest
import torch
from torch import nn

import poison
import redzone
from poison import assert_fill_independent
from redzone import guarded_copy, margin, redzoned_empty, run_both

NAMES = (("empty", torch), ("empty_like", torch), ("empty_strided", torch), ("new_empty", torch.Tensor), ("zeros", torch),
         ("zeros_like", torch), ("new_zeros", torch.Tensor), ("to", torch.Tensor), ("cuda", torch.Tensor))


def _current():
    return tuple(getattr(owner, name) for name, owner in NAMES)


def _variants(like, like3=torch.ones(2, 3, 4).permute(2, 0, 1), none=torch.ones(3, 0)):
    """(what, allocation) for every layout and signature variant; run once unpatched and once inside the context."""
    return [
        ("contiguous", lambda: torch.empty((4, 6), dtype=torch.float32)),
        ("varargs", lambda: torch.empty(4, 6, dtype=torch.float32)),
        ("default dtype", lambda: torch.empty(5)),
        ("size=", lambda: torch.empty(size=(2, 2), dtype=torch.float32)),
        ("dtype= device=", lambda: torch.empty(7, device="cpu", dtype=torch.bfloat16)),
        ("device object f64", lambda: torch.empty((2, 3), device=torch.device("cpu"), dtype=torch.float64)),
        ("channels_last", lambda: torch.empty((2, 3, 4, 5), dtype=torch.float32, memory_format=torch.channels_last)),
        ("requires_grad", lambda: torch.empty((3, 3), dtype=torch.float32, requires_grad=True)),
        ("int64", lambda: torch.empty((3, 5), dtype=torch.int64)),
        ("int32", lambda: torch.empty(9, dtype=torch.int32)),
        ("bool", lambda: torch.empty((2, 9), dtype=torch.bool)),
        ("uint8", lambda: torch.empty(33, dtype=torch.uint8)),
        ("empty_like", lambda: torch.empty_like(like)),
        ("empty_like dtype=", lambda: torch.empty_like(like, dtype=torch.bfloat16)),
        ("empty_like transposed", lambda: torch.empty_like(like.t())),
        ("empty_like permuted", lambda: torch.empty_like(like3)),
        ("empty_like contiguous_format", lambda: torch.empty_like(like.t(), memory_format=torch.contiguous_format)),
        ("empty_strided padded rows", lambda: torch.empty_strided((3, 4), (8, 1), dtype=torch.float32)),
        ("empty_strided permuted", lambda: torch.empty_strided((3, 4), (1, 3), dtype=torch.bfloat16)),
        ("new_empty tuple", lambda: like.new_empty((2, 7))),
        ("new_empty varargs", lambda: like.new_empty(2, 7)),
        ("new_empty dtype=", lambda: like.new_empty((6,), dtype=torch.bfloat16)),
        ("new_empty dtype= device=", lambda: like.new_empty((6,), dtype=torch.float64, device="cpu")),
        ("zeros", lambda: torch.zeros((4, 6), dtype=torch.float32)),
        ("zeros varargs bf16", lambda: torch.zeros(3, 7, dtype=torch.bfloat16, device="cpu")),
        ("zeros int32", lambda: torch.zeros(9, dtype=torch.int32)),
        ("zeros_like transposed", lambda: torch.zeros_like(like.t())),
        ("zeros_like dtype=", lambda: torch.zeros_like(like, dtype=torch.float64)),
        ("new_zeros", lambda: like.new_zeros((2, 7))),
        ("zero elements", lambda: torch.empty((0, 4), dtype=torch.float32)),
        ("zero elements like", lambda: torch.empty_like(none)),
    ]


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_layouts_are_what_the_unpatched_allocator_chose(fill):
    like = torch.zeros(3, 5)
    plain = [(what, make()) for what, make in _variants(like)]
    with redzoned_empty(fill, devices="all") as rz:
        zoned = [make() for _, make in _variants(like)]
        n_buffers = len(rz.registry)
        rz.check()
    assert n_buffers == sum(p.numel() > 0 for _, p in plain)       # zero-element tensors come back untouched
    for (what, p), z in zip(plain, zoned):
        assert (z.dtype, z.shape, z.stride(), z.requires_grad, z.device) == (p.dtype, p.shape, p.stride(), p.requires_grad, p.device), what
        assert z.is_contiguous() == p.is_contiguous(), what
        assert z.is_contiguous(memory_format=torch.channels_last) == p.is_contiguous(memory_format=torch.channels_last) \
            if z.dim() == 4 else True, what
        assert not what.startswith(("zeros", "new_zeros")) or not z.any(), what
        assert z.is_leaf and z._base is None, what                  # a tensor of its own, not an autograd view
        if p.numel() == 0:
            assert z.untyped_storage().nbytes() == p.untyped_storage().nbytes(), what
            continue
        span = p.untyped_storage().nbytes()
        assert z.untyped_storage().nbytes() == span + 2 * margin(span), what
        assert z.storage_offset() * z.element_size() == margin(span), what
    b16 = zoned[0].view(torch.bfloat16)                              # reinterpreting a red-zoned tensor works as on a plain one
    assert b16.shape == (4, 12) and b16.data_ptr() == zoned[0].data_ptr()


def test_margin_rule():
    assert margin(1) == margin(14) == margin(4096) == 4096            # at least 4 KiB
    assert margin(4097) == 4608 and margin(5000) == 5120              # else the span rounded up to 512
    assert margin((1 << 20) - 1) == margin(1 << 20) == margin(1 << 30) == 1 << 20      # capped at 1 MiB
    assert all(margin(s) % 512 == 0 for s in range(1, 20000, 7))
    with redzoned_empty("nan", devices="all") as rz:
        t = torch.empty(7, dtype=torch.bfloat16)                      # span 14: the back margin starts at byte 14, unrounded
        e = rz.registry[-1]
        assert (e.front, e.span, e.backing.numel()) == (4096, 14, 4096 + 14 + 4096)
        assert t.data_ptr() == e.backing.data_ptr() + e.front
        assert e.site == ("test_redzone_alloc.py", "test_margin_rule") and e.dtype == torch.bfloat16 and e.shape == (7,)


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_floats_are_filled_like_poison_and_margins_carry_the_fill(fill):
    byte = poison.FILL_BYTE[fill]
    with redzoned_empty(fill, devices="all") as rz:
        made = [torch.empty(9), torch.empty(9, dtype=torch.bfloat16), torch.empty((2, 3), dtype=torch.float64),
                torch.empty_strided((3, 4), (8, 1), dtype=torch.float32)]
        for e in rz.registry:
            assert bool((e.backing == byte).all()) and e.byte == byte      # interior, row padding and both margins
    if fill == "nan":
        assert all(bool(torch.isnan(t).all()) for t in made)
    else:
        assert all(bool(torch.isfinite(t).all()) and float(t.abs().min()) > 1e38 for t in made)


def test_uint8_workspaces_follow_the_allow_list_of_poison(monkeypatch):
    def _attn_forward():                          # (same function name as the listed site; the file name is what differs)
        return torch.empty(16, dtype=torch.uint8)

    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real(*a, **k).fill_(0x5A))
    with redzoned_empty("nan", devices="all") as rz:
        off = _attn_forward()
        assert rz.registry[-1].byte == 0
    assert (off == 0x5A).all()
    monkeypatch.setitem(poison.UINT8_FLOAT_SITES, ("test_redzone_alloc.py", "_attn_forward"), "this test")
    for fill, byte in poison.FILL_BYTE.items():
        with redzoned_empty(fill, devices="all") as rz:
            on = _attn_forward()
            assert rz.registry[-1].byte == byte and bool((rz.registry[-1].backing == byte).all())
        assert (on == byte).all()
    assert redzone.UINT8_FLOAT_SITES is poison.UINT8_FLOAT_SITES      # imported, not copied


def test_restored_after_exit_and_after_exception():
    names = _current()
    with redzoned_empty("big", devices="all"):
        assert all(now is not was for now, was in zip(_current(), names))
    assert _current() == names
    with pytest.raises(ZeroDivisionError):
        with redzoned_empty("nan", devices="all"):
            1 / 0
    assert _current() == names
    with pytest.raises(ValueError):
        with redzoned_empty("zero"):
            pass
    with pytest.raises(ValueError):
        with redzoned_empty("nan", devices="cpu"):
            pass
    assert _current() == names
    with pytest.raises(RuntimeError, match="no redzoned_empty context"):
        guarded_copy(torch.zeros(3), "cpu")
    with redzoned_empty("nan", devices="all") as outer:      # nests: the inner block restores the outer wrappers
        wrapped = _current()
        with redzoned_empty("big", devices="all") as inner:
            torch.empty(3)
            assert len(inner.registry) == 1 and not outer.registry      # the innermost context owns what is made inside it
        assert _current() == wrapped
    assert _current() == names


def test_gpu_mode_leaves_cpu_tensors_alone():
    x = torch.arange(6.0)
    with redzoned_empty("nan") as rz:
        t = torch.empty(8)
        y = x.to("cpu")
        z = x.to(torch.float64)
        assert not rz.registry
    assert t.storage_offset() == 0 and y is x and z.storage_offset() == 0


# --------------------------------------------------------------------------------------------------- the mutations
def _past_end_one_element():
    t = torch.empty(10)
    t.as_strided((11,), (1,))[10] = 1.0


def _before_start_one_element():
    t = torch.empty(10)
    t.as_strided((1,), (1,), t.storage_offset() - 1)[0] = 1.0


def _extra_row():
    t = torch.empty((5, 64))                               # rows of 256 bytes
    t.as_strided((6, 64), (64, 1))[5] = 1.0


def _bf16_vector_store_tail():
    t = torch.empty(7, dtype=torch.bfloat16)               # span 14 bytes: a 16-byte store of 8 elements ends 2 bytes past it
    t.as_strided((8,), (1,))[:] = 1.0


def _interior_padding():
    t = torch.empty_strided((3, 4), (8, 1), dtype=torch.float32)      # 20 elements of storage: rows 0 and 1 have 4 of padding
    t.as_strided((2, 4), (8, 1), t.storage_offset() + 4)[:] = 1.0


def _ff_bytes_past_end():
    t = torch.empty(10)
    raw = t.view(torch.uint8)
    raw.as_strided((4,), (1,), raw.storage_offset() + 40).fill_(0xFF)


def _7f_bytes_past_end():
    t = torch.empty(10)
    raw = t.view(torch.uint8)
    raw.as_strided((4,), (1,), raw.storage_offset() + 40).fill_(0x7F)


def _past_end_of_zeros():
    t = torch.zeros(10)                                    # the reducer's buckets and the optimizer's flat buffers
    assert not t.any()
    t.as_strided((11,), (1,))[10] = 0.0                    # a zero is no fill value: caught under both


def _ones_past_end_of_int64():
    t = torch.empty(6, dtype=torch.int64)
    t.as_strided((7,), (1,))[6] = 1                        # little endian: only the lowest byte is non-zero


def _zeros_past_end_of_int64():
    t = torch.empty(6, dtype=torch.int64)
    t.as_strided((7,), (1,))[6] = 0


# (stand-in, side, first..last damaged byte, bytes damaged, caught under "nan", caught under "big"): the table of DESIGN.md
MUTATIONS = [
    (_past_end_one_element, "back", "+0..+3", 4, True, True),
    (_before_start_one_element, "front", "-4..-1", 4, True, True),
    (_extra_row, "back", "+0..+255", 256, True, True),
    (_bf16_vector_store_tail, "back", "+0..+1", 2, True, True),
    (_interior_padding, None, None, 0, False, False),              # inside the tensor's own storage: not canary
    (_ff_bytes_past_end, "back", "+0..+3", 4, False, True),        # the fill's own value is not seen under that fill
    (_7f_bytes_past_end, "back", "+0..+3", 4, True, False),
    (_past_end_of_zeros, "back", "+0..+3", 4, True, True),
    (_ones_past_end_of_int64, "back", "+0..+0", 1, True, True),
    (_zeros_past_end_of_int64, None, None, 0, False, False),       # integer margins are zero: the documented blind spot
]


@pytest.mark.parametrize("fill", ["nan", "big"])
@pytest.mark.parametrize("row", MUTATIONS, ids=lambda r: r[0].__name__.lstrip("_"))
def test_mutations(row, fill):
    mutate, side, where, count, caught_nan, caught_big = row
    with redzoned_empty(fill, devices="all") as rz:
        rz.check()
        mutate()
        if not (caught_nan if fill == "nan" else caught_big):
            rz.check()
            return
        with pytest.raises(AssertionError) as err:
            rz.check()
    msg = str(err.value)
    assert f"test_redzone_alloc.py:{mutate.__name__}:" in msg, msg               # the allocation's call site
    assert f"{side} margin damaged, {count} bytes in {where} relative to the tensor's {'start' if side == 'front' else 'end'}" in msg, msg
    assert "1 damaged of 2 margins" in msg and re.search(r"torch\.\w+ \(\d+(, \d+)*,?\)", msg), msg    # dtype and shape


def test_run_both_checks_under_both_fills():
    def case(mutate):
        def fn():
            mutate()
            return dict(y=torch.ones(2))
        return fn

    for mutate in (_ff_bytes_past_end, _7f_bytes_past_end, _past_end_one_element):      # each missed by at most one fill
        with pytest.raises(AssertionError, match="back margin damaged"):
            run_both(case(mutate), devices="all")
    a, b = run_both(case(_interior_padding), devices="all")
    assert torch.equal(a["y"], b["y"])


def test_every_damaged_buffer_is_named():
    with redzoned_empty("big", devices="all") as rz:
        _past_end_one_element()
        torch.empty(3)
        _before_start_one_element()
        with pytest.raises(AssertionError) as err:
            rz.check()
    msg = str(err.value)
    assert "2 damaged of 6 margins" in msg and "_past_end_one_element: " in msg and "_before_start_one_element: " in msg


# --------------------------------------------------------------------------------------------------- reads past the end
def _sum_op(src, extra):
    """A stand-in op: moves its input inside the context, sums n + extra elements of it into a buffer of its own."""
    def fn():
        x = src.to("cpu")
        n = x.numel()
        out = torch.empty(1)
        out[0] = x.as_strided((n + extra,), (1,)).sum()
        return dict(y=out)
    return fn


def test_a_read_past_the_end_of_an_input_is_caught():
    src = torch.arange(1.0, 12.0)
    good = run_both(_sum_op(src, 0), devices="all")
    assert_fill_independent(*good, "sum of n elements")
    assert float(good[0]["y"]) == float(src.sum())
    bad = run_both(_sum_op(src, 1), devices="all")           # the margins are intact: check() passed
    with pytest.raises(AssertionError, match="non-finite|differs between the fills"):
        assert_fill_independent(*bad, "sum of n + 1 elements")


def test_a_read_past_the_end_of_a_workspace_is_caught():
    def op(extra):
        def fn():
            ws = torch.empty(8)
            ws[:] = 1.0
            return dict(y=ws.as_strided((8 + extra,), (1,)).sum().reshape(1))
        return fn

    assert_fill_independent(*run_both(op(0), devices="all"), "sum of the workspace")
    with pytest.raises(AssertionError, match="non-finite|differs between the fills"):
        assert_fill_independent(*run_both(op(1), devices="all"), "sum of the workspace and one more")


# --------------------------------------------------------------------------------------------------- caller inputs
@pytest.mark.parametrize("fill", ["nan", "big"])
def test_moved_inputs_are_red_zoned_copies(fill):
    byte = poison.FILL_BYTE[fill]
    x = torch.arange(12.0).view(3, 4)
    idx = torch.arange(5)
    keep = torch.tensor([True, False, True])
    leaf = torch.ones(3, requires_grad=True)
    with redzoned_empty(fill, devices="all") as rz:
        xd, xt, x16 = x.to("cpu"), x.t().to("cpu"), x.to(device="cpu", dtype=torch.bfloat16)
        idxd, keepd = idx.to("cpu"), keep.to("cpu")
        n = len(rz.registry)
        grad = leaf.to("cpu")                                 # would need its graph: passed through
        plain = guarded_copy(x, "cpu")
        assert n == 5 and len(rz.registry) == 6
        by_dtype = {e.dtype: e for e in rz.registry}
        for dt, want in ((torch.float32, byte), (torch.bfloat16, byte), (torch.int64, 0), (torch.bool, 0)):
            e = by_dtype[dt]
            assert e.byte == want and bool((e.backing[:e.front] == want).all()) and bool((e.backing[e.front + e.span:] == want).all())
        assert all(e.site == ("test_redzone_alloc.py", "test_moved_inputs_are_red_zoned_copies") for e in rz.registry)
        rz.check()
        xd.as_strided((13,), (1,))[12] = 5.0                  # an op that writes past the end of its input
        with pytest.raises(AssertionError, match=r"back margin damaged, 4 bytes in \+0\.\.\+3"):
            rz.check()
    assert grad is leaf
    for got, want in ((xd, x), (xt, x.t()), (x16, x.to(torch.bfloat16)), (idxd, idx), (keepd, keep), (plain, x)):
        assert got is not want and got.dtype == want.dtype and torch.equal(got, want) and got.storage_offset() > 0
    assert xt.stride() == x.t().stride() and not xd.requires_grad


def test_module_to_lives_with_the_wrapper():
    """nn.Module.to moves parameters and buffers through Tensor.to: they come out red-zoned, still nn.Parameters, still
    trainable -- the FlatAdam cases build their nn.Sequential inside the context."""
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(5, 3), nn.BatchNorm1d(3))
    want = {k: v.clone() for k, v in net.state_dict().items()}
    with redzoned_empty("nan", devices="all") as rz:
        net = net.to(torch.float64)                           # (on the CPU a move to "cpu" hands the parameters back as they are)
        assert len(rz.registry) == len(want)                  # weight, bias, BN weight, bias, two running stats, the int64 counter
        for p in net.parameters():
            assert isinstance(p, nn.Parameter) and p.requires_grad and p.is_leaf and p.storage_offset() > 0
        net(torch.ones(4, 5, dtype=torch.float64)).sum().backward()
        with torch.no_grad():
            for p in net.parameters():
                p -= 0.1 * p.grad
        rz.check()
    assert all(p.grad is not None for p in net.parameters())
    assert torch.equal(net.state_dict()["1.running_var"] != want["1.running_var"], torch.ones(3, dtype=torch.bool))
    assert int(net.state_dict()["1.num_batches_tracked"]) == 1


# --------------------------------------------------------------------------------------------------- integer tensors
@pytest.mark.parametrize("fill", ["nan", "big"])
def test_integer_interiors_are_the_allocators_and_margins_are_zero(fill, monkeypatch):
    """An allocator that hands back a known pattern stands in for torch.empty: the interior must come out as that pattern
    (nothing copied, nothing filled), both margins zero under either fill."""
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real(*a, **k).view(torch.uint8).fill_(0x5A).view(k.get("dtype", torch.float32)))
    with redzoned_empty(fill, devices="all") as rz:
        for dt in (torch.int32, torch.int64, torch.int16, torch.int8, torch.bool, torch.uint8):
            t = torch.empty(8, dtype=dt)
            e = rz.registry[-1]
            assert e.byte == 0 and not e.backing[:e.front].any() and not e.backing[e.front + e.span:].any(), dt
            assert bool((e.backing[e.front:e.front + e.span] == 0x5A).all()), dt
            assert bool((t.view(torch.uint8) == 0x5A).all()), dt
        f = torch.empty(8, dtype=torch.float32)
        assert bool((rz.registry[-1].backing == poison.FILL_BYTE[fill]).all()) and f.numel() == 8
        rz.check()
