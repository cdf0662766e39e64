"""Host logic of the KV-cached decode, on the CPU: no CPU path, no autograd, capacity checked before any launch, and
the two new entry points validate their arguments before any device work."""
import ctypes
import types

import pytest
import torch


class _StubVQ(torch.nn.Module):
    def __init__(self, codebook_size, num_patches):
        super().__init__()
        self.codebook = types.SimpleNamespace(codebook_size=codebook_size)
        self.num_patches = num_patches

    def decode_indices(self, ids):
        return ids


def _parti():
    from amk.models import Parti

    return Parti(64, _StubVQ(48, 6), None, None, 77, 2, 32, 1).eval()


def test_decode_has_no_cpu_path():
    from amk import ops
    from amk.models import Transformer

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _parti().sample(torch.randn(2, 7, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention_decode(torch.randn(2, 1, 64), torch.randn(2, 1, 128), torch.zeros(2, 8, 128),
                             torch.zeros(1, dtype=torch.int32), 2, 32, 32 ** -0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Transformer(64, 50, 2, 32, 1, 1, 50).eval().sample(torch.randint(0, 50, (2, 5)), max_len=3)


def test_decode_refuses_tensors_that_require_grad():
    from amk import ops

    q = torch.randn(2, 1, 64, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.attention_decode(q, torch.randn(2, 1, 128), torch.zeros(2, 8, 128), torch.zeros(1, dtype=torch.int32),
                             2, 32, 32 ** -0.5)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.attention_decode(q.detach(), None, torch.zeros(2, 8, 128, requires_grad=True), None, 2, 32, 32 ** -0.5)


def test_capacity_below_num_patches_is_refused_before_any_launch():
    m = _parti()
    with pytest.raises(ValueError, match="capacity 5 is smaller than the 6 image tokens"):
        m.begin_decode(torch.randn(2, 7, 64), capacity=5)   # raised ahead of context_norm: nothing ran
    with pytest.raises(ValueError, match="tau"):
        m.sample(torch.randn(2, 7, 64), tau=0.0)
    with pytest.raises(TypeError, match="CLIP"):
        m.sample(["a photo"])


def test_entry_points_validate_before_device_work():
    from amk import lib

    L = lib.load()
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(4096)   # aligned, never dereferenced: every call below is refused on the host
    strides = [64, 32, 128, 32, 1024, 128, 32, 64, 32]
    assert L.amk_attn_decode_ws_floats(2, 3, 64, 200) >= 2 * 3 * 4 * (64 + 2) + 2 * 3
    assert L.amk_attn_decode_ws_floats(0, 3, 64, 200) == 0
    assert L.amk_attn_decode(p, p, p, p, p, p, p, p, null, 2, 2, 48, 8, *strides, 0.125, null) == -2   # head dim
    assert b"head dim 48" in L.amk_last_error()
    assert L.amk_attn_decode(p, p, p, p, p, p, p, p, null, 2, 2, 288, 8, *strides, 0.125, null) == -2
    assert L.amk_attn_decode(null, p, p, p, p, p, p, p, null, 2, 2, 32, 8, *strides, 0.125, null) == -1
    assert b"null" in L.amk_last_error()
    assert L.amk_attn_decode(p, p, null, p, p, p, p, p, null, 2, 2, 32, 8, *strides, 0.125, null) == -1   # k_new alone
    assert L.amk_attn_decode(p, p, p, p, p, p, p, null, null, 2, 2, 32, 8, *strides, 0.125, null) == -1   # append, no n_dev
    assert L.amk_attn_decode(p, p, p, p, p, p, null, p, null, 2, 2, 32, 8, *strides, 0.125, null) == -1   # no workspace
    assert L.amk_attn_decode(p, p, p, p, p, p, p, p, null, 2, 2, 32, 0, *strides, 0.125, null) == -1      # capacity 0
    odd = ctypes.c_void_p(4100)
    assert L.amk_attn_decode(odd, p, p, p, p, p, p, p, null, 2, 2, 32, 8, *strides, 0.125, null) == -1
    assert b"aligned" in L.amk_last_error()
    bad = list(strides)
    bad[5] = 130
    assert L.amk_attn_decode(p, p, p, p, p, p, p, p, null, 2, 2, 32, 8, *bad, 0.125, null) == -1
