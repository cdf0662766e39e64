"""Host logic of the bf16 decode, on the CPU: the two new entry points validate their arguments before any device work,
the ops refuse CPU tensors and other dtypes, and a decode state is f32 outside autocast."""
import ctypes

import pytest
import torch


def test_entry_points_validate_before_device_work():
    from amk import lib

    L = lib.load()
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(4096)   # aligned, never dereferenced: every call below is refused on the host
    strides = [64, 32, 128, 32, 1024, 128, 32, 64, 32]
    dec = L.amk_attn_decode_bf16
    assert dec(p, p, p, p, p, p, p, p, null, 2, 2, 48, 8, *strides, 0.125, null) == -2
    assert b"head dim 48" in L.amk_last_error()
    assert dec(p, p, p, p, p, p, p, p, null, 2, 2, 288, 8, *strides, 0.125, null) == -2
    assert dec(null, p, p, p, p, p, p, p, null, 2, 2, 32, 8, *strides, 0.125, null) == -1
    assert dec(p, p, null, p, p, p, p, p, null, 2, 2, 32, 8, *strides, 0.125, null) == -1       # k_new alone
    assert dec(p, p, p, p, p, p, p, null, null, 2, 2, 32, 8, *strides, 0.125, null) == -1       # append, no n_dev
    assert dec(p, p, p, p, p, p, null, p, null, 2, 2, 32, 8, *strides, 0.125, null) == -1       # no workspace
    assert dec(ctypes.c_void_p(4104), p, p, p, p, p, p, p, null, 2, 2, 32, 8, *strides, 0.125, null) == -1
    assert b"aligned" in L.amk_last_error()
    bad = list(strides)
    bad[5] = 132                # a multiple of 4, as the f32 kernel takes, but not of 8
    assert dec(p, p, p, p, p, p, p, p, null, 2, 2, 32, 8, *bad, 0.125, null) == -1
    assert b"multiples of 8" in L.amk_last_error()
    rows = L.amk_gemm_rows_bf16
    assert rows(null, 176, p, 176, null, p, 132, 8, 130, 170, 0, null) == -1
    assert rows(p, 176, p, 176, null, p, 132, 8, 130, 0, 0, null) == -1                          # K = 0
    assert rows(p, 172, p, 176, null, p, 132, 8, 130, 170, 0, null) == -1                        # ldx % 8
    assert rows(p, 176, p, 168, null, p, 132, 8, 130, 170, 0, null) == -1                        # ldw < K
    assert rows(p, 176, p, 176, null, p, 130, 8, 130, 170, 1, null) == -1                        # ldy % 4
    assert rows(ctypes.c_void_p(4104), 176, p, 176, null, p, 132, 8, 130, 170, 0, null) == -1
    assert b"aligned" in L.amk_last_error()
    assert L.amk_version() == 140


def test_the_ops_have_no_cpu_path_and_no_autograd():
    from amk import ops

    bf = torch.bfloat16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention_decode(torch.zeros(2, 1, 64, dtype=bf), torch.zeros(2, 1, 128, dtype=bf), torch.zeros(2, 8, 128, dtype=bf),
                             torch.zeros(1, dtype=torch.int32), 2, 32, 32 ** -0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_rows_bf16(torch.zeros(2, 64, dtype=bf), torch.zeros(16, 64, dtype=bf))
    with pytest.raises(RuntimeError, match="bf16 matrices"):
        ops.linear_rows_bf16(torch.zeros(2, 64), torch.zeros(16, 64, dtype=bf))
    with pytest.raises(RuntimeError, match="float32 or a bfloat16 cache"):
        ops.attention_decode(torch.zeros(2, 1, 64).half(), None, torch.zeros(2, 8, 128).half(), None, 2, 32, 32 ** -0.5)


def test_state_dtype_outside_autocast():
    """(The autocast side runs on the GPU: tests/test_parti_decode_bf16_gpu.py.)"""
    from amk.models.transformer import Decoder

    assert Decoder.decode_dtype("cuda") == torch.float32
    assert Decoder.decode_dtype("cpu") == torch.float32
    assert Decoder.decode_dtype("cuda", torch.bfloat16) == torch.bfloat16
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        Decoder.decode_dtype("cuda", torch.float16)
