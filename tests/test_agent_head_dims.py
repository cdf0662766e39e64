"""AgentAttention at head dims 32 and 128, no GPU: the CPU oracle against the reference-pinned fixtures
(tools/gen_agent_golden_dh.py), the head-dim-aware size queries of the C ABI, and the rejection of other head dims
before any device work."""
import ctypes

import pytest
import torch

from amk import lib as amk_lib
from oracle import ref_cpu
from util import assert_close, load_golden, weights_of

TIGHT = 2e-6   # test_oracle_golden.py's tolerance: the oracle restates the reference's fp32 op sequence


@pytest.mark.parametrize("d", [32, 128])
def test_agent_head_dim_oracle_matches_reference(d):
    fx = load_golden(f"agent_d{d}")
    dim, h, dd, agent_num = (int(v) for v in fx["dims"])
    assert dd == d
    w0 = weights_of(fx)
    assert float(w0["bias1"].abs().min()) > 0.0 and float(w0["bias2"].abs().min()) > 0.0
    w = {n: v.clone().requires_grad_(True) for n, v in w0.items()}
    x = torch.from_numpy(fx["x"]).requires_grad_(True)
    out = ref_cpu.agent_attention(x, w, h, d, agent_num)
    assert_close(out, fx["out"], TIGHT, "out")
    names = sorted(w)
    gs = torch.autograd.grad((out * torch.from_numpy(fx["cot"])).sum(), [x] + [w[n] for n in names], allow_unused=True)
    assert_close(gs[0], fx["gx"], TIGHT, "grad x")
    for n, g in zip(names, gs[1:]):
        if n in ("bias1", "bias2"):
            # shift-invariant softmax rows: zero in exact arithmetic; both sides hold only f32 rounding residue
            assert float(g.abs().max()) < 1e-5 and float(abs(fx["g:" + n]).max()) < 1e-5
            continue
        assert_close(g, fx["g:" + n], TIGHT, f"grad {n}")


CHUNK = {32: 128, 64: 128, 128: 64}


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 127, 128, 129, 1024])
def test_agent_dh_size_queries(d, T):
    L = amk_lib.load()
    nc = -(-T // CHUNK[d])
    assert L.amk_agent_num_chunks_dh(T, d) == nc
    B, H, P = 3, 5, 7
    cells, rows = B * H * nc * P, B * H * P
    assert L.amk_agent_ws_floats_dh(B, H, T, P, d, 0) == cells * (d + 2)
    assert L.amk_agent_ws_floats_dh(B, H, T, P, d, 1) == 3 * cells * d + 2 * rows * d + rows
    if d == 64:   # the head-dim-free forms keep their meaning: the D = 64 sizes
        assert L.amk_agent_num_chunks(T) == nc
        assert L.amk_agent_ws_floats(B, H, T, P, 0) == L.amk_agent_ws_floats_dh(B, H, T, P, 64, 0)
        assert L.amk_agent_ws_floats(B, H, T, P, 1) == L.amk_agent_ws_floats_dh(B, H, T, P, 64, 1)


def test_agent_dh_size_queries_reject_other_head_dims():
    L = amk_lib.load()
    for d in (0, 16, 48, 96, 256):
        assert L.amk_agent_num_chunks_dh(100, d) == 0
        assert L.amk_agent_ws_floats_dh(2, 2, 100, 2, d, 0) == 0
        assert L.amk_agent_ws_floats_dh(2, 2, 100, 2, d, 1) == 0


def test_agent_unsupported_head_dim_is_refused_before_device_work():
    """Non-null dummy pointers pass the argument checks; the head-dim check must answer before any HIP call."""
    L = amk_lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    B, H, T, P = 1, 2, 16, 2
    st = [H * T * 48, 48, T * 48]
    rc = L.amk_agent_attn_fwd(*([p] * 10), B, H, T, 48, P, *(st * 4), 1.0, null)
    assert rc == -2, rc
    msg = L.amk_last_error()
    assert b"48" in msg and b"32" in msg and b"64" in msg and b"128" in msg, msg
    rc = L.amk_agent_attn_bwd(*([p] * 14), B, H, T, 48, P, *(st * 7), 1.0, null)
    assert rc == -2, rc
    assert b"48" in L.amk_last_error()
    rc = L.amk_agent_conv_grad_reduce(p, p, 4, 48, p, p, null)
    assert rc == -2, rc
    with pytest.raises(RuntimeError, match="amk_agent_attn_fwd"):
        amk_lib.check(L.amk_agent_attn_fwd(*([p] * 10), B, H, T, 48, P, *(st * 4), 1.0, null), "amk_agent_attn_fwd")
