"""SoftmaxAttention at head dims 96 to 256, no GPU: the CPU oracle against the reference-pinned fixtures
(tools/gen_attention_golden_dh.py), and the C ABI's answers for the head dims it takes (a multiple of 32 from 32 to 256)
and the ones it refuses -- all given before any device work."""
import ctypes

import pytest
import torch

from amk import lib as amk_lib
from oracle import ref_cpu
from util import assert_close, load_golden, weights_of

TOL = 2e-5
NEW_DIMS = (96, 160, 192, 224, 256)
AMK_EINVAL, AMK_EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("d", [96, 192, 256])
@pytest.mark.parametrize("variant", ["self", "cross_ctxmask", "self_causal"])
def test_softmax_head_dim_oracle_matches_reference(d, variant):
    fx = load_golden(f"softmax_attention_d{d}")
    dim, h, dd = (int(v) for v in fx["dims"])
    assert dd == d
    w0 = weights_of(fx)
    w = {n: v.clone().requires_grad_(True) for n, v in w0.items()}
    x = torch.from_numpy(fx["x"]).requires_grad_(True)
    ctx = torch.from_numpy(fx["context"]).requires_grad_(True)
    kw = {"self": dict(),
          "cross_ctxmask": dict(context=ctx, context_mask=torch.from_numpy(fx["ctxmask"])),
          "self_causal": dict(causal_mask=torch.from_numpy(fx["causal"]))}[variant]
    out = ref_cpu.softmax_attention(x, w, h, d, **kw)
    assert_close(out, fx[f"{variant}:out"], TOL, "out")
    names = sorted(w)
    wrt = [x] + ([ctx] if "context" in kw else []) + [w[n] for n in names]
    gs = torch.autograd.grad((out * torch.from_numpy(fx["cot"])).sum(), wrt)
    assert_close(gs[0], fx[f"{variant}:gx"], TOL, "grad x")
    off = 1
    if "context" in kw:
        assert_close(gs[1], fx[f"{variant}:gctx"], TOL, "grad context")
        off = 2
    if f"{variant}:g:W_o.weight" in fx:
        for n, g in zip(names, gs[off:]):
            assert_close(g, fx[f"{variant}:g:{n}"], TOL, f"grad {n}")


def _dummy():
    """A non-null host pointer 4 bytes past a 16-byte boundary: it passes the null checks and fails the alignment
    check, which comes after the head-dim check and before any HIP call."""
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    return buf, ctypes.c_void_p(((base + 15) & ~15) + 4)


def _fwd(L, fn, d, p, extra=()):
    B, H, T = 1, 2, 16
    st = [H * T * d, H * d, d]
    null = ctypes.c_void_p(0)
    return fn(*([p] * 5), *extra, null, null, B, H, T, T, d, *(st * 4), 1.0, null)


def _bwd(L, d, p):
    B, H, T = 1, 2, 16
    st = [H * T * d, H * d, d]
    null = ctypes.c_void_p(0)
    return L.amk_attn_bwd(*([p] * 10), null, null, B, H, T, T, d, *(st * 8), 1.0, 9, null)


@pytest.mark.parametrize("d", NEW_DIMS)
def test_new_head_dims_pass_the_head_dim_check(d):
    """Taken head dims reach the alignment check (AMK_EINVAL); before, they stopped at the head-dim check."""
    L = amk_lib.load()
    buf, p = _dummy()
    assert _fwd(L, L.amk_attn_fwd, d, p) == AMK_EINVAL
    assert b"aligned" in L.amk_last_error(), L.amk_last_error()
    assert _bwd(L, d, p) == AMK_EINVAL
    assert b"aligned" in L.amk_last_error(), L.amk_last_error()


@pytest.mark.parametrize("d", [48, 80, 288])
def test_other_head_dims_still_refused(d):
    L = amk_lib.load()
    buf, p = _dummy()
    assert _fwd(L, L.amk_attn_fwd, d, p) == AMK_EUNSUPPORTED
    msg = L.amk_last_error()
    assert str(d).encode() in msg and b"multiple of 32" in msg, msg
    assert _bwd(L, d, p) == AMK_EUNSUPPORTED
    assert str(d).encode() in L.amk_last_error()


def test_kept_scores_refused_for_new_head_dims():
    """No score-keeping forward nor one-pass backward exists at 96 to 256: kept scores would never be read."""
    L = amk_lib.load()
    buf, p = _dummy()
    assert _fwd(L, L.amk_attn_fwd_keep, 96, p, extra=(p,)) == AMK_EUNSUPPORTED
    assert b"kept scores" in L.amk_last_error(), L.amk_last_error()
    B, H, T, d = 1, 2, 16, 96
    st = [H * T * d, H * d, d]
    null = ctypes.c_void_p(0)
    rc = L.amk_attn_bwd_kept(*([p] * 11), null, null, B, H, T, T, d, *(st * 8), 1.0, 9, null)
    assert rc == AMK_EUNSUPPORTED
    assert b"kept scores" in L.amk_last_error(), L.amk_last_error()
