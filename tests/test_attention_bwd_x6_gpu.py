"""The kept-scores attention backward with its dV and dK products on split-bf16 MFMA (AMK_ATTN_BWD_X6,
csrc/attn_bwd_fused_x6.hip) against the f32 variant of the same call -- the yardstick of tests/attn_bwd_x6_ref.py: per
element, worst |got - fp64| / A within FACTOR = 2 of the f32 variant's -- with dq bitwise the f32 variant's, and the
"auto" dispatch of ops.ATTENTION_BACKWARD_X6.  The small shapes force the variant through stages = 9 | 32 | 128."""
import pytest
import torch

import attn_bwd_x6_ref as ref
from util import assert_close

pytestmark = pytest.mark.gpu
D = 64
SCALE = D ** -0.5
TOL = 2e-5   # tests/test_attention_x6_keep_gpu.py
F32, X6 = 9 | 32, 9 | 32 | 128          # delta + fused at 256 keys per workgroup; the same on split-bf16
REPRO = 64
SHAPES = [(1, 1, 32, 256), (2, 2, 40, 77), (1, 2, 200, 130), (2, 1, 33, 300), (1, 1, 256, 320), (1, 1, 1, 1), (1, 2, 95, 512)]


@pytest.fixture(autouse=True)
def restore_ops():
    from amk import ops

    names = ("ATTENTION_FORWARD", "ATTENTION_BACKWARD_X6", "ATTENTION_BWD_X6_MIN_SCORES", "KERNEL_EVENTS",
             "DETERMINISTIC_ATTENTION_BACKWARD", "ATTENTION_BACKWARD_KEYS")
    old = {n: getattr(ops, n) for n in names}
    yield ops
    for n, v in old.items():
        setattr(ops, n, v)


def _bthd(t, device):
    """(B, H, T, D) on the CPU -> the same values as a (B, H, T, D) view of (B, T, H, D) storage on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(device).permute(0, 2, 1, 3)


def _forward(ops, q, k, v, km, cm):
    q, k, v, o, stats, scores = ops._attn_forward(q, k, v, km, cm, SCALE, keep_scores=True)
    assert scores is not None
    return q, k, v, o, stats, scores


def _backward(ops, fwd, d_o, km, cm, stages, kept=True):
    q, k, v, o, stats, scores = fwd
    B, H, I, _ = q.shape
    dq, dk, dv = (ops._new_bthd(B, H, T, D, q) for T in (I, k.shape[2], k.shape[2]))
    for t in (dq, dk, dv):
        t.fill_(float("nan"))
    ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, km, cm, SCALE, stages=stages, scores=scores if kept else None)
    return dq, dk, dv


@pytest.mark.parametrize("mode", ref.MASKS)
@pytest.mark.parametrize("B,H,I,J", SHAPES)
def test_dk_dv_within_the_factor_of_the_f32_variant_and_dq_bitwise(device, restore_ops, B, H, I, J, mode):
    ops = restore_ops
    km, cm = ref.make_masks(mode, B, I, J)
    kmd, cmd = (None if m is None else m.to(device) for m in (km, cm))
    for fi, family in enumerate(ref.FAMILIES):
        cpu = ref.make_inputs(family, B, H, I, J, 4000 + 10 * I + fi)
        want = ref.reference(*cpu, SCALE, km, cm)
        q, k, v, d_o = (_bthd(t, device) for t in cpu)
        fwd = _forward(ops, q, k, v, kmd, cmd)
        f32 = _backward(ops, fwd, d_o, kmd, cmd, F32 | REPRO)
        x6 = _backward(ops, fwd, d_o, kmd, cmd, X6 | REPRO)
        assert torch.equal(x6[0], f32[0]), f"{family}: dq is not bitwise the f32 variant's"
        for name, a, b in (("dk", x6[1], f32[1]), ("dv", x6[2], f32[2])):
            fig_x6 = ref.figure(a, want[name], want["A_" + name])
            fig_32 = ref.figure(b, want[name], want["A_" + name])
            print(f"{family} {mode} {(B, H, I, J)} {name}: split-bf16 {fig_x6[0]:.3e} f32 {fig_32[0]:.3e} "
                  f"(A = 0: {fig_x6[1]:.3e} / {fig_32[1]:.3e})")
            assert ref.within_factor(fig_x6, fig_32), (family, name, fig_x6, fig_32)
        # reproducible, and dk / dv do not depend on how dq leaves
        again = _backward(ops, fwd, d_o, kmd, cmd, X6 | REPRO)
        atomics = _backward(ops, fwd, d_o, kmd, cmd, X6)
        for name, a, b, c in zip(("dq", "dk", "dv"), x6, again, atomics):
            assert torch.equal(a, b), f"{family}: {name} differs between two runs"
            if name != "dq":
                assert torch.equal(a, c), f"{family}: {name} differs between the atomic and the reproducible dq form"
        assert_close(atomics[0], x6[0], TOL, "dq by atomics against the reproducible dq")


def test_batch_and_head_are_independent(device, restore_ops):
    """A (batch, head) slice of a larger call equals the call on that slice alone, bit for bit.  Five query tiles: the
    kernel starts (batch, head) slice n at query tile 5 n mod tiles, so here every slice starts at tile 0 and sums its
    tiles in the same order in both calls (at another tile count dk and dv would agree up to that order only)."""
    ops = restore_ops
    B, H, I, J = 2, 2, 150, 300
    cpu = ref.make_inputs("normal", B, H, I, J, 77)
    km, _ = ref.make_masks("key_mask", B, I, J)
    q, k, v, d_o = (_bthd(t, device) for t in cpu)
    whole = _backward(ops, _forward(ops, q, k, v, km.to(device), None), d_o, km.to(device), None, X6 | REPRO)
    for b, h in ((0, 1), (1, 0)):
        qs, ks, vs, gs = (_bthd(t[b:b + 1, h:h + 1], device) for t in cpu)
        kms = km[b:b + 1].to(device)
        part = _backward(ops, _forward(ops, qs, ks, vs, kms, None), gs, kms, None, X6 | REPRO)
        for name, a, w in zip(("dq", "dk", "dv"), part, whole):
            assert torch.equal(a[0, 0], w[b, h]), (name, b, h)


def test_refusals(device, restore_ops):
    """AMK_EUNSUPPORTED, nothing launched: head dim other than 64, 128 keys per workgroup forced or chosen, no fused bit,
    no kept scores (amk_attn_bwd), strided dq."""
    ops = restore_ops
    B, H, I, J = 1, 2, 40, 300

    def refused(fwd, d_o, stages, kept=True, dq=None):
        q, k, v, o, stats, scores = fwd
        dh = q.shape[3]
        dk, dv = (torch.full((B, J, H, dh), float("nan"), device=device).permute(0, 2, 1, 3) for _ in range(2))
        if dq is None:
            dq = torch.full((B, I, H, dh), float("nan"), device=device).permute(0, 2, 1, 3)
        with pytest.raises(RuntimeError, match=r"code -2: .*AMK_ATTN_BWD_X6"):
            ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, None, None, SCALE, stages=stages,
                               scores=scores if kept else None)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dk).all()) and bool(torch.isnan(dq).all()), "a refused call wrote its outputs"

    mk = lambda T, dh, seed: _bthd(ref.seeded((B, H, T, dh), seed), device)
    fwd64 = ops._attn_forward(mk(I, 64, 1), mk(J, 64, 2), mk(J, 64, 3), None, None, SCALE, keep_scores=True)
    fwd128 = ops._attn_forward(mk(I, 128, 1), mk(J, 128, 2), mk(J, 128, 3), None, None, 128 ** -0.5, keep_scores=True)
    assert fwd64[5] is not None and fwd128[5] is not None
    refused(fwd128, mk(I, 128, 4), 9 | 128)                      # head dim
    refused(fwd64, mk(I, 64, 4), 9 | 16 | 128)                   # 128 keys forced
    refused(tuple(t[:, :, :100] if i in (1, 2) else t for i, t in enumerate(fwd64)), mk(I, 64, 4), 9 | 128)   # ... chosen: J = 100
    refused(fwd64, mk(I, 64, 4), 7 | 128)                        # no fused bit
    refused(fwd64, mk(I, 64, 4), X6, kept=False)                 # amk_attn_bwd
    refused(fwd64, mk(I, 64, 4), X6, dq=torch.full((B, H, I, 64), float("nan"), device=device))   # strided dq


def _train(ops, q, k, v, cot):
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qd, kd, vd, SCALE)
    return (o,) + torch.autograd.grad((o * cot).sum(), [qd, kd, vd])


def test_autograd_dispatch(device, restore_ops):
    """"auto" from ATTENTION_BWD_X6_MIN_SCORES scores on (lowered here), not below it, never for a caller's own `stages`;
    "0" restores the f32 products: under the reproducible mode the gradients are those of stages 73 bit for bit."""
    ops = restore_ops
    B, H, I, J = 1, 2, 150, 256
    cpu = ref.make_inputs("normal", B, H, I, J, 5)
    want = ref.reference(*cpu, SCALE)
    q, k, v, cot = (_bthd(t, device) for t in cpu)
    ops.DETERMINISTIC_ATTENTION_BACKWARD = True
    ops.ATTENTION_BWD_X6_MIN_SCORES = B * H * I * J
    fwd = ops._attn_forward(q, k, v, None, None, SCALE, keep_scores=True, auto_x6=True)
    by_bits = {st: _backward(ops, fwd, cot, None, None, st) for st in (73, 73 | 32 | 128)}
    assert not torch.equal(by_bits[73][1], by_bits[73 | 32 | 128][1])      # the two variants are told apart by dk's last bits
    for mode, min_scores, bits in (("auto", B * H * I * J, 73 | 32 | 128), ("auto", B * H * I * J + 1, 73),
                                   ("0", 1, 73), ("1", 1 << 40, 73 | 32 | 128)):
        ops.ATTENTION_BACKWARD_X6, ops.ATTENTION_BWD_X6_MIN_SCORES = mode, min_scores
        ops.KERNEL_EVENTS = {}
        o, *g = _train(ops, q, k, v, cot)
        assert "attn_bwd_fused_kernel(kept scores)" in ops.KERNEL_EVENTS, set(ops.KERNEL_EVENTS)
        ops.KERNEL_EVENTS = None
        for name, a, b in zip(("dq", "dk", "dv"), g, by_bits[bits]):
            assert torch.equal(a, b), (mode, min_scores, name)
            assert_close(a, want[name].float(), TOL, f"{mode} {name}")
    ops.ATTENTION_BACKWARD_X6 = "auto"
    ops.ATTENTION_BWD_X6_MIN_SCORES = 1
    same = _backward(ops, fwd, cot, None, None, 73)                          # a caller's own stages: exactly those bits
    assert all(torch.equal(a, b) for a, b in zip(same, by_bits[73]))


def test_graph_capture(device, restore_ops):
    """One captured and replayed forward + backward equals the eager one under the reproducible mode."""
    ops = restore_ops
    B, H, I, J = 2, 2, 100, 300
    ops.DETERMINISTIC_ATTENTION_BACKWARD = True
    ops.ATTENTION_BACKWARD_X6 = "1"
    q, k, v, cot = (_bthd(t, device) for t in ref.make_inputs("normal", B, H, I, J, 9))
    step = lambda: list(_train(ops, q, k, v, cot))
    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, static):
        assert torch.equal(a, b)
