"""The score-keeping split-bf16 attention forward (amk_attn_fwd_x6_keep, csrc/attn_fwd_x6.hip), its unmasked
specialisation and the "auto" dispatch of ops.ATTENTION_FORWARD.

Kept scores are held per element to the bound derived in tests/attn_x6_ref.py (gamma_384 sum|q'||k| (1 + 2^-7)^2 plus the
truncation of the split, nothing relative to a tensor maximum); the emulation of tests/test_attention_x6_bounds.py stands
at 0.022 of it."""
import pytest
import torch

import attn_x6_ref as ref
from oracle import ref_cpu
from util import assert_close, rel_err, seeded

pytestmark = pytest.mark.gpu
TOL = 2e-5   # tests/test_attention_gpu.py
D = 64
SCALE = D ** -0.5


@pytest.fixture(autouse=True)
def restore_ops():
    from amk import ops

    names = ("ATTENTION_FORWARD", "ATTENTION_KEEP_SCORES", "ATTENTION_KEEP_SCORES_BUDGET_BYTES", "KERNEL_EVENTS",
             "DETERMINISTIC_ATTENTION_BACKWARD", "ATTENTION_BACKWARD_KEYS", "ATTENTION_BACKWARD_TWO_KERNEL",
             "ATTENTION_X6_MIN_SCORES")
    old = {n: getattr(ops, n) for n in names}
    yield ops
    for n, v in old.items():
        setattr(ops, n, v)


def _masks(mode, B, I, J, device):
    km = cm = None
    if mode == "key_mask":
        km = torch.ones(B, J, dtype=torch.uint8)
        km[0, 2::5] = 0
        km[-1, -J // 3:] = 0
        km = km.to(device)
    elif mode == "causal":
        cm = torch.ones(I, J).triu(1).to(torch.uint8).to(device)
    return km, cm


@pytest.mark.parametrize("mode", ["plain", "key_mask", "causal"])
@pytest.mark.parametrize("B,H,I,J", [(1, 1, 32, 32), (2, 2, 40, 77), (1, 2, 200, 130), (1, 1, 256, 320)])
def test_kept_scores_against_fp64_per_element(device, restore_ops, B, H, I, J, mode):
    """Every kept score (the value before any fill, with or without a mask) is inside the per-element bound."""
    ops = restore_ops
    ops.ATTENTION_FORWARD = "bf16x6"
    km, cm = _masks(mode, B, I, J, device)
    for fi, family in enumerate(ref.FAMILIES):
        q, k = ref.make_qk(family, B, H, I, J, 1000 + 10 * I + fi)
        q, k = q.to(device), k.to(device)
        v = seeded((B, H, J, D), 5).to(device)
        *_, scores = ops._attn_forward(q, k, v, km, cm, SCALE, keep_scores=True)
        assert scores is not None
        want, bound = ref.reference(q, k, SCALE)
        nbad, ratio = ref.worst_ratio(ref.unpack_scores(scores, B, H, I, J), want, bound)
        print(f"{family} {mode} {(B, H, I, J)}: worst |err| / bound {ratio:.4f}")
        assert nbad == 0, f"{family}: {nbad} scores outside the bound (worst {ratio:.3g}x)"


@pytest.mark.parametrize("B,H,I,J", [(2, 2, 200, 130), (2, 1, 33, 300)])
def test_backward_consumes_x6_kept_scores(device, restore_ops, B, H, I, J):
    """Layout: dk and dv of amk_attn_bwd_kept on the x6-kept scores agree per element with amk_attn_bwd recomputing the
    scores in f32, on the same q, k, v, o and statistics; 128 and 256 keys per workgroup, dq by atomics and reproducible."""
    ops = restore_ops
    ops.ATTENTION_FORWARD = "bf16x6"
    mk = lambda seed, T: seeded((B, T, H, D), seed).to(device).permute(0, 2, 1, 3)
    q, k, v, d_o = mk(1, I), mk(2, J), mk(3, J), mk(4, I)
    km = torch.ones(B, J, dtype=torch.uint8)
    km[0, 5::7] = 0
    km = km.to(device)
    for mask in (None, km):
        q, k, v, o, stats, scores = ops._attn_forward(q, k, v, mask, None, SCALE, keep_scores=True)
        assert scores is not None
        for keys in (16, 32):          # AMK_ATTN_BWD_KEYS128 / KEYS256
            for stages in (9, 73):     # atomics / reproducible dq
                out = {}
                for kept in (False, True):
                    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
                    ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, mask, None, SCALE, stages=stages | keys,
                                       scores=scores if kept else None)
                    out[kept] = (dq, dk, dv)
                for name, a, b in zip(("dq", "dk", "dv"), out[True], out[False]):
                    assert_close(a, b, 2e-6, f"{name} keys bit {keys} stages {stages} masked {mask is not None}")


@pytest.mark.parametrize("keep", [True, False])
def test_plain_kernel_staircase(device, restore_ops, keep):
    """The input of test_lazy_reference_moves_in_every_tile (tests/test_attention_gpu.py; 70 x 333, the reference has to
    move in every tile, ragged last tile) through the unmasked split-bf16 kernel, keeping the scores or not, against the
    fp64 oracle at that test's tolerances."""
    ops = restore_ops
    ops.ATTENTION_FORWARD = "bf16x6"
    ops.ATTENTION_KEEP_SCORES = keep
    B, H, I, J = 2, 2, 70, 333
    q = seeded((B, H, I, D), 71)
    k = seeded((B, H, J, D), 72) * 0.3
    v = seeded((B, H, J, D), 73)
    cot = seeded((B, H, I, D), 74)
    u = torch.nn.functional.normalize(seeded((D,), 75), dim=0)
    ramp = (torch.arange(J) // 64).float().view(1, 1, J, 1) / (J // 64)
    k = k + ramp * u * 70.0
    q = q + u * torch.linspace(0.0, 6.0, I).view(1, 1, I, 1)
    qc, kc, vc = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref = ref_cpu.attention_core(qc, kc, vc, SCALE)
    g_ref = [g.float() for g in torch.autograd.grad((o_ref * cot.double()).sum(), [qc, kc, vc])]
    ops.KERNEL_EVENTS = {}
    qd, kd, vd = (t.to(device).requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qd, kd, vd, SCALE)
    g = torch.autograd.grad((o * cot.to(device)).sum(), [qd, kd, vd])
    assert set(ops.KERNEL_EVENTS) == ({"attn_fwd_x6_keep_kernel", "attn_bwd_fused_kernel(kept scores)"} if keep else
                                      {"attn_fwd_x6_kernel", "attn_bwd_fused_kernel"})
    assert_close(o, o_ref.detach().float(), TOL, "o")
    for name, a, b in zip(("dq", "dk", "dv"), g, g_ref):
        assert rel_err(a, b) < 1e-3, (name, rel_err(a, b))


@pytest.mark.parametrize("B,H,I,J", [(1, 2, 20, 100), (1, 1, 1, 1), (2, 1, 5, 64)])
@pytest.mark.parametrize("keep", [True, False])
def test_plain_kernel_small_and_ragged(device, restore_ops, B, H, I, J, keep):
    """Fewer than 32 queries with a ragged key tile (J % 64 != 0), one query and one key, exactly one full tile."""
    ops = restore_ops
    ops.ATTENTION_FORWARD = "bf16x6"
    ops.ATTENTION_KEEP_SCORES = keep
    q, k, v, cot = (seeded((B, H, T, D), s) for s, T in ((1, I), (2, J), (3, J), (4, I)))
    qc, kc, vc = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref = ref_cpu.attention_core(qc, kc, vc, SCALE)
    g_ref = torch.autograd.grad((o_ref * cot).sum(), [qc, kc, vc])
    qd, kd, vd = (t.to(device).requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qd, kd, vd, SCALE)
    g = torch.autograd.grad((o * cot.to(device)).sum(), [qd, kd, vd])
    assert_close(o, o_ref, TOL, "o")
    for name, a, b in zip(("dq", "dk", "dv"), g, g_ref):
        if J == 1 and name != "dv":   # one key: dq = dk = 0 in real arithmetic (tests/test_attention_gpu.py _core_case)
            assert float(a.abs().max()) <= 1e-6, name
            continue
        assert_close(a, b, TOL, name)


def _launches(ops, fn):
    ops.KERNEL_EVENTS = {}
    out = fn()
    names = set(ops.KERNEL_EVENTS)
    ops.KERNEL_EVENTS = None
    return out, names


def test_auto_dispatch(device, restore_ops):
    """"auto": ops.attention takes the split-bf16 forward (at or above ATTENTION_X6_MIN_KEYS keys and
    ATTENTION_X6_MIN_SCORES scores) and keeps the scores; a bare _attn_forward stays on the f32 kernel; "f32" restores
    the f32 launches in the autograd path too."""
    ops = restore_ops
    B, H, I, J = 1, 2, 150, ops.ATTENTION_X6_MIN_KEYS
    ops.ATTENTION_X6_MIN_SCORES = B * H * I * J      # a small call for the test: exactly at both thresholds
    q, k, v = (seeded((B, H, T, D), s).to(device) for s, T in ((1, I), (2, J), (3, J)))
    o_ref = ref_cpu.attention_core(q.cpu(), k.cpu(), v.cpu(), SCALE)

    def train():
        qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = ops.attention(qd, kd, vd, SCALE)
        o.sum().backward()
        return o

    ops.ATTENTION_FORWARD = "auto"
    o, names = _launches(ops, train)
    assert names == {"attn_fwd_x6_keep_kernel", "attn_bwd_fused_kernel(kept scores)"}, names
    assert_close(o, o_ref, TOL, "auto")
    _, names = _launches(ops, lambda: ops.attention(q, k, v, SCALE))
    assert names == {"attn_fwd_x6_kernel"}, names
    _, names = _launches(ops, lambda: ops.attention(q, k[:, :, :J - 1], v[:, :, :J - 1], SCALE))
    assert names == {"attn_fwd_kernel"}, names                      # below the key threshold
    _, names = _launches(ops, lambda: ops.attention(q[:, :, :I - 1], k, v, SCALE))
    assert names == {"attn_fwd_kernel"}, names                      # below the score-count threshold
    _, names = _launches(ops, lambda: ops._attn_forward(q, k, v, None, None, SCALE, keep_scores=True))
    assert names == {"attn_fwd_keep_kernel"}, names                 # bare call: f32
    _, names = _launches(ops, lambda: ops._attn_forward(q, k, v, None, None, SCALE))
    assert names == {"attn_fwd_kernel"}, names
    ops.ATTENTION_FORWARD = "f32"
    o, names = _launches(ops, train)
    assert names == {"attn_fwd_keep_kernel", "attn_bwd_fused_kernel(kept scores)"}, names
    assert_close(o, o_ref, TOL, "f32")


def test_budget_exhaustion_falls_back_to_recompute(device, restore_ops):
    ops = restore_ops
    ops.ATTENTION_FORWARD = "bf16x6"
    B, H, I, J = 2, 2, 130, 200
    q, k, v, cot = (seeded((B, H, T, D), s) for s, T in ((1, I), (2, J), (3, J), (4, I)))
    qc, kc, vc = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref = ref_cpu.attention_core(qc, kc, vc, SCALE)
    g_ref = torch.autograd.grad((o_ref * cot).sum(), [qc, kc, vc])

    def train():
        qd, kd, vd = (t.to(device).requires_grad_(True) for t in (q, k, v))
        o = ops.attention(qd, kd, vd, SCALE)
        return (o,) + torch.autograd.grad((o * cot.to(device)).sum(), [qd, kd, vd])

    alive = ops._kept_scores_bytes[0]
    ops.ATTENTION_KEEP_SCORES_BUDGET_BYTES = alive + 1        # nothing fits
    got, names = _launches(ops, train)
    assert names == {"attn_fwd_x6_kernel", "attn_bwd_fused_kernel"}, names
    for name, a, b in zip(("o", "dq", "dk", "dv"), got, (o_ref,) + tuple(g_ref)):
        assert_close(a, b, TOL, name)
    ops.ATTENTION_KEEP_SCORES_BUDGET_BYTES = alive + (1 << 30)   # room again: the shared accounting was not disturbed
    got, names = _launches(ops, train)
    assert names == {"attn_fwd_x6_keep_kernel", "attn_bwd_fused_kernel(kept scores)"}, names
    del got
    assert ops._kept_scores_bytes[0] == alive                    # released with the tensors
