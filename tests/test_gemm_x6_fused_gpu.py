"""The fused forms of the split-bf16 GEMM on ready planes (csrc/gemm_x6.hip: amk_gemm_x6_nt2, amk_gemm_x6_nt_swiglu,
amk_gemm_x6_nt_swiglu_bwd, planes from amk_gemm_x6_split_table) against fp64 under the per-element bounds of
tests/gemm_x6_ref.py, at the smallest shapes where each can go wrong: the row-tile edge (M = 1, 127, 129, 333), widths 4,
68, 132 (an a / b pair across a 128-row plane tile) and 200, contractions 4, 36, 52 and 256 (tail of the 32-step, padding),
two segments 32 + 36, a strided A.  Then the autograd Functions ops puts on them, against fp64 autograd."""
import pytest
import torch

import dense_f32_ref as R32
import gemm_x6_ref as ref

pytestmark = pytest.mark.gpu

MS = (1, 127, 129, 333)
NK = ((4, 4), (68, 36), (132, 52), (200, 256))   # (width, contraction)


def make_planes(device, weights, gates=()):
    """[X6Planes] of CPU f32 matrices by ONE table-driven split (the weights laid out in one flat buffer at 256-element
    boundaries, as amk.dp lays parameters out)."""
    from amk import dense

    ent, off = [], 0
    for i, w in enumerate(weights):
        ent.append((off, w.shape[0], w.shape[1], i in gates))
        off += -(-w.numel() // 256) * 256
    flat = torch.zeros(off, device=device)
    for (o, R, K, _), w in zip(ent, weights):
        flat[o:o + R * K] = w.reshape(-1).to(device)
    table, nblk, elems, spans = dense.x6_split_plan(ent)
    buf = torch.zeros(elems, device=device, dtype=torch.bfloat16)
    dense.x6_split_table(flat, table.to(device), nblk, buf)
    return [dense.X6Planes(buf[dw:dw + nw], buf[dt:dt + nt], g, R, K) for (_, R, K, g), (dw, nw, dt, nt) in zip(ent, spans)]


split_ref = ref.split_planes_gpu


def check(got, want, bound, what):
    nbad, ratio = ref.worst_ratio(got, want.to(got.device), bound.to(got.device))
    print(f"{what}: worst |err| / bound = {ratio:.3f}")
    assert nbad == 0, f"{what}: {nbad} elements outside the bound, worst ratio {ratio:.3f}"


def dev(D, device):
    return {k: v.to(device) for k, v in D.items()}


def test_split_table_equals_split_bit_for_bit(device):
    g = torch.Generator().manual_seed(5)
    shapes = [(68, 36), (4, 4), (200, 52), (264, 256), (136, 36), (8, 4)]
    gates = (3, 4, 5)   # H = 132 (an a / b pair across plane tiles), 68, 4
    ws = [torch.randn(s, generator=g) * 2.0 ** torch.randint(-6, 7, s, generator=g).float() for s in shapes]
    pls = make_planes(device, ws, gates)
    for i, (w, pl) in enumerate(zip(ws, pls)):
        wd = w.to(device)
        R, K = w.shape
        want_t = split_ref(wd.t().contiguous())
        assert torch.equal(pl.wt.view(3, K, ref.pad32(R)).view(torch.int16), want_t.view(torch.int16)), f"W^T planes of {i}"
        want = split_ref(wd)
        if i in gates:
            _, rows = ref.gate_order(w)
            got = pl.w.view(3, -1, ref.pad32(K))
            assert got.shape[1] == 128 * -(-(R // 2) // 64)
            assert torch.equal(got[:, rows.to(device)].view(torch.int16), want.view(torch.int16)), f"gate-order planes of {i}"
            pad = torch.ones(got.shape[1], dtype=torch.bool, device=device)
            pad[rows.to(device)] = False
            assert not got[:, pad].float().any(), "padding rows of the gate order must be zero"
        else:
            assert torch.equal(pl.w.view(3, R, ref.pad32(K)).view(torch.int16), want.view(torch.int16)), f"W planes of {i}"


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", NK)
def test_nt_and_input_gradient_on_table_planes(device, M, N, K):
    """NT (+ bias) against the W planes and dX = dY W against the W^T planes of the same table-driven split."""
    from amk import dense

    for family in ref.FAMILIES:
        D = dev(R32.make_nt(family, M, N, K, 21), device)
        (pl,) = make_planes(device, [D["w"].cpu()])
        for bias in (None, D["bias"]):
            want, bound = ref.ref_nt(D["a"], D["w"], bias)
            check(dense.gemm_x6_nt(D["a"], pl.w, N, bias), want, bound, f"nt {family} bias={bias is not None}")
        dy = R32.make_act(family, M, N, 22).to(device)
        wt = D["w"].t().contiguous()
        want, bound = ref.ref_nt(dy, wt)
        check(dense.gemm_x6_nt(dy, pl.wt, K), want, bound, f"dX {family}")


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", (4, 68, 132, 200))
def test_two_segment_input_gradient(device, M, N):
    from amk import dense

    for family in ref.FAMILIES:
        D = dev(R32.make_nn(family, M, N, 32, 23, K2=36), device)    # w (32, N), w2 (36, N): dX = a w + a2 w2
        pa, pb = make_planes(device, [D["w"].cpu(), D["w2"].cpu()])
        want, bound = ref.ref_nt(D["a"], D["w"].t(), None, D["a2"], D["w2"].t())
        check(dense.gemm_x6_nt(D["a"], pa.wt, N, a2=D["a2"], planes2=pb.wt), want, bound, f"nt2 {family}")


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,K", NK)
def test_swiglu_forward(device, M, H, K):
    from amk import dense

    for family in ref.FAMILIES:
        D = dev(R32.make_swiglu(family, M, H, K, 24), device)
        (pl,) = make_planes(device, [D["w"].cpu()], gates=(0,))
        g, gb, ab, abb = ref.ref_nt_swiglu(D["a"], D["w"], D["bias"])
        gate, kept = dense.gemm_x6_nt_swiglu(D["a"], pl.w, H, D["bias"], keep_ab=True)
        check(gate, g, gb, f"gate {family}")
        check(kept, ab, abb, f"(a | b) {family}")
        only, none = dense.gemm_x6_nt_swiglu(D["a"], pl.w, H, D["bias"], keep_ab=False)
        assert none is None and torch.equal(only, gate), "the gate must not depend on keep_ab"
        g0, gb0, _, _ = ref.ref_nt_swiglu(D["a"], D["w"], None)
        check(dense.gemm_x6_nt_swiglu(D["a"], pl.w, H, None, keep_ab=False)[0], g0, gb0, f"gate without bias {family}")


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,K", NK)
def test_swiglu_backward(device, M, H, K):
    from amk import dense

    for family in ref.FAMILIES:
        D = dev(R32.make_swiglu_bwd(family, M, H, K, 25), device)   # dy (M, K), w3 (K, H), ab (M, 2H)
        (pl,) = make_planes(device, [D["w3"].cpu()])
        want, bound = ref.ref_nt_swiglu_bwd(D["dy"], D["w3"].t().contiguous(), D["ab"])
        check(dense.gemm_x6_nt_swiglu_bwd(D["dy"], pl.wt, D["ab"]), want, bound, f"(dA | dB) {family}")


def test_strided_rows(device):
    """A as a column slice of a wider buffer (the q / kv views), in every form that reads an A."""
    from amk import dense

    D = dev(R32.make_swiglu("unit", 129, 68, 36, 26), device)
    wide = torch.randn(129, 100, device=device)
    wide[:, 8:44] = D["a"]
    a = wide[:, 8:44]
    assert a.stride(0) == 100 and a.data_ptr() % 16 == 0
    plg, pln = make_planes(device, [D["w"].cpu(), D["w"].cpu()], gates=(0,))
    assert torch.equal(dense.gemm_x6_nt(a, pln.w, 136, D["bias"]), dense.gemm_x6_nt(D["a"], pln.w, 136, D["bias"]))
    assert torch.equal(dense.gemm_x6_nt_swiglu(a, plg.w, 68, D["bias"])[0], dense.gemm_x6_nt_swiglu(D["a"], plg.w, 68, D["bias"])[0])
    a2 = torch.randn(129, 136, device=device)
    both = torch.cat([a2, D["a"]], 1)      # (129, 172): two row-strided segments of one buffer
    w2 = torch.randn(136, 200).mul(0.1)
    w1 = torch.randn(36, 200).mul(0.1)
    p2, p1 = make_planes(device, [w2, w1])
    got = dense.gemm_x6_nt(both[:, :136], p2.wt, 200, a2=both[:, 136:], planes2=p1.wt)
    want, bound = ref.ref_nt(a2, w2.t().to(device), None, D["a"], w1.t().to(device))
    check(got, want, bound, "two strided segments")


def _with_planes(device, *weights, gate=None, transposed=True):
    pls = make_planes(device, [w.detach().cpu() for w in weights], gates=tuple(i for i, w in enumerate(weights) if w is gate))
    for w, pl in zip(weights, pls):
        if not transposed:
            pl.wt = None      # forward products only: the backward then takes the f32 input-gradient kernels
        w._amk_x6, w._amk_x6_version = pl, w._version
    return pls


@pytest.mark.parametrize("transposed", [True, False])
def test_functions_against_fp64_autograd(device, transposed):
    """ops.linear / linear2 / swiglu_ffn take the x6 Functions when the weights carry current planes, and every output and
    gradient agrees with fp64 autograd at the f32 level; without planes the same calls take the f32 paths."""
    from amk import ops
    from util import assert_close

    old = ops.GEMM_MODE, ops.X6_LINEAR
    ops.GEMM_MODE, ops.X6_LINEAR = "auto", True
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)
    M, Dm, H = 200, 132, 68
    x = r(2, M // 2, Dm).to(device).requires_grad_(True)
    P = {k: v.to(device).requires_grad_(True) for k, v in dict(
        w=r(132, Dm) * 0.2, b=r(132), wa=r(128, Dm) * 0.2, wb=r(256, Dm) * 0.2, w12=r(2 * H, Dm) * 0.2, b12=r(2 * H) * 0.1,
        w3=r(Dm, H) * 0.2, b3=r(Dm)).items()}

    def run(x, P, lin, lin2, ffn):
        y = lin(x, P["w"], P["b"])
        q, kv = lin2(x, P["wa"], P["wb"])
        f = ffn(x, P["w12"], P["b12"], P["w3"], P["b3"])
        loss = y.pow(2).sum() + (q.sum(-1, keepdim=True) * kv).pow(2).sum() * 1e-3 + f.pow(2).sum()
        names = sorted(P)
        return [y, q, kv, f] + list(torch.autograd.grad(loss, [x] + [P[n] for n in names])), ["y", "q", "kv", "f", "dx"] + names

    def ffn64(x, w12, b12, w3, b3):
        a, b = torch.nn.functional.linear(x, w12, b12).chunk(2, -1)
        return torch.nn.functional.linear(torch.nn.functional.silu(a) * b, w3, b3)

    F = torch.nn.functional
    want, names = run(x.detach().double().requires_grad_(True), {k: v.detach().double().requires_grad_(True) for k, v in P.items()},
                      F.linear, lambda x, a, b: (F.linear(x, a), F.linear(x, b)), ffn64)
    seen = []
    orig = ops._x6_planes
    ops._x6_planes = lambda kind, *a, **k: (seen.append((kind, orig(kind, *a, **k) is not None)), orig(kind, *a, **k))[1]
    try:
        plain, _ = run(x, P, ops.linear, ops.linear2, ops.swiglu_ffn)
        assert seen and not any(ok for _, ok in seen)
        _with_planes(device, P["w"], P["wa"], P["wb"], P["w3"], transposed=transposed)
        _with_planes(device, P["w12"], gate=P["w12"], transposed=transposed)
        del seen[:]
        got, _ = run(x, P, ops.linear, ops.linear2, ops.swiglu_ffn)
        assert seen == [("linear", True), ("linear2", True), ("ffn", True)]
        with torch.no_grad():
            P["w"].mul_(1.0)       # an in-place write: the planes of w are no longer trusted
        assert ops._x6_planes("linear", x, P["w"]) is None and ops._x6_planes("linear2", x, P["wa"], P["wb"]) is not None
    finally:
        ops._x6_planes = orig
        ops.GEMM_MODE, ops.X6_LINEAR = old
    for n, a, b, c in zip(names, got, want, plain):
        assert_close(a, b, 3e-6, n)
        assert_close(c, b, 3e-6, n + " (f32 path)")
