"""The bf16-element AgentAttention kernels on the MI355X (amk_agent_attn_bf16_fwd / _bwd, csrc/agent.hip): bit for bit
the f32 kernels on the upcast tensors with o, dq, dk, dv rounded once; inside agent_ref's bounds and
agent_bf16_ref's intervals against fp64; bitwise repeatable and independent of batch and head; the same through
ops.agent_attention and the AgentAttention module under bf16 autocast, where AMK_AGENT_BF16 changes no bit.

Every output sits in a NaN canvas between guards (bf16 NaN for the bf16 tensors; under padded strides and views the
padding is canvas too, and NaN in the inputs), workspaces are sized exactly by amk_agent_bf16_ws_floats, and everything
a call does not own must be untouched.  No element is left out of a check."""
import contextlib
import ctypes

import pytest
import torch

import agent_bf16_ref as bref
import agent_ref as ref
import test_agent_bounds_gpu as f32sweep       # the f32 entry points' guarded runner

pytestmark = pytest.mark.gpu

GUARD = 64          # elements before and after every buffer (a multiple of 8: the buffers stay 16-byte aligned)
NAN = float("nan")
BF16 = torch.bfloat16
SAME_F32 = ("agents", "vagent", "M", "L", "dw_part", "db_part", "dconv_w", "dconv_b")    # bitwise the f32 path's


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    as_int = torch.int16 if a.dtype == BF16 else torch.int32
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def flat(n, dev):
    whole = torch.full((n + 2 * GUARD,), NAN, device=dev)
    return whole, whole[GUARD:GUARD + n]


def guards_untouched(whole):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all())


def layout_specs(layout, n, B, H, T, D):
    """[(elements of one storage, [(offset, (sb, st, sh)) per tensor in it])] for n bf16 tensors (B, H, T, D):
    packed    one (B, T, n H D) storage, the module's '(qkv h d)' columns
    separate  contiguous (B, H, T, D), one storage each
    padded    (B, H, T, D + 8) storage: rows of D + 8 elements
    view      the inner block of a (B, H, T + 3, D + 16) buffer from row 1, column 8 (a 16-byte-aligned offset)"""
    HD = H * D
    if layout == "packed":
        W = n * HD
        return [(B * T * W, [(j * HD, (T * W, W, D)) for j in range(n)])]
    if layout == "separate":
        return [(B * HD * T, [(0, (HD * T, D, T * D))]) for _ in range(n)]
    if layout == "padded":
        W = D + 8
        return [(B * H * T * W, [(0, (H * T * W, W, T * W))]) for _ in range(n)]
    if layout == "view":
        W, rows = D + 16, T + 3
        return [(B * H * rows * W, [(W + 8, (H * rows * W, W, rows * W))]) for _ in range(n)]
    raise ValueError(layout)


class Slabs:
    """n bf16 tensors (B, H, T, D) of a layout in NaN canvases: .views, .strides ((sb, st, sh) each), .untouched()."""

    def __init__(self, layout, n, B, H, T, D, dev):
        self.shape, self.wholes, self.views, self.strides, self._where = (B, H, T, D), [], [], [], []
        for numel, members in layout_specs(layout, n, B, H, T, D):
            whole = torch.full((numel + 2 * GUARD,), NAN, device=dev, dtype=BF16)
            self.wholes.append(whole)
            for off, (sb, st, sh) in members:
                assert off % 8 == 0 and min(sb, st, sh) % 8 == 0
                assert off + (B - 1) * sb + (H - 1) * sh + (T - 1) * st + D <= numel                 # stays inside
                self.views.append(torch.as_strided(whole, (B, H, T, D), (sb, sh, st, 1), GUARD + off))
                self.strides.append((sb, st, sh))
                self._where.append((len(self.wholes) - 1, GUARD + off, (sb, sh, st, 1)))

    def untouched(self, head=None):
        """Everything outside the tensors' own elements (of head `head` alone, if given) is still NaN."""
        masks = [torch.zeros(w.numel(), dtype=torch.bool, device=w.device) for w in self.wholes]
        for i, off, strides in self._where:
            m = torch.as_strided(masks[i], self.shape, strides, off)
            (m if head is None else m[:, head:head + 1]).fill_(True)
        return all(bool(torch.isnan(w[~m]).all()) for w, m in zip(self.wholes, masks))


@pytest.fixture
def stream_env(monkeypatch):
    @contextlib.contextmanager
    def ctx(value):
        with monkeypatch.context() as m:
            if value is None:
                m.delenv("AMK_AGENT_STREAM", raising=False)
            else:
                m.setenv("AMK_AGENT_STREAM", value)      # read per call by the host code
            yield
    return ctx


def run(inp, P, scale, layout, dev, what="", head=None):
    """Forward, backward and the convolution gradient's reduction through the bf16 entry points, every buffer a guarded
    NaN canvas; asserts that nothing outside the outputs was written.  head: the call covers that head alone (H = 1)
    of the same buffers, with the full call's strides.  {name: tensor} for the outputs (of the heads the call covers)."""
    from amk import lib as L_

    L = L_.load()
    q, k, v, g, cw, cb = (x.to(dev) for x in inp)
    B, H, T, D = q.shape
    ins = Slabs(layout, 3, B, H, T, D, dev)
    for dst, src in zip(ins.views, (q, k, v)):
        dst.copy_(src)                                       # bf16-valued f32 -> bf16: exact
    gs, os_, ds = Slabs(layout, 1, B, H, T, D, dev), Slabs(layout, 1, B, H, T, D, dev), Slabs(layout, 3, B, H, T, D, dev)
    gs.views[0].copy_(g)
    sel = (lambda x: x) if head is None else (lambda x: x[:, head:head + 1])
    Hc = H if head is None else 1
    NC = int(L.amk_agent_num_chunks_dh(T, D))
    cells, rows = B * Hc * NC, B * Hc * P
    sizes = {"agents": rows * D, "vagent": rows * D, "stats1": rows * 2, "ws_f": int(L.amk_agent_bf16_ws_floats(B, Hc, T, P, D, 0)),
             "ws_b": int(L.amk_agent_bf16_ws_floats(B, Hc, T, P, D, 1)), "dw_part": cells * 9 * D, "db_part": cells * D,
             "dconv_w": D * 9, "dconv_b": D}
    assert sizes["ws_f"] == bref.ws_floats(B, Hc, T, P, D, 0) and sizes["ws_b"] == bref.ws_floats(B, Hc, T, P, D, 1)
    buf = {n: flat(s, dev) for n, s in sizes.items()}
    b = {n: inner for n, (whole, inner) in buf.items()}
    (qv, kv, vv), (ov,), (gv,), (dqv, dkv, dvv) = (tuple(sel(x) for x in s.views) for s in (ins, os_, gs, ds))
    s3 = lambda strides: [x for s in strides for x in s]
    L_.check(L.amk_agent_attn_bf16_fwd(_ptr(qv), _ptr(kv), _ptr(vv), _ptr(cw), _ptr(cb), _ptr(ov), _ptr(b["agents"]),
                                       _ptr(b["vagent"]), _ptr(b["stats1"]), _ptr(b["ws_f"]), B, Hc, T, D, P, *s3(ins.strides),
                                       *os_.strides[0], float(scale), _stream()), "amk_agent_attn_bf16_fwd")
    L_.check(L.amk_agent_attn_bf16_bwd(_ptr(qv), _ptr(kv), _ptr(vv), _ptr(cw), _ptr(gv), _ptr(b["agents"]), _ptr(b["vagent"]),
                                       _ptr(b["stats1"]), _ptr(dqv), _ptr(dkv), _ptr(dvv), _ptr(b["ws_b"]), _ptr(b["dw_part"]),
                                       _ptr(b["db_part"]), B, Hc, T, D, P, *s3(ins.strides), *gs.strides[0], *s3(ds.strides),
                                       float(scale), _stream()), "amk_agent_attn_bf16_bwd")
    L_.check(L.amk_agent_conv_grad_reduce(_ptr(b["dw_part"]), _ptr(b["db_part"]), cells, D, _ptr(b["dconv_w"]), _ptr(b["dconv_b"]),
                                          _stream()), "amk_agent_conv_grad_reduce")
    torch.cuda.synchronize()
    assert os_.untouched(head), f"{what}: o's canvas was written outside the tensor"
    assert ds.untouched(head), f"{what}: the canvas of dq / dk / dv was written outside the tensors"
    for n, (whole, inner) in buf.items():
        assert guards_untouched(whole), f"{what}: a guard of {n} was written"
    st = b["stats1"].view(B, Hc, P, 2)
    out = {"o": ov, "agents": b["agents"].view(B, Hc, P, D), "vagent": b["vagent"].view(B, Hc, P, D), "M": st[..., 0], "L": st[..., 1],
           "dq": dqv, "dk": dkv, "dv": dvv, "dconv_w": b["dconv_w"].view(D, 1, 3, 3), "dconv_b": b["dconv_b"],
           "dw_part": b["dw_part"].view(B, Hc, NC, 9, D), "db_part": b["db_part"].view(B, Hc, NC, D)}
    for n in bref.ROUNDED:
        assert out[n].dtype == BF16
    return out


def envs(c):
    return (None, "0") if c["both"] else (None,)


# ---------------------------------------------------------------------------------------------- 1. to the bit against the f32 kernels
@pytest.mark.parametrize("c", bref.CASES, ids=lambda c: c["id"])
def test_bits_of_the_f32_kernels(device, c, stream_env):
    """A derived condition, not a tolerance: same arithmetic in the same order, so the f32 outputs are bitwise those of
    amk_agent_attn_fwd / _bwd on the exact f32 upcast, and o, dq, dk, dv are those kernels' f32 results rounded once."""
    inp = bref.case_inputs(c)
    P, scale = c["P"], c["D"] ** -0.5
    for env in envs(c):
        what = f"{c['id']} AMK_AGENT_STREAM={env}"
        with stream_env(env):
            out = run(inp, P, scale, c["layout"], device, what)
            f32 = f32sweep.run(inp, P, scale, "packed", device, what + " f32")
        for n in SAME_F32:
            assert same_bits(out[n], f32[n]), f"{what}: {n} differs from the f32 kernels'"
        for n in bref.ROUNDED:
            assert bool(torch.isfinite(f32[n]).all())
            want = f32[n].contiguous().to(BF16)
            assert torch.equal(want.double(), bref.bf16_rne(f32[n].contiguous().double())), "torch's conversion is not RNE here"
            assert same_bits(out[n].contiguous(), want), f"{what}: {n} is not the f32 kernels' result rounded to nearest even"


# ---------------------------------------------------------------------------------------------- 2. against fp64
@pytest.mark.parametrize("c", bref.CASES, ids=lambda c: c["id"])
def test_against_fp64(device, c, stream_env):
    inp = bref.case_inputs(c)
    P, scale = c["P"], c["D"] ** -0.5
    R = bref.reference(*(x.to(device) for x in inp), P, scale)
    assert all(bool(torch.isfinite(R[n]).all()) for n in ref.OUTPUTS), "the family does not give a finite reference"
    for env in envs(c):
        what = f"{c['id']} AMK_AGENT_STREAM={env}"
        with stream_env(env):
            out = run(inp, P, scale, c["layout"], device, what)
        for n in bref.F32_OUT:
            ref.assert_within(out[n], R, n, what, key="bf16path_" + n)
        for n in bref.ROUNDED:
            bref.assert_rounded_within(out[n], R, n, what)


# ---------------------------------------------------------------------------------------------- 3. what a tolerance cannot see
# (D, P, AMK_AGENT_STREAM): both forms of the chunk kernels of the backward (streaming, LDS-staged) and every head dim
FORMS = [(32, 6, None), (64, 5, None), (64, 5, "0"), (64, 9, None), (128, 16, None)]
_form_id = lambda f: f"d{f[0]}_P{f[1]}" + ("" if f[2] is None else "_staged")
ALL_OUT = ref.OUTPUTS + ("dw_part", "db_part")


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_bitwise_repeat(device, form, stream_env):
    """Two runs give identical bits in every output, and the bits do not depend on the layout."""
    D, P, env = form
    B, H, T = 2, 3, 2 * ref.chunk_len(D) + 1
    inp = bref.make_inputs("diffuse", B, H, T, D, P, D ** -0.5, 31)
    with stream_env(env):
        a = run(inp, P, D ** -0.5, "packed", device)
        b = run(inp, P, D ** -0.5, "packed", device)
        c = run(inp, P, D ** -0.5, "view", device)
    for n in ALL_OUT:
        assert same_bits(a[n], b[n]), f"{_form_id(form)}: {n} differs between two runs"
        assert same_bits(a[n], c[n]), f"{_form_id(form)}: {n} depends on the layout"


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_batch_element_alone(device, form, stream_env):
    D, P, env = form
    B, H, T = 3, 3, ref.chunk_len(D) + 5
    inp = bref.make_inputs("diffuse", B, H, T, D, P, D ** -0.5, 41)
    with stream_env(env):
        whole = run(inp, P, D ** -0.5, "packed", device)
        alone = run(tuple(x[1:2] for x in inp[:4]) + inp[4:], P, D ** -0.5, "packed", device)
    for n in ("o", "agents", "vagent", "M", "L", "dq", "dk", "dv", "dw_part", "db_part"):
        assert same_bits(whole[n][1:2], alone[n]), f"{_form_id(form)}: {n} of a batch element depends on the batch"


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("layout", ["packed", "padded"])
def test_head_alone_with_the_full_strides(device, form, layout, stream_env):
    """Head 1 of three, called as a one-head tensor at the full call's strides (the f32 dq workspace is contiguous
    whatever those are): with a zero convolution weight (family conv_zero: the only coupling between heads) its o, dq,
    dk, dv, agents, vagent and stats1 keep their bits, and the other heads' rows of the canvases stay untouched."""
    D, P, env = form
    B, H, T = 2, 3, ref.chunk_len(D) + 5
    inp = bref.make_inputs("conv_zero", B, H, T, D, P, D ** -0.5, 43)
    with stream_env(env):
        whole = run(inp, P, D ** -0.5, layout, device)
        alone = run(inp, P, D ** -0.5, layout, device, head=1)
    for n in ("o", "agents", "vagent", "M", "L", "dq", "dk", "dv"):
        assert same_bits(whole[n][:, 1:2], alone[n]), f"{_form_id(form)}: {n} of head 1 depends on the call's other heads"


# ---------------------------------------------------------------------------------------------- 4. ops.agent_attention under autocast
def _agent_kernels(prof):
    return {ref.kernel_id(e.name) for e in prof.events()} - {None}


def _ops_call(ops, qkv2, cw, cb, H, D, P, scale, g2, autocast):
    from torch.profiler import ProfilerActivity, profile

    qkv2 = qkv2.detach().clone().requires_grad_(True)
    cw, cb = cw.detach().clone().requires_grad_(True), cb.detach().clone().requires_grad_(True)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with (torch.autocast("cuda", autocast) if autocast is not None else contextlib.nullcontext()):
            o2 = ops.agent_attention(qkv2, cw, cb, H, D, P, scale)
        o2.backward(g2.to(o2.dtype))
        torch.cuda.synchronize()
    return o2, qkv2.grad, cw.grad, cb.grad, _agent_kernels(prof)


@pytest.mark.parametrize("D,P,env", [(64, 5, None), (64, 5, "0"), (32, 9, None), (128, 3, None)])
def test_ops_under_autocast(device, D, P, env, stream_env, monkeypatch):
    from amk import ops

    B, H, T = 2, 2, ref.chunk_len(D) + 1
    scale = D ** -0.5
    inp = bref.make_inputs("diffuse", B, H, T, D, P, scale, 77)
    q, k, v, g, cw, cb = (x.to(device) for x in inp)
    bthd = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, H * D)
    qkv_f32 = torch.cat([bthd(q), bthd(k), bthd(v)], -1).contiguous()
    g2 = bthd(g).contiguous()
    with stream_env(env):
        out = run(inp, P, scale, "packed", device, "ops")
        o2, dqkv, dcw, dcb, seen = _ops_call(ops, qkv_f32.to(BF16), cw, cb, H, D, P, scale, g2, BF16)
        assert o2.dtype == BF16 and dqkv.dtype == BF16 and dcw.dtype == torch.float32 and dcb.dtype == torch.float32
        assert same_bits(o2, bthd(out["o"]).contiguous())
        assert same_bits(dqkv, torch.cat([bthd(out["dq"]), bthd(out["dk"]), bthd(out["dv"])], -1).contiguous())
        assert same_bits(dcw, out["dconv_w"]) and same_bits(dcb, out["dconv_b"])
        assert seen == bref.expected_kernels(D, P, env), sorted(seen)
        # every other call runs today's f32 kernels
        want = ref.expected_kernels(D, P, env)
        with monkeypatch.context() as m:
            m.setattr(ops, "AGENT_BF16", False)
            o3, dqkv3, dcw3, dcb3, seen = _ops_call(ops, qkv_f32.to(BF16), cw, cb, H, D, P, scale, g2, BF16)
        assert seen == want, sorted(seen)
        # (the switch changes no bit: o rounded here, where W_o's input cast rounds it in a module)
        assert o3.dtype == torch.float32 and same_bits(o3.to(BF16), o2) and same_bits(dqkv3, dqkv)
        assert same_bits(dcw3, dcw) and same_bits(dcb3, dcb)
        assert _ops_call(ops, qkv_f32, cw, cb, H, D, P, scale, g2, BF16)[4] == want                       # f32 qkv under autocast
        assert _ops_call(ops, qkv_f32.half(), cw, cb, H, D, P, scale, g2, torch.float16)[4] == want       # f16 autocast
        assert _ops_call(ops, qkv_f32, cw, cb, H, D, P, scale, g2, None)[4] == want                       # no autocast
    with pytest.raises(RuntimeError, match="fp32"):
        ops.agent_attention(qkv_f32.to(BF16), cw, cb, H, D, P, scale)                                     # bf16 outside autocast


# ---------------------------------------------------------------------------------------------- 5. the module
@pytest.mark.parametrize("dim,heads,d,agent_num", [(192, 3, 32, 9), (192, 3, 64, 9), (192, 3, 128, 9), (384, 6, 64, 47)])
def test_module_switch_changes_no_bit(device, dim, heads, d, agent_num, monkeypatch):
    """AgentAttention forward + backward under bf16 autocast with the switch on and off: the rounding points coincide
    (o at W_o's input, dqkv at the projection's backward), so the output, x.grad and every parameter gradient are equal
    bit for bit."""
    from amk import ops
    from amk.models import AgentAttention

    torch.manual_seed(5)
    mod = AgentAttention(dim, heads, d, agent_num=agent_num).to(device)
    x0 = torch.randn(2, 300, dim, device=device)
    cot = torch.randn(2, 300, dim, device=device)

    def step(on):
        from torch.profiler import ProfilerActivity, profile

        with monkeypatch.context() as m:
            m.setattr(ops, "AGENT_BF16", on)
            mod.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                with torch.autocast("cuda", BF16):
                    y = mod(x)
                y.backward(cot.to(y.dtype))
                torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}
        return y.detach().clone(), x.grad.clone(), grads, _agent_kernels(prof)

    y1, gx1, g1, seen1 = step(True)
    y0, gx0, g0, seen0 = step(False)
    assert seen1 == bref.expected_kernels(d, heads) and seen0 == ref.expected_kernels(d, heads), (sorted(seen1), sorted(seen0))
    assert same_bits(y1, y0) and same_bits(gx1, gx0)
    assert set(g1) == set(g0) and {"qkv.weight", "W_o.weight", "W_o.bias", "dwc.1.weight", "dwc.1.bias"} <= set(g1)
    for n in g1:
        assert same_bits(g1[n], g0[n]), f"{n}.grad depends on AMK_AGENT_BF16"
    assert bool(torch.isfinite(y1).all()) and float(gx1.abs().max()) > 0


def test_zz_report(device, capsys):
    """Prints the worst figures of the run (last in the file)."""
    with capsys.disabled():
        print("\nf32 outputs of the bf16 path: worst hard ratio, worst q / limit")
        for key, (ratio, q) in sorted(ref.WORST.items()):
            if key.startswith("bf16path_"):
                print(f"  {key[9:]:8s} {ratio:.4f}  {q:.4f}")
        print("bf16 outputs: worst position inside the interval")
        for key, pos in sorted(bref.WORST.items()):
            print(f"  {key:8s} {pos:.4f}")
