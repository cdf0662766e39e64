"""The AgentAttention kernels of csrc/agent.hip on the MI355X, called through the C ABI (amk_agent_attn_fwd / _bwd /
amk_agent_conv_grad_reduce) and held element by element to the two tiers of tests/agent_ref.py (the hard f32 bound
and 4 x the CPU emulation's q) against the fp64 reference, over the input families, the memory layouts and the shapes
at the edges of the chunking, the agent count and the host dispatch.

Every output (o, dq, dk, dv, agents, vagent, stats1, the convolution gradient's partials, dconv_w, dconv_b) is written
into a NaN canvas between guards; under padded strides and views the padding is part of the canvas (and NaN in the
inputs too, so a read outside a row poisons the result).  Everything a call does not own must be untouched; the
workspaces are sized exactly by amk_agent_ws_floats_dh and sit between guards as well.  No element is left out of a
bound check.  CASES is a plain list built without a GPU: tests/test_agent_bounds.py proves from it that the sweep
reaches every kernel instantiation and every edge (test_paths_cover_dispatch).
AMK_AGENT_BOUNDS_REPORT=<file>: the worst hard ratio and q / limit per output as JSON."""
import contextlib
import ctypes
import json
import os

import pytest
import torch

import agent_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64          # floats before and after every buffer (a multiple of 4: the buffers stay 16-byte aligned)
NAN = float("nan")
FWD_OUT = ("agents", "vagent", "M", "L", "o")
BWD_OUT = ("dq", "dk", "dv", "dconv_w", "dconv_b")


# ---------------------------------------------------------------------------------------------- the case list
def _grid(D):
    """(T, P, H, B, layout): the smallest shapes at which each thing can go wrong, per head dim."""
    CH = ref.chunk_len(D)
    return [
        (1, 1, 1, 2, "separate"),
        (5, 5, 2, 2, "packed"),                 # P == T
        (CH - 1, 4, 3, 2, "view"),
        (CH, 8, 2, 1, "packed"),
        (CH + 1, 6, 2, 2, "bthd_pad"),
        (2 * CH + 1, 7, 3, 2, "packed"),
        (3 * CH, 2, 3, 1, "bthd_pad"),          # P < H
        (2 * CH + 44, 5, 1, 2, "view"),
        (16, 16, 1, 1, "bthd_pad"),             # P == T == MAXP
        (CH + 1, 9, 3, 1, "separate"),
        (2 * CH + 1, 15, 2, 1, "view"),
        (3 * CH, 16, 1, 2, "separate"),         # H 1 with P 16
        (64 * CH + 1, 16 if D == 128 else 5, 1 if D == 128 else 2, 1, "packed"),   # the combine kernel's second pass
    ]


# where the round robin over the families starts (P <= 8, P > 8): chosen so that the 65-chunk cases get large (D 32),
# climb (D 64) and needles (D 128), the families that stress the combine kernel's rescale
_OFFSET = {32: (4, 1), 64: (3, 6), 128: (6, 6)}


def _cases():
    out = []
    for D in (32, 64, 128):
        n = {True: _OFFSET[D][0], False: _OFFSET[D][1]}
        for (T, P, H, B, layout) in _grid(D):
            fam = ref.FAMILIES[n[P <= 8] % len(ref.FAMILIES)]
            n[P <= 8] += 1
            out.append(dict(id=f"d{D}_T{T}_P{P}_H{H}_B{B}_{layout}_{fam}", D=D, T=T, P=P, H=H, B=B, layout=layout, family=fam,
                            both=(D == 64 and P <= 8), seed=len(out) + 1))    # both: also under AMK_AGENT_STREAM=0
    return out


CASES = _cases()


def case_kernels(c):
    ks = ref.expected_kernels(c["D"], c["P"], None)
    return ks | ref.expected_kernels(c["D"], c["P"], "0") if c["both"] else ks


def backward_forms(c):
    """Which forms of the chunk kernels of the backward a case runs."""
    f = {"stream" if c["D"] == 64 and c["P"] <= 8 else "staged"}
    return f | {"staged"} if c["both"] else f


# every family meets every head dim, and both forms of the backward at D = 64
for _D in (32, 64, 128):
    assert {c["family"] for c in CASES if c["D"] == _D} == set(ref.FAMILIES), _D
for _form in ("stream", "staged"):
    assert {c["family"] for c in CASES if c["D"] == 64 and _form in backward_forms(c)} == set(ref.FAMILIES), _form
assert {c["P"] for c in CASES if c["D"] == 64 and c["both"]} >= {1, 4, 5, 6, 8}
for _D in (32, 64, 128):
    assert {c["P"] for c in CASES if c["D"] == _D} >= {1, 2, 4, 5, 6, 7, 8, 9, 15, 16}
    assert {c["H"] for c in CASES if c["D"] == _D} == {1, 2, 3}


# ---------------------------------------------------------------------------------------------- buffers
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def flat(n, dev):
    """(whole, inner): n floats of NaN between GUARD floats of NaN."""
    whole = torch.full((n + 2 * GUARD,), NAN, device=dev)
    return whole, whole[GUARD:GUARD + n]


def guards_untouched(whole):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all())


def layout_specs(layout, n, B, H, T, D):
    """[(floats of one storage, [(offset, (sb, st, sh)) per tensor in it])] for n tensors (B, H, T, D) of a layout:
    packed    one (B, T, n H D) storage, the module's '(qkv h d)' columns
    separate  contiguous (B, H, T, D), one storage each
    bthd_pad  (B, T, H D + 8) storage: a padded row stride
    view      the inner block of a (B, H, T + 3, D + 12) buffer from row 1, column 4 (a 16-byte-aligned offset)"""
    HD = H * D
    if layout == "packed":
        W = n * HD
        return [(B * T * W, [(j * HD, (T * W, W, D)) for j in range(n)])]
    if layout == "separate":
        return [(B * HD * T, [(0, (HD * T, D, T * D))]) for _ in range(n)]
    if layout == "bthd_pad":
        W = HD + 8
        return [(B * T * W, [(0, (T * W, W, D))]) for _ in range(n)]
    if layout == "view":
        W, rows = D + 12, T + 3
        return [(B * H * rows * W, [(W + 4, (H * rows * W, W, rows * W))]) for _ in range(n)]
    raise ValueError(layout)


class Slabs:
    """n tensors (B, H, T, D) of a layout in NaN canvases: .views, .strides ((sb, st, sh) each), .untouched()."""

    def __init__(self, layout, n, B, H, T, D, dev):
        self.shape, self.wholes, self.views, self.strides, self._where = (B, H, T, D), [], [], [], []
        for numel, members in layout_specs(layout, n, B, H, T, D):
            whole = torch.full((numel + 2 * GUARD,), NAN, device=dev)
            self.wholes.append(whole)
            for off, (sb, st, sh) in members:
                assert off % 4 == 0 and off + (B - 1) * sb + (H - 1) * sh + (T - 1) * st + D <= numel    # stays inside
                self.views.append(torch.as_strided(whole, (B, H, T, D), (sb, sh, st, 1), GUARD + off))
                self.strides.append((sb, st, sh))
                self._where.append((len(self.wholes) - 1, GUARD + off, (sb, sh, st, 1)))

    def untouched(self):
        """Everything outside the tensors' own elements is still NaN."""
        masks = [torch.zeros(w.numel(), dtype=torch.bool, device=w.device) for w in self.wholes]
        for i, off, strides in self._where:
            torch.as_strided(masks[i], self.shape, strides, off).fill_(True)
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


def run(inp, P, scale, layout, dev, what=""):
    """Forward, backward and the convolution gradient's reduction through the C ABI, every buffer a guarded NaN
    canvas; asserts that nothing outside the outputs was written.  {name: tensor} for the outputs."""
    from amk import lib as L_

    L = L_.load()
    q, k, v, g, cw, cb = (x.to(dev) for x in inp)
    B, H, T, D = q.shape
    ins = Slabs(layout, 3, B, H, T, D, dev)
    for dst, src in zip(ins.views, (q, k, v)):
        dst.copy_(src)
    gs, os_, ds = Slabs(layout, 1, B, H, T, D, dev), Slabs(layout, 1, B, H, T, D, dev), Slabs(layout, 3, B, H, T, D, dev)
    gs.views[0].copy_(g)
    NC = int(L.amk_agent_num_chunks_dh(T, D))
    cells, rows = B * H * NC, B * H * P
    sizes = {"agents": rows * D, "vagent": rows * D, "stats1": rows * 2, "ws_f": int(L.amk_agent_ws_floats_dh(B, H, T, P, D, 0)),
             "ws_b": int(L.amk_agent_ws_floats_dh(B, H, T, P, D, 1)), "dw_part": cells * 9 * D, "db_part": cells * D,
             "dconv_w": D * 9, "dconv_b": D}
    assert sizes["ws_f"] == ref.ws_floats(B, H, T, P, D, 0) and sizes["ws_b"] == ref.ws_floats(B, H, T, P, D, 1)
    buf = {n: flat(s, dev) for n, s in sizes.items()}
    b = {n: inner for n, (whole, inner) in buf.items()}
    (qv, kv, vv), (ov,), (gv,), (dqv, dkv, dvv) = ins.views, os_.views, gs.views, ds.views
    s3 = lambda strides: [x for s in strides for x in s]
    L_.check(L.amk_agent_attn_fwd(_ptr(qv), _ptr(kv), _ptr(vv), _ptr(cw), _ptr(cb), _ptr(ov), _ptr(b["agents"]), _ptr(b["vagent"]),
                                  _ptr(b["stats1"]), _ptr(b["ws_f"]), B, H, T, D, P, *s3(ins.strides), *os_.strides[0],
                                  float(scale), _stream()), "amk_agent_attn_fwd")
    L_.check(L.amk_agent_attn_bwd(_ptr(qv), _ptr(kv), _ptr(vv), _ptr(cw), _ptr(gv), _ptr(b["agents"]), _ptr(b["vagent"]),
                                  _ptr(b["stats1"]), _ptr(dqv), _ptr(dkv), _ptr(dvv), _ptr(b["ws_b"]), _ptr(b["dw_part"]),
                                  _ptr(b["db_part"]), B, H, T, D, P, *s3(ins.strides), *gs.strides[0], *s3(ds.strides),
                                  float(scale), _stream()), "amk_agent_attn_bwd")
    L_.check(L.amk_agent_conv_grad_reduce(_ptr(b["dw_part"]), _ptr(b["db_part"]), cells, D, _ptr(b["dconv_w"]), _ptr(b["dconv_b"]),
                                          _stream()), "amk_agent_conv_grad_reduce")
    torch.cuda.synchronize()
    assert os_.untouched(), f"{what}: o's canvas was written outside the tensor"
    assert ds.untouched(), f"{what}: the canvas of dq / dk / dv was written outside the tensors"
    for n, (whole, inner) in buf.items():
        assert guards_untouched(whole), f"{what}: a guard of {n} was written"
    st = b["stats1"].view(B, H, P, 2)
    return {"o": ov, "agents": b["agents"].view(B, H, P, D), "vagent": b["vagent"].view(B, H, P, D), "M": st[..., 0], "L": st[..., 1],
            "dq": dqv, "dk": dkv, "dv": dvv, "dconv_w": b["dconv_w"].view(D, 1, 3, 3), "dconv_b": b["dconv_b"],
            "dw_part": b["dw_part"].view(B, H, NC, 9, D), "db_part": b["db_part"].view(B, H, NC, D)}


def case_inputs(c):
    return ref.make_inputs(c["family"], c["B"], c["H"], c["T"], c["D"], c["P"], c["D"] ** -0.5, c["seed"])


def check_all(out, R, what, names=ref.OUTPUTS):
    for n in names:
        ref.assert_within(out[n], R, n, what)


# ---------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_sweep(device, c, stream_env):
    inp = case_inputs(c)
    P, scale = c["P"], c["D"] ** -0.5
    R = ref.reference(*(x.to(device) for x in inp), P, scale)
    assert all(bool(torch.isfinite(R[n]).all()) for n in ref.OUTPUTS), "the family does not give a finite reference"
    what = f"{c['id']} {sorted(backward_forms(c))}"
    with stream_env(None):
        out = run(inp, P, scale, c["layout"], device, what)
    check_all(out, R, what)
    if c["both"]:
        with stream_env("0"):
            out0 = run(inp, P, scale, c["layout"], device, what + " AMK_AGENT_STREAM=0")
        check_all(out0, R, what + " AMK_AGENT_STREAM=0")
        for n in FWD_OUT:
            assert same_bits(out[n], out0[n]), f"{what}: the forward's {n} depends on AMK_AGENT_STREAM"
        for n in BWD_OUT:
            d = (out[n].double() - out0[n].double()).abs().reshape(R[n].shape)
            assert bool((d <= R["bound_" + n]).all()), f"{what}: the two backward forms differ in {n} by more than the bound"


def test_ops_matches_abi(device):
    """ops.agent_attention (the module's packed layout, its own workspaces) equals the ABI call bit for bit."""
    from amk import ops

    B, H, T, D, P = 2, 2, 129, 64, 5
    scale = D ** -0.5
    inp = ref.make_inputs("diffuse", B, H, T, D, P, scale, 77)
    out = run(inp, P, scale, "packed", device, "ops")
    q, k, v, g, cw, cb = (x.to(device) for x in inp)
    bthd = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, H * D)
    qkv2 = torch.cat([bthd(q), bthd(k), bthd(v)], -1).contiguous().requires_grad_(True)
    cw, cb = cw.clone().requires_grad_(True), cb.clone().requires_grad_(True)
    o2 = ops.agent_attention(qkv2, cw, cb, H, D, P, scale)
    o2.backward(bthd(g).contiguous())
    torch.cuda.synchronize()
    assert same_bits(o2, bthd(out["o"]))
    assert same_bits(qkv2.grad, torch.cat([bthd(out["dq"]), bthd(out["dk"]), bthd(out["dv"])], -1))
    assert same_bits(cw.grad, out["dconv_w"]) and same_bits(cb.grad, out["dconv_b"])


# ---------------------------------------------------------------------------------------------- what a tolerance cannot see
# (D, P, AMK_AGENT_STREAM): every form of the chunk kernels
FORMS = [(32, 6, None), (64, 4, None), (64, 5, None), (64, 8, None), (64, 5, "0"), (64, 9, None), (128, 16, None)]
_form_id = lambda f: f"d{f[0]}_P{f[1]}" + ("" if f[2] is None else "_staged")
ALL_OUT = ref.OUTPUTS + ("dw_part", "db_part")


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_bitwise_repeat(device, form, stream_env):
    """No atomics anywhere: two runs give identical bits in every output, the convolution's gradients included."""
    D, P, env = form
    B, H, T = 2, 3, 2 * ref.chunk_len(D) + 1
    inp = ref.make_inputs("diffuse", B, H, T, D, P, D ** -0.5, 31)
    with stream_env(env):
        a = run(inp, P, D ** -0.5, "packed", device)
        b = run(inp, P, D ** -0.5, "bthd_pad", device)        # nor do the bits depend on the layout
    for n in ALL_OUT:
        assert same_bits(a[n], b[n]), f"{_form_id(form)}: {n} differs between two runs"


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_batch_and_head_independence(device, form, stream_env):
    """Nothing in a (b, h) chain depends on B or on the other heads' q and k: element 1 of a batch of 3 equals the
    same element run alone, and head 1's o, dq, dk, dv (its attention part and the convolution of v / dO, which the
    other heads' q and k do not enter) keep their bits when heads 0 and 2 get other q and k."""
    D, P, env = form
    B, H, T = 3, 3, ref.chunk_len(D) + 5
    scale = D ** -0.5
    inp = ref.make_inputs("diffuse", B, H, T, D, P, scale, 41)
    with stream_env(env):
        whole = run(inp, P, scale, "packed", device)
        alone = run(tuple(x[1:2] for x in inp[:4]) + inp[4:], P, scale, "packed", device)
        for n in ("o", "agents", "vagent", "M", "L", "dq", "dk", "dv", "dw_part", "db_part"):
            assert same_bits(whole[n][1:2], alone[n]), f"{_form_id(form)}: {n} of a batch element depends on the batch"
        q2, k2 = inp[0].clone(), inp[1].clone()
        other = ref.make_inputs("diffuse", B, H, T, D, P, scale, 42)
        for h in (0, 2):
            q2[:, h], k2[:, h] = other[0][:, h] * 3, other[1][:, h] * 3
        moved = run((q2, k2) + inp[2:], P, scale, "packed", device)
    for n in ("o", "agents", "vagent", "M", "L", "dq", "dk", "dv"):
        assert same_bits(whole[n][:, 1], moved[n][:, 1]), f"{_form_id(form)}: {n} of head 1 depends on the other heads' q / k"
    assert not same_bits(whole["o"][:, 0], moved["o"][:, 0]) and not same_bits(whole["dk"][:, 2], moved["dk"][:, 2])


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_shift_invariance(device, form, stream_env):
    """A constant vector added to every key of a head shifts every stage-1 score of an agent by the same amount (the
    scalar bias1 the kernels drop): stats1.M moves, everything else stays within the bounds."""
    D, P, env = form
    B, H, T = 1, 2, 2 * ref.chunk_len(D) + 7
    scale = D ** -0.5
    inp = ref.make_inputs("diffuse", B, H, T, D, P, scale, 51)
    shift = torch.randn(D, generator=torch.Generator().manual_seed(52))
    inp2 = (inp[0], inp[1] + shift) + inp[2:]
    R, R2 = (ref.reference(*(x.to(device) for x in i), P, scale) for i in (inp, inp2))
    with stream_env(env):
        a, b = run(inp, P, scale, "separate", device), run(inp2, P, scale, "separate", device)
    check_all(a, R, _form_id(form))
    check_all(b, R2, _form_id(form) + " shifted")
    assert not same_bits(a["M"], b["M"])
    for n in ref.OUTPUTS:
        if n != "M":
            d = (a[n].double() - b[n].double()).abs().reshape(R[n].shape)
            assert bool((d <= R["bound_" + n] + R2["bound_" + n]).all()), f"{_form_id(form)}: {n} moves with a shift of the keys"


@pytest.mark.parametrize("D,P", [(32, 6), (64, 5), (128, 16)])
def test_position_freedom(device, D, P):
    """Rotating whole chunks of k / v leaves V_agent within the bound (a softmax does not know positions) and
    stats1.M bit for bit (a chunk's scores do not depend on the chunk's index, a maximum not on the order)."""
    CH = ref.chunk_len(D)
    B, H, T = 1, 2, 3 * CH
    scale = D ** -0.5
    inp = ref.make_inputs("climb", B, H, T, D, P, scale, 61)
    R = ref.reference(*(x.to(device) for x in inp), P, scale)
    a = run(inp, P, scale, "separate", device)
    b = run((inp[0], torch.roll(inp[1], CH, 2), torch.roll(inp[2], CH, 2)) + inp[3:], P, scale, "separate", device)
    for out, what in ((a, "in place"), (b, "rotated")):
        check_all(out, R, f"position d{D} {what}", ("vagent", "M", "L"))
    assert same_bits(a["M"], b["M"]), "stats1.M depends on the position of the chunks"
    d = (a["vagent"].double() - b["vagent"].double()).abs()
    assert bool((d <= R["bound_vagent"]).all())


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_conv_grad_reduce_alone(device, rows, D):
    """amk_agent_conv_grad_reduce on partials of its own against fp64 column sums, written in the parameter's
    (D, 1, 3, 3) layout; the partials sit exactly between NaN guards (a row too many poisons the sum)."""
    from amk import lib as L_

    L = L_.load()
    g = torch.Generator().manual_seed(rows + D)
    mag = torch.exp2(torch.randint(-8, 9, (rows, 1, 1), generator=g).float())
    wp_, bp_ = torch.randn(rows, 9, D, generator=g) * mag, torch.randn(rows, D, generator=g) * mag[:, 0]
    (ww, wp), (wb, bp), (wo, dw), (wc, db) = flat(rows * 9 * D, device), flat(rows * D, device), flat(9 * D, device), flat(D, device)
    wp.copy_(wp_.reshape(-1))
    bp.copy_(bp_.reshape(-1))
    L_.check(L.amk_agent_conv_grad_reduce(_ptr(wp), _ptr(bp), rows, D, _ptr(dw), _ptr(db), _stream()), "amk_agent_conv_grad_reduce")
    torch.cuda.synchronize()
    R = ref.reduce_reference(wp_.to(device), bp_.to(device))
    ref.assert_within(dw.view(D, 1, 3, 3), R, "dconv_w", f"reduce rows {rows} d{D}", tight=False, key="reduce_w")
    ref.assert_within(db, R, "dconv_b", f"reduce rows {rows} d{D}", tight=False, key="reduce_b")
    assert guards_untouched(wo) and guards_untouched(wc)


@pytest.mark.parametrize("D,P,env", [(32, 8, None), (32, 9, None), (64, 4, None), (64, 5, None), (64, 8, None), (64, 8, "0"),
                                     (64, 9, None), (128, 8, None), (128, 16, None)])
def test_runtime_launches_the_predicted_kernels(device, D, P, env, stream_env):
    """The restatement against the runtime, one case per distinct set of expected_kernels: the agent kernels that the
    profiler reports are exactly the predicted instantiations."""
    from torch.profiler import ProfilerActivity, profile

    inp = ref.make_inputs("diffuse", 1, 2, ref.chunk_len(D) + 3, D, P, D ** -0.5, 71)
    with stream_env(env):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            run(inp, P, D ** -0.5, "packed", device)
            torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    seen = {ref.kernel_id(n) for n in names} - {None}
    assert seen == ref.expected_kernels(D, P, env), (sorted(seen), sorted(n for n in set(names) if "agent" in n))


def test_zz_report(device, capsys):
    """Prints the worst figures of the run (last in the file); AMK_AGENT_BOUNDS_REPORT=<file>: also as JSON."""
    with capsys.disabled():
        print("\noutput: worst hard ratio, worst q / limit")
        for key, (ratio, q) in sorted(ref.WORST.items()):
            print(f"  {key:8s} {ratio:.4f}  {q:.4f}")
    path = os.environ.get("AMK_AGENT_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(ref.WORST, f, indent=1)
