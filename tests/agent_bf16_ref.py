"""The bf16-element form of the AgentAttention kernels (csrc/agent.hip, amk_agent_attn_bf16_fwd / _bwd) against
tests/agent_ref.py: inputs, reference, the interval a rounded output must lie in, the case grid, a restatement of the
host code and an emulation with the defects a bf16 path can have.

The bf16 kernels are the f32 kernels on another element type: q, k, v, d_o are bf16 and widen exactly on the load, the
arithmetic is the f32 chain in the same order, o, dq, dk, dv are rounded to nearest even once, on the store; agents,
vagent, stats1, the convolution's parameters and gradients stay f32.  So
* the inputs are agent_ref.make_inputs with q, k, v, d_o rounded to bf16 values (make_inputs), the reference is
  agent_ref.reference on those values, and the f32 outputs are held to both tiers of agent_ref unchanged;
* a bf16 output x = rne(y), y the f32 result with |y - ref| <= b, lies in [rne(ref - b), rne(ref + b)] because
  rounding is monotonic (interval); b = min(hard bound, ftz + 4 Q u32 S), the smaller of agent_ref's two tiers.  The
  interval adds nothing for the rounding itself: a second rounding, a truncation or a rounded intermediate moves an
  element out of it wherever b is below the spacing of bf16, which is the case at almost every element (b is a few
  u32 of the magnitudes, a bf16 ulp is 2^17 u32 of the value).
Q is agent_ref.Q_EMU where the emulation stays below it on these inputs too: tests/test_agent_bf16_bounds.py::
test_emulation runs agent_ref.emulate over the bf16-valued inputs of every case of the grid; its worst q per output is
    agents 0.212   vagent 1.74   M 0.776   L 0.686   o 1.14   dq 0.988   dk 1.13   dv 1.94   dconv_w 0.850   dconv_b 0.289
against Q_EMU's 1.73, 1.9, 0.685, 0.658, 1.48, 1.18, 2.02, 1.57, 0.912, 0.965.  M, L and dv exceed it (other seeds, and
the view layout's conv_binade case at D = 32 for dv), so Q_EMU_BF16 carries this emulation's figures for them, rounded
up by less than a quarter -- never a figure from the GPU.  dv's enters the interval; the f32 outputs M and L are held
by agent_ref.assert_within to agent_ref's own, smaller limit, which the kernels meet with room (below).

Defects (emulate_defect, flagged by test_planted_defects on the grid's small cases):
    truncate        o, dq, dk, dv truncated towards zero to bf16 instead of rounded to nearest even
    dq_twice        the stage-2 part of dq rounded to bf16 before the pooled dA / len is added (a bf16 dq tensor used
                    for the read-modify-write of the f32 path), the sum rounded again
    vagent_bf16     vagent rounded to bf16 before stage 2 and the backward read it
    d_o_coarser     dO read from a copy rounded once more, to the next coarser grid (7 significant bits: what is left of
                    a bf16 value after another rounding that loses a bit)

Measured on the MI355X over tests/test_agent_bf16_gpu.py (test_zz_report): f32 outputs hard ratio, q / (4 Q_EMU); bf16
outputs the worst position of an element inside its interval (1 = at its end):
    agents 0.074, 0.026    vagent 0.0049, 0.086    M 0.030, 0.100    L 0.013, 0.143    dconv_w 0.025, 0.233
    dconv_b 0.0019, 0.075  o 1.0   dq 1.0   dk 1.0   dv 1.0
The first run passed on every case, layout and form of the backward: no element outside an interval, every f32 output
and every rounded output bit for bit what the f32 kernels give on the upcast tensors
(an element reaches the end of its interval whenever ref +- b rounds to the same bf16 value as ref does: the interval is
then a single value, and the kernel's element is that value).
"""
import torch

import agent_ref as ref

F64 = torch.float64
ROUNDED = ("o", "dq", "dk", "dv")                                   # bf16 outputs
F32_OUT = tuple(n for n in ref.OUTPUTS if n not in ROUNDED)
Q_EMU_BF16 = {"M": 0.78, "L": 0.69, "dv": 1.94}                     # where this emulation exceeds agent_ref.Q_EMU (docstring)
DEFECTS = ("truncate", "dq_twice", "vagent_bf16", "d_o_coarser")


def q_emu(name):
    return Q_EMU_BF16.get(name, ref.Q_EMU[name])


# ---------------------------------------------------------------------------------------------- bf16 in fp64
def _ulp(v, bits=8):
    """The spacing at each fp64 value of a format with `bits` significant bits and f32's exponent range."""
    _, ex = torch.frexp(v)
    return torch.exp2((ex - 1).clamp(min=-126).to(F64) - (bits - 1))


def _on_grid(v, fn, bits=8):
    u = _ulp(v, bits)
    return torch.where(torch.isfinite(v), fn(v / u) * u, v)


def bf16_rne(v):
    """fp64 -> the nearest bf16 value, ties to even, as fp64 (exact: v / ulp is a scaling by a power of two)."""
    return _on_grid(v.to(F64), torch.round)


def bf16_trunc(v):
    return _on_grid(v.to(F64), torch.trunc)


def bf16_round(x):
    """f32 -> the nearest bf16 value, ties to even, held as f32."""
    return bf16_rne(x).to(torch.float32)


# ---------------------------------------------------------------------------------------------- inputs, reference, interval
def make_inputs(family, B, H, T, D, P, scale, seed):
    """agent_ref.make_inputs with q, k, v, d_o rounded to bf16 values (held as f32); conv_w, conv_b stay f32."""
    q, k, v, g, cw, cb = ref.make_inputs(family, B, H, T, D, P, scale, seed)
    return tuple(bf16_round(x) for x in (q, k, v, g)) + (cw, cb)


def reference(q, k, v, d_o, conv_w, conv_b, P, scale):
    return ref.reference(q, k, v, d_o, conv_w, conv_b, P, scale)


def interval(R, name):
    """(lo, hi) as fp64: the bf16 values a rounded output element must lie between."""
    b = torch.minimum(R["bound_" + name], R["ftz_" + name] + ref.TIGHT_FACTOR * q_emu(name) * ref.U32 * R["S_" + name])
    return bf16_rne(R[name] - b), bf16_rne(R[name] + b)


WORST = {}   # rounded output -> worst position inside the interval over every check of the process


def outside(got, R, name):
    """(number of elements outside the interval, worst position inside it: 0 = the reference's own rounding, 1 = an end)."""
    lo, hi = interval(R, name)
    a = got.detach().to(lo.device, F64).reshape(lo.shape)
    bad = ~((a >= lo) & (a <= hi))
    mid = bf16_rne(R[name])
    pos = torch.where(a > mid, (a - mid) / (hi - mid).clamp_min(1e-300), (mid - a) / (mid - lo).clamp_min(1e-300))
    pos = torch.where(a == mid, torch.zeros_like(pos), pos)
    pos = torch.where(torch.isnan(a), torch.full_like(pos, float("inf")), pos)
    return int(bad.sum()), float(pos.max()) if pos.numel() else 0.0


def assert_rounded_within(got, R, name, what=""):
    nbad, pos = outside(got, R, name)
    WORST[name] = max(WORST.get(name, 0.0), pos)
    print(f"{what} {name}: {nbad} outside the interval, worst position {pos:.4g}")
    assert nbad == 0, f"{what} {name}: {nbad} elements outside [rne(ref - b), rne(ref + b)] (worst position {pos:.3g})"


# ---------------------------------------------------------------------------------------------- the case grid
LAYOUTS = ("packed", "separate", "padded", "view")


def _grid(D):
    """(T, P, H, B, layout): the shapes of tests/test_agent_bounds_gpu.py's grid, restated."""
    CH = ref.chunk_len(D)
    return [
        (1, 1, 1, 2, "separate"),
        (5, 5, 2, 2, "packed"),
        (CH - 1, 4, 3, 2, "view"),
        (CH, 8, 2, 1, "packed"),
        (CH + 1, 6, 2, 2, "padded"),
        (2 * CH + 1, 7, 3, 2, "packed"),
        (3 * CH, 2, 3, 1, "padded"),
        (2 * CH + 44, 5, 1, 2, "view"),
        (16, 16, 1, 1, "padded"),
        (CH + 1, 9, 3, 1, "separate"),
        (2 * CH + 1, 15, 2, 1, "view"),
        (3 * CH, 16, 1, 2, "separate"),
        (64 * CH + 1, 16 if D == 128 else 5, 1 if D == 128 else 2, 1, "packed"),   # the combine kernel's second pass
    ]


# where the round robin over the families starts (P <= 8, P > 8), per head dim
_OFFSET = {32: (4, 1), 64: (3, 6), 128: (6, 6)}


def _cases():
    out = []
    for D in (32, 64, 128):
        n = {True: _OFFSET[D][0], False: _OFFSET[D][1]}
        for (T, P, H, B, layout) in _grid(D):
            fam = ref.FAMILIES[n[P <= 8] % len(ref.FAMILIES)]
            n[P <= 8] += 1
            out.append(dict(id=f"d{D}_T{T}_P{P}_H{H}_B{B}_{layout}_{fam}", D=D, T=T, P=P, H=H, B=B, layout=layout, family=fam,
                            both=(D == 64 and P <= 8), seed=len(out) + 101))   # both: also under AMK_AGENT_STREAM=0
    return out


CASES = _cases()
for _D in (32, 64, 128):
    assert {c["family"] for c in CASES if c["D"] == _D} == set(ref.FAMILIES), _D
    assert {c["layout"] for c in CASES if c["D"] == _D} == set(LAYOUTS), _D


def case_inputs(c):
    return make_inputs(c["family"], c["B"], c["H"], c["T"], c["D"], c["P"], c["D"] ** -0.5, c["seed"])


# ---------------------------------------------------------------------------------------------- host restatement
def ws_floats(B, H, T, P, D, backward):
    """amk_agent_bf16_ws_floats: the f32 path's size, plus the f32 stage-2 part of dq in the backward."""
    n = ref.ws_floats(B, H, T, P, D, backward)
    return n + B * H * T * D if n and backward else n


SHARED = ("agent_s1_combine_kernel", "agent_mid_kernel", "agent_conv_reduce_kernel")   # f32 workspaces only: both paths


def expected_kernels(D, P, stream_env=None):
    """agent_ref.expected_kernels for the bf16 entry points: every kernel that touches a bf16 tensor is the
    agent_*_bf16_kernel instantiation, the three shared ones keep their names."""
    out = set()
    for k in ref.expected_kernels(D, P, stream_env):
        name, args = k.split("<")
        out.add(k if name in SHARED else name[:-len("kernel")] + "bf16_kernel<" + args)
    return out


# ---------------------------------------------------------------------------------------------- emulation with defects
def emulate(q, k, v, d_o, conv_w, conv_b, P, scale):
    """agent_ref.emulate with o, dq, dk, dv rounded once to bf16 (held as f32)."""
    E = ref.emulate(q, k, v, d_o, conv_w, conv_b, P, scale)
    return {n: (bf16_round(t) if n in ROUNDED else t) for n, t in E.items()}


def emulate_defect(q, k, v, d_o, conv_w, conv_b, P, scale, defect=None):
    """agent_ref.emulate's chain (without its planted faults) with one of DEFECTS; defect=None equals `emulate` bit for
    bit (tests/test_agent_bf16_bounds.py::test_defect_emulation_is_the_emulation)."""
    import torch.nn.functional as F

    f32 = torch.float32
    rnd = bf16_trunc if defect == "truncate" else bf16_rne
    out = lambda x: rnd(x).to(f32)
    q, k, v, g, w, cb = (x.to(f32) for x in (q, k, v, d_o, conv_w, conv_b))
    if defect == "d_o_coarser":
        g = _on_grid(g.to(F64), torch.round, bits=7).to(f32)
    B, H, T, D = q.shape
    CH, NC = ref.chunk_len(D), ref.num_chunks(T, D)
    Tp = NC * CH
    scale = float(scale)
    mem, lens = ref.pool_matrix(T, P, "cpu", f32, ref.bins(T, P))
    lens = lens.view(-1, 1)
    tr = lambda x: x.transpose(-1, -2)
    ch = lambda x: F.pad(x, (0, 0, 0, Tp - T)).view(B, H, NC, CH, x.shape[-1])
    valid = (torch.arange(Tp) < T).view(1, 1, NC, 1, CH)

    def fold(parts):
        acc = torch.zeros_like(parts[:, :, 0])
        for c in range(NC):
            acc = acc + parts[:, :, c]
        return acc

    A = (mem @ q) / lens
    As = A * scale
    kc, vc, qc, gc = ch(k), ch(v), ch(q), ch(g)
    s = torch.einsum("bhpd,bhctd->bhcpt", As, kc).masked_fill(~valid, float("-inf"))
    m_c = s.max(-1).values
    e = torch.exp(s - m_c.unsqueeze(-1))
    l_c = e.sum(-1)
    part = torch.einsum("bhcpt,bhctd->bhcpd", e, vc)
    M = m_c.max(2).values
    a_c = torch.exp(m_c - M.unsqueeze(2))
    L = torch.zeros_like(M)
    sacc = torch.zeros_like(A)
    for c in range(NC):
        L = L + a_c[:, :, c] * l_c[:, :, c]
        sacc = sacc + a_c[:, :, c].unsqueeze(-1) * part[:, :, c]
    va_saved = sacc / L.unsqueeze(-1)
    va = bf16_round(va_saved) if defect == "vagent_bf16" else va_saved
    s2 = q @ tr(As)
    e2 = torch.exp(s2 - s2.max(-1, keepdim=True).values)
    p2 = e2 / e2.sum(-1, keepdim=True)
    o = (cb + ref._emu_conv(v, w)) + p2 @ va
    sc = (q @ tr(A)) * scale
    eb = torch.exp(sc - sc.max(-1, keepdim=True).values)
    pb = eb / eb.sum(-1, keepdim=True)
    dp = g @ tr(va)
    dl = (pb * dp).sum(-1, keepdim=True)
    ds = pb * (dp - dl)
    dq = (ds * scale) @ A
    if defect == "dq_twice":
        dq = bf16_round(dq)
    dVa = fold(torch.einsum("bhctp,bhctd->bhcpd", ch(pb), gc))
    dA2 = fold(scale * torch.einsum("bhctp,bhctd->bhcpd", ch(ds), qc))
    delta1 = (dVa * va).sum(-1)
    pr = torch.exp(tr((k @ tr(A)) * scale) - M.unsqueeze(-1)) / L.unsqueeze(-1)
    d1 = pr * (dVa @ tr(v) - delta1.unsqueeze(-1))
    dk = tr(d1 * scale) @ A
    dv = ref._emu_conv(g, w, flip=True) + tr(pr) @ dVa
    pa1 = scale * torch.einsum("bhctp,bhctd->bhcpd", ch(tr(d1)), kc)
    dA = dA2
    for c in range(NC):
        dA = dA + pa1[:, :, c]
    dA = dA / lens
    dq = dq + tr(mem) @ dA
    vp = F.pad(v, (0, 0, 1, 1, 1, 1))
    taps = torch.stack([ch(g * vp[:, a:a + H, b:b + T, :]).sum(3) for a in range(3) for b in range(3)], 3)
    dw = ref.emu_reduce(taps.reshape(B * H * NC, 9 * D)).view(9, D).t().reshape(D, 1, 3, 3)
    db = ref.emu_reduce(gc.sum(3).reshape(B * H * NC, D))
    return {"agents": A, "vagent": va_saved, "M": M, "L": L, "o": out(o), "dq": out(dq), "dk": out(dk), "dv": out(dv),
            "dconv_w": dw, "dconv_b": db}
