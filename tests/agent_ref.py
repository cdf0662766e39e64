"""fp64 reference, per-element error bounds, input families, an f32 emulation and a restatement of the host dispatch for
the AgentAttention kernels (csrc/agent.hip).

The reference is computed in fp64 on the f32 values the kernels read and takes the arguments of the C ABI: q, k, v,
d_o as (B, H, T, D) views of any layout, the depthwise convolution's weight (D, 1, 3, 3) and bias (D), the agent count
P (independent of H) and the scale.
    agents_i = mean of q[lo_i : hi_i],  lo_i = floor(i T / P),  hi_i = ceil((i + 1) T / P)   (bins overlap when T % P != 0)
    vagent   = softmax((A scale) K^T) V,     stats1 = (M, L): row max of the scaled stage-1 scores, L = sum exp(s - M)
    o        = softmax((q scale) A^T) vagent + dwconv3x3(v over the (head, token) plane, zero padded) + bias
and dq, dk, dv, dconv_w, dconv_b by torch.autograd in fp64.  u32 = 2^-24.  No bound is relative to a tensor's maximum.

Hard tier.  The kernels are plain f32 (no fast-math); a sum of terms t_i reached through at most n rounded operations,
in any order, fused or not, is within gamma_n sum|t_i| (gamma_n = n u32 / (1 - n u32)); expf is within 1 ulp = 2 u32
(the HIP math API's stated maximum).  Errors of intermediate results are carried forward to first order, exponent
errors through expm1, normaliser errors through 1 / (1 - e).  With NC chunks of CH tokens, n_tok = NC + 20 covers every
sum over tokens (at most 8 rows per lane group, 3 shuffle steps, 3 adds over the waves, the scale or the combine's
product, NC partials folded in chunk order, a division).  Per output, from the source:
* agents: len adds in a fixed but non-sequential order (lane groups, shuffles, waves) and a division:
  dA = gamma_{len + 2} mean|q|.
* scores: the forward rounds A scale, then D products and adds; the backward rounds the dot product, then the scale:
  ds1_ij = gamma_{D + 3} scale |A_i|.|k_j| + scale |dA_i|.|k_j|, ds2 likewise with q; dM_i = max_j ds1_ij (the kernel's
  maximum is one of its own scores).
* one unnormalised weight: relative error eps_ij = expm1(ds_ij + dM_i + 8 u32 (|s_ij - M_i| + 1)): the roundings of
  s - m_chunk and of m_chunk - M (|s - m| + |m - M| = |s - M|), two expf, their product; the backward's single expf of
  s scale - M with M as stored.
* normaliser: ebar_i = sum_j p_ij eps_ij + gamma_{NC + 12} (stage 1: chunk row sums of CH / 64 adds and 6 shuffle
  steps, one product and one add per chunk in the combine) or + gamma_{P + 2} (stage 2, in registers); a normalised
  weight is off by E_ij = (1 + eps_ij) / (1 - ebar_i) - 1 (+ 2 u32 for stage 2's division and the backward's 1 / L).
* vagent: (p1 E1) |v| + gamma_{n_tok} p1 |v|.      stats1: |dM| <= dM_i;  |dL| <= L ebar_i.
* o: (p2 E2) |va| + p2 |dva| + gamma_{P + 12} (p2 |va| + sum_taps |w| |v| + |b|): the bias, nine taps, P agents in one
  chain.
* backward, with dP2 = dO va^T, dl = sum_i p2 dP2, dS2 = p2 (dP2 - dl), dVa = p2^T dO, delta1 = <dVa, va>,
  dP1 = dVa v^T, dS1 = p1 (dP1 - delta1):
    e(dP2) = gamma_{D + 2} |dO| |va|^T + |dO| |dva|^T;   e(dl) = sum_i p2 (E2 |dP2| + e(dP2)) + gamma_{P + 1} sum_i p2 |dP2|
    e(dS2) = p2 ((E2 + 2 u32) |dP2 - dl| + e(dP2) + e(dl))          -- the conditioning: p |dP - delta|
    e(dVa) = (p2 E2)^T |dO| + gamma_{n_tok} p2^T |dO|  (partials pva folded in chunk order by agent_mid_kernel)
    e(delta1) = e(dVa).|va| + |dVa|.|dva| + gamma_{D + 2} |dVa|.|va|;   e(dP1) = gamma_{D + 2} |dVa| |v|^T + e(dVa) |v|^T
    e(dS1) = p1 ((E1 + 2 u32) |dP1 - delta1| + e(dP1) + e(delta1))
    dk: scale (e(dS1)^T |A| + |dS1|^T |dA|) + gamma_{P + 3} scale |dS1|^T |A|
    dv: (p1 E1)^T |dVa| + p1^T e(dVa) + gamma_{P + 12} (p1^T |dVa| + sum_taps |w| |dO|)   (transposed conv of dO)
    dA: (scale (e(dS2)^T |q| + e(dS1) |k|) + gamma_{2 n_tok + 6} scale (|dS2|^T |q| + |dS1| |k|)) / len  (pa2 folded
        by the mid kernel, pa1 in chunk order by the pool backward, then dA / len)
    dq: scale (e(dS2) |A| + |dS2| |dA|) + sum over the bins holding the token of e(dA_i)
        + gamma_{P + 3} (scale |dS2| |A| + sum over those bins of S(dA_i))
* dconv_w[c][a][b] = sum_{b,h,t} dO v(shifted), dconv_b = sum dO: gamma_n sum |dO| |v| (sum |dO|) with
  n = ceil(rows / 64) + 84 over rows = B H NC partial rows: at most 8 terms per lane group, 3 shuffle steps and 3 adds
  over the waves per workgroup, rows / 64 strided adds and 64 folds in agent_conv_reduce_kernel.
Flush-to-zero adds n 2^-126 (1 + the plain sum of the multiplicands' magnitudes) per output ("ftz_" entries).

Tight tier.  The hard tier lies far above what f32 reaches: it lets every rounding error take its worst sign, so it
grows with the length of a sum where the error grows like its root (dq at T = 8193: 10^5 above the kernel's error),
and on the hard families (large, climb) it is wide by construction.  A second pass over the same propagation
(_propagate(rms=True)) gives every element the size its error typically has: independent errors add in squares, a sum
of n terms t_i rounds to sqrt(n) u32 (|sum| + sqrt(sum t_i^2)), and the error of M, common to a row's weights and its
normaliser, is left out of p (it cancels there; L alone moves with it).  With S that size in units of u32,
    q = (|got - ref| - ftz) / (u32 S)
is O(1) at every shape and family, and is held per output to TIGHT_FACTOR x the worst q that the f32 emulation below
(`emulate`: the kernels' chain -- chunked stage 1 with per-chunk (max, sum, partial) and the combine's
expf(m_c - M) rescale, torch.exp in f32, partials folded in chunk order, dA / len in the pool backward, the
convolution gradient's 64 strided sums folded in order) reaches over the inputs of every case of the GPU sweep and
every family at three further shapes: Q_EMU, asserted by tests/test_agent_bounds.py, never taken from the GPU.

Input families (make_inputs): diffuse, peaked, needles, climb, large, flat_q, conv_binade, conv_zero -- see there.

Measured on the MI355X, worst over tests/test_agent_bounds_gpu.py -- hard ratio, q / (4 Q_EMU):
    agents 0.251, 0.095    vagent 0.005, 0.101    M 0.030, 0.118    L 0.013, 0.166    o 0.245, 0.186
    dq 0.0003, 0.122       dk 0.0014, 0.100       dv 0.280, 0.172   dconv_w 0.037, 0.194    dconv_b 0.012, 0.145
    amk_agent_conv_grad_reduce alone (hard tier): dconv_w 0.040, dconv_b 0.037
The first run passed on every path -- streaming <4 | 6 | 8>, the LDS-staged <D, 8 | 16> at all three head dims
(<64, 8> under AMK_AGENT_STREAM=0), 65 chunks, every layout -- and every bitwise property held (repeat, batch and
head independence, M under a rotation of the chunks): no fault was found in csrc/agent.hip.  The kernel's worst q is
0.4 to 0.8 of the emulation's (its products and sums are fused), so the tight tier sits about five times above the
kernel's own worst error at every shape, the 65-chunk cases included.
"""
import re

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
FTZ = 2.0 ** -126
TIGHT_FACTOR = 4.0
F64 = torch.float64
MAXP = 16
CW = 8.0     # roundings of one weight's exponent, in u32 (|s - M| + 1)
FAMILIES = ("diffuse", "peaked", "needles", "climb", "large", "flat_q", "conv_binade", "conv_zero")
OUTPUTS = ("agents", "vagent", "M", "L", "o", "dq", "dk", "dv", "dconv_w", "dconv_b")

# worst q of the f32 emulation per output (tests/test_agent_bounds.py::test_emulation_defines_q)
Q_EMU = {"agents": 1.73, "vagent": 1.9, "M": 0.685, "L": 0.658, "o": 1.48, "dq": 1.18, "dk": 2.02, "dv": 1.57,
         "dconv_w": 0.912, "dconv_b": 0.965}


def gamma(n):
    n = torch.as_tensor(n, dtype=F64)
    return n * U32 / (1 - n * U32)


# ---------------------------------------------------------------------------------------------- host restatement
def chunk_len(D):
    return 64 if D == 128 else 128


def num_chunks(T, D):
    return -(-T // chunk_len(D)) if T > 0 and D in (32, 64, 128) else 0


def ws_floats(B, H, T, P, D, backward):
    if min(B, H, T, P) <= 0 or D not in (32, 64, 128):
        return 0
    cells, rows = B * H * num_chunks(T, D) * P, B * H * P
    return 3 * cells * D + 2 * rows * D + rows if backward else cells * (D + 2)


def bins(T, P):
    """(lo, hi) of the P adaptive bins over T tokens: the kernel's bin_lo / bin_hi."""
    return [i * T // P for i in range(P)], [((i + 1) * T + P - 1) // P for i in range(P)]


def _atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def expected_kernels(D, P, stream_env=None):
    """The kernel instantiations that amk_agent_attn_fwd + _bwd + amk_agent_conv_grad_reduce launch; stream_env: the
    value of AMK_AGENT_STREAM (None: unset)."""
    pm = 8 if P <= 8 else 16
    ks = {f"agent_pool_kernel<{D}>", f"agent_s1_partial_kernel<{D},{pm}>", f"agent_s1_combine_kernel<{D}>",
          f"agent_s2_kernel<{D},{pm}>", f"agent_mid_kernel<{D}>", f"agent_pool_bwd_kernel<{D}>",
          f"agent_conv_reduce_kernel<{D}>"}
    streaming = (1 if stream_env is None else _atoi(stream_env)) != 0 and P <= 8 and D == 64
    if streaming:
        w = 4 if P <= 4 else 6 if P <= 6 else 8
        ks |= {f"agent_s2_bwd_stream_kernel<{w}>", f"agent_s1_bwd_stream_kernel<{w}>"}
    else:
        ks |= {f"agent_s2_bwd_kernel<{D},{pm}>", f"agent_s1_bwd_kernel<{D},{pm}>"}
    return ks


def all_instantiations():
    """Every instantiation the host code can launch."""
    out = set()
    for D in (32, 64, 128):
        for P in (8, 16):
            out |= expected_kernels(D, P, "0")
    for P in (4, 6, 8):
        out |= expected_kernels(64, P, None)
    return out


def kernel_id(name):
    """'agent_s2_kernel<64,8>' from a kernel name as a profiler reports it (demangled or mangled); None for others."""
    m = re.search(r"(agent_\w+?_kernel)<([\d, ]+)>", name)
    if m:
        return f"{m.group(1)}<{m.group(2).replace(' ', '')}>"
    m = re.search(r"\d+(agent_\w+?_kernel)I((?:Li\d+E)+)E", name)
    if m:
        return m.group(1) + "<" + ",".join(re.findall(r"Li(\d+)E", m.group(2))) + ">"
    return None


FEATURES = ("last chunk of one token", "exactly full last chunk", "T < chunk", "NC > 64", "P == T", "P == 1", "P == 16",
            "P > H", "P < H", "H == 1", "overlapping bins", "bin crosses a 64-token block", "padded strides",
            "views into a wider buffer", "packed qkv", "separate tensors")


def features(case):
    """The edges a case (dict with B, H, T, D, P, layout) reaches."""
    B, H, T, D, P = (case[k] for k in "BHTDP")
    CH, NC = chunk_len(D), num_chunks(T, D)
    lo, hi = bins(T, P)
    f = set()
    if NC >= 2 and T % CH == 1:
        f.add("last chunk of one token")
    if T % CH == 0:
        f.add("exactly full last chunk")
    if T < CH:
        f.add("T < chunk")
    if NC > 64:
        f.add("NC > 64")
    for name, hit in (("P == T", P == T), ("P == 1", P == 1), ("P == 16", P == 16), ("P > H", P > H), ("P < H", P < H),
                      ("H == 1", H == 1), ("overlapping bins", T % P != 0),
                      ("bin crosses a 64-token block", any(a // 64 != (b - 1) // 64 for a, b in zip(lo, hi)))):
        if hit:
            f.add(name)
    f.add({"bthd_pad": "padded strides", "view": "views into a wider buffer", "packed": "packed qkv",
           "separate": "separate tensors"}[case["layout"]])
    return f


# ---------------------------------------------------------------------------------------------- reference
def pool_matrix(T, P, device, dtype=F64, lohi=None):
    """(membership (P, T) of 0 / 1, bin lengths (P))."""
    lo, hi = lohi or bins(T, P)
    t = torch.arange(T, device=device)
    mem = (t >= torch.tensor(lo, device=device).view(-1, 1)) & (t < torch.tensor(hi, device=device).view(-1, 1))
    return mem.to(dtype), torch.tensor([b - a for a, b in zip(lo, hi)], device=device, dtype=dtype)


def dwconv(x, w, flip=False):
    """Depthwise 3x3 over the (head, token) plane of x (B, H, T, D), zero padded; w (D, 1, 3, 3).  flip: the
    transposed convolution."""
    B, H, T, D = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros_like(x)
    for a in range(3):
        for b in range(3):
            sa, sb = (2 - a, 2 - b) if flip else (a, b)
            out = out + xp[:, sa:sa + H, sb:sb + T, :] * w[:, 0, a, b]
    return out


def _conv_wgrad(g, v):
    """(D, 1, 3, 3): sum over (batch, head, token) of g[h, t] v[h + a - 1, t + b - 1]."""
    B, H, T, D = g.shape
    vp = F.pad(v, (0, 0, 1, 1, 1, 1))
    return torch.stack([torch.stack([(g * vp[:, a:a + H, b:b + T, :]).sum((0, 1, 2)) for b in range(3)], -1)
                        for a in range(3)], -2).view(D, 1, 3, 3)


def _ftz(n, *mags):
    s = 1.0
    for m in mags:
        s = s + m
    return n * FTZ * s


def reference(q, k, v, d_o, conv_w, conv_b, P, scale):
    """{name, "bound_" name, "ftz_" name, "S_" name} for name in OUTPUTS, fp64, on the inputs' device."""
    B, H, T, D = q.shape
    dev = q.device
    q64, k64, v64 = (x.detach().to(F64).clone().requires_grad_(True) for x in (q, k, v))
    w64, b64 = (x.detach().to(F64).clone().requires_grad_(True) for x in (conv_w, conv_b))
    g = d_o.detach().to(F64)
    mem, lens = pool_matrix(T, P, dev)
    A = (mem / lens.view(-1, 1)) @ q64                                        # (B, H, P, D)
    s1 = (A * scale) @ k64.transpose(-1, -2)                                  # (B, H, P, T)
    M = s1.max(-1).values
    e1 = torch.exp(s1 - M.unsqueeze(-1))
    L = e1.sum(-1)
    p1 = e1 / L.unsqueeze(-1)
    va = p1 @ v64
    s2 = (q64 * scale) @ A.transpose(-1, -2)                                  # (B, H, T, P)
    p2 = torch.softmax(s2, -1)
    o = p2 @ va + dwconv(v64, w64) + b64
    dq, dk, dv, dw, db = torch.autograd.grad(o, [q64, k64, v64, w64, b64], g)
    R = {"agents": A, "vagent": va, "M": M, "L": L, "o": o, "dq": dq, "dk": dk, "dv": dv, "dconv_w": dw, "dconv_b": db}
    R = {n: t.detach() for n, t in R.items()}
    with torch.no_grad():
        _bounds(R, q64.detach(), k64.detach(), v64.detach(), g, w64.detach(), b64.detach(), s1.detach(), p1.detach(),
                s2.detach(), p2.detach(), mem, lens, P, scale)
    return R


def _bounds(R, q, k, v, g, w, b, s1, p1, s2, p2, mem, lens, P, scale):
    hard, ftz = _propagate(R, q, k, v, g, w, b, s1, p1, s2, p2, mem, lens, P, scale, rms=False)
    typical, _ = _propagate(R, q, k, v, g, w, b, s1, p1, s2, p2, mem, lens, P, scale, rms=True)
    for name in OUTPUTS:
        R["ftz_" + name] = ftz[name]
        R["bound_" + name] = hard[name] + ftz[name]
        R["S_" + name] = typical[name] / U32


def _propagate(R, q, k, v, g, w, b, s1, p1, s2, p2, mem, lens, P, scale, rms):
    """The first-order error terms of every output ({name: tensor}, {name: flush-to-zero term}).  rms=False: the hard
    tier (worst case: magnitudes add, gamma_n per sum).  rms=True: the same propagation with independent errors adding
    in squares and a sum of n terms rounding to sqrt(n) u32 (|result| + root sum of squares of the terms) -- the
    size rounding errors typically have, the tight tier's S."""
    B, H, T, D = q.shape
    dev = q.device
    NC = num_chunks(T, D)
    n_tok = NC + 20
    tr = lambda x: x.transpose(-1, -2)
    t64 = lambda n: torch.as_tensor(n, dtype=F64, device=dev)
    if rms:
        sq = lambda x: torch.where(x.abs() < 1e-150, torch.zeros_like(x), x) ** 2 if torch.is_tensor(x) else x * x   # (no denormal squares)
        G = lambda n: t64(n).sqrt() * U32
        MM = lambda X, Y: torch.sqrt(sq(X) @ sq(Y))
        SS = lambda X, keepdim=False: torch.sqrt(sq(X).sum(-1, keepdim=keepdim))
        ADD = lambda *xs: torch.sqrt(sum(sq(x) for x in xs))
        RND = lambda n, terms, result: G(n) * (result.abs() + terms)
        CONV = lambda x, ww, flip=False: torch.sqrt(dwconv(x * x, ww * ww, flip))
        WG = lambda gg, vv: torch.sqrt(_conv_wgrad(gg * gg, vv * vv))
        cw = CW ** 0.5
    else:
        G = lambda n: t64(n) * U32 / (1 - t64(n) * U32)
        MM = lambda X, Y: X @ Y
        SS = lambda X, keepdim=False: X.sum(-1, keepdim=keepdim)
        ADD = lambda *xs: sum(xs)
        RND = lambda n, terms, result: G(n) * terms
        CONV = dwconv
        WG = _conv_wgrad
        cw = CW
    aq, ak, av, ag, aw = q.abs(), k.abs(), v.abs(), g.abs(), w.abs()
    A, va, M, L = R["agents"], R["vagent"], R["M"], R["L"]
    aA, ava = A.abs(), va.abs()
    ln = lens.view(-1, 1)
    out, ftz = {}, {}
    # agents
    out["agents"] = RND(ln + 2, MM(mem / ln, aq), A)
    ftz["agents"] = (ln + 2) * FTZ * torch.ones_like(A)
    dA = out["agents"] + ftz["agents"]
    # stage 1.  The error of M is common to a row's weights and its normaliser: the worst case carries it, the typical
    # size does not (it cancels in p; L alone moves with it)
    es1 = ADD(RND(D + 3, scale * MM(aA, tr(ak)), s1), scale * MM(dA, tr(ak)))
    dM = es1.max(-1).values
    spread1 = cw * U32 * ((s1 - M.unsqueeze(-1)).abs() + 1)
    eps1 = torch.expm1(ADD(es1, spread1) if rms else es1 + dM.unsqueeze(-1) + spread1)
    ebar1 = ADD(SS(p1 * eps1), G(NC + 12))
    if rms:
        E1 = ADD(eps1, ebar1.unsqueeze(-1), 2 * U32)
    else:
        E1 = (1 + eps1) / (1 - ebar1.clamp(max=0.5)).unsqueeze(-1) - 1 + 2 * U32
    out["M"], ftz["M"] = dM, FTZ * torch.ones_like(M)
    out["L"], ftz["L"] = (L * ADD(ebar1, dM) if rms else L * ebar1), _ftz(T + 20, torch.zeros_like(L))
    out["vagent"] = ADD(MM(p1 * E1, av), RND(n_tok, MM(p1, av), va))
    ftz["vagent"] = _ftz(T + 20, av.sum(-2, keepdim=True).expand_as(va))
    dva = out["vagent"] + ftz["vagent"]
    # stage 2
    es2 = ADD(RND(D + 3, scale * MM(aq, tr(aA)), s2), scale * MM(aq, tr(dA)))
    spread2 = cw * U32 * ((s2 - s2.max(-1, keepdim=True).values).abs() + 1)
    eps2 = torch.expm1(ADD(es2, spread2) if rms else es2 + es2.max(-1, keepdim=True).values + spread2)
    ebar2 = ADD(SS(p2 * eps2, True), G(P + 2))
    E2 = ADD(eps2, ebar2, 2 * U32) if rms else (1 + eps2) / (1 - ebar2.clamp(max=0.5)) - 1 + 2 * U32
    S_conv = CONV(av, aw)
    out["o"] = ADD(MM(p2 * E2, ava), MM(p2, dva), RND(P + 12, ADD(MM(p2, ava), S_conv, b.abs()), R["o"]))
    ftz["o"] = 0.0 if rms else _ftz(P + 12, ava.sum(-2, keepdim=True).expand_as(q), S_conv)
    # stage-2 backward
    dp2 = g @ tr(va)
    edp2 = ADD(RND(D + 2, MM(ag, tr(ava)), dp2), MM(ag, tr(dva)))
    dl = (p2 * dp2).sum(-1, keepdim=True)
    edl = ADD(SS(p2 * ADD(E2 * dp2.abs(), edp2), True), RND(P + 1, SS(p2 * dp2.abs(), True), dl))
    ds2 = p2 * (dp2 - dl)
    eds2 = p2 * ADD((E2 + 2 * U32) * (dp2 - dl).abs(), edp2, edl) + FTZ
    e_dq2 = scale * ADD(MM(eds2, aA), MM(ds2.abs(), dA))
    dVa = tr(p2) @ g
    e_dVa = ADD(MM(tr(p2 * E2), ag), RND(n_tok, MM(tr(p2), ag), dVa)) + _ftz(T + 20, ag.sum(-2, keepdim=True).expand_as(dVa))
    delta1 = (dVa * va).sum(-1)
    edelta1 = ADD(SS(e_dVa * ava), SS(dVa.abs() * dva), RND(D + 2, SS(dVa.abs() * ava), delta1))
    # stage-1 backward
    dp1 = dVa @ tr(v)
    edp1 = ADD(RND(D + 2, MM(dVa.abs(), tr(av)), dp1), MM(e_dVa, tr(av)))
    ds1 = p1 * (dp1 - delta1.unsqueeze(-1))
    eds1 = p1 * ADD((E1 + 2 * U32) * (dp1 - delta1.unsqueeze(-1)).abs(), edp1, edelta1.unsqueeze(-1)) + FTZ
    out["dk"] = ADD(scale * MM(tr(eds1), aA), scale * MM(tr(ds1.abs()), dA), RND(P + 3, scale * MM(tr(ds1.abs()), aA), R["dk"]))
    ftz["dk"] = _ftz(P + 3, aA.sum(-2, keepdim=True).expand_as(k))
    S_convT = CONV(ag, aw, True)
    out["dv"] = ADD(MM(tr(p1 * E1), dVa.abs()), MM(tr(p1), e_dVa),
                    RND(P + 12, ADD(MM(tr(p1), dVa.abs()), S_convT), R["dv"]))
    ftz["dv"] = 0.0 if rms else _ftz(P + 12, dVa.abs().sum(-2, keepdim=True).expand_as(v), S_convT)
    dA_sum = scale * (tr(ds2) @ q + ds1 @ k)                        # dA len
    S_dA = ADD(scale * MM(tr(ds2.abs()), aq), scale * MM(ds1.abs(), ak))
    e_dA = ADD(scale * MM(tr(eds2), aq), scale * MM(eds1, ak), RND(2 * n_tok + 6, S_dA, dA_sum)) / ln
    out["dq"] = ADD(e_dq2, MM(tr(mem), e_dA), RND(P + 3, ADD(scale * MM(ds2.abs(), aA), MM(tr(mem), S_dA / ln)), R["dq"]))
    ftz["dq"] = _ftz(2 * T + 40, aA.sum(-2, keepdim=True).expand_as(q), (aq.sum(-2, keepdim=True) + ak.sum(-2, keepdim=True)).expand_as(q))
    # convolution gradients
    n_cv = -(-(B * H * NC) // 64) + 84
    out["dconv_w"] = RND(n_cv, WG(ag, av), R["dconv_w"])
    out["dconv_b"] = RND(n_cv, SS(tr(ag.reshape(-1, D))), R["dconv_b"])
    ftz["dconv_w"], ftz["dconv_b"] = _ftz(n_cv, torch.zeros_like(out["dconv_w"])), _ftz(n_cv, torch.zeros_like(out["dconv_b"]))
    return out, ftz


def reduce_reference(wpart, bpart):
    """amk_agent_conv_grad_reduce alone: fp64 column sums in the (D, 1, 3, 3) / (D) layouts with the hard bound
    gamma_{rows + 66} sum|part| (rows / 64 strided adds, 64 folds; at most rows + 64 on any path)."""
    rows, _, D = wpart.shape
    w64, b64 = wpart.to(F64), bpart.to(F64)
    n = rows + 66
    R = {"dconv_w": w64.sum(0).t().reshape(D, 1, 3, 3), "dconv_b": b64.sum(0)}
    S = {"dconv_w": w64.abs().sum(0).t().reshape(D, 1, 3, 3), "dconv_b": b64.abs().sum(0)}
    for name in ("dconv_w", "dconv_b"):
        R["ftz_" + name] = n * FTZ * torch.ones_like(S[name])
        R["bound_" + name] = float(gamma(n)) * S[name] + R["ftz_" + name]
        R["S_" + name] = float(gamma(n)) * S[name] / U32
    return R


# ---------------------------------------------------------------------------------------------- checking
WORST = {}   # output -> [worst hard ratio, worst q / (TIGHT_FACTOR Q_EMU)] over every check of the process


def measures(got, R, name):
    """(elements outside the hard bound, worst |err| / hard bound, worst q, flat index of the worst ratio)."""
    ref = R[name]
    a = got.detach().to(ref.device, F64).reshape(ref.shape)
    err = (a - ref).abs()
    hb, S, ftz = R["bound_" + name], R["S_" + name], R["ftz_" + name]
    bad = ~(err <= hb)                                          # (a NaN result is outside the bound too)
    zero = torch.zeros_like(err)
    inf = torch.full_like(err, float("inf"))
    ratio = torch.where(err > 0, err / hb, zero)
    ratio = torch.where(torch.isnan(err), inf, ratio)
    q = torch.where((err > ftz) & (S > 0), (err - ftz).clamp_min(0) / (U32 * S), zero)
    q = torch.where((err > ftz) & ~(S > 0), inf, q)
    q = torch.where(torch.isnan(err), inf, q)
    if a.numel() == 0:
        return 0, 0.0, 0.0, -1
    return int(bad.sum()), float(ratio.max()), float(q.max()), int(ratio.reshape(-1).argmax())


def violations(got, R, name, tight=True):
    """Number of elements that miss the hard tier, plus 1 if the tight tier is missed."""
    nbad, _, q, _ = measures(got, R, name)
    return nbad + (1 if tight and q > TIGHT_FACTOR * Q_EMU[name] else 0)


def assert_within(got, R, name, what="", tight=True, key=None):
    """Both tiers on every element (tight=False: the hard tier alone); records the worst figures in WORST[key or name]."""
    nbad, ratio, q, at = measures(got, R, name)
    lim = TIGHT_FACTOR * Q_EMU[name]
    w = WORST.setdefault(key or name, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], q / lim if tight else 0.0)
    where = tuple(int(i) for i in torch.unravel_index(torch.tensor(max(at, 0)), R[name].shape)) if R[name].dim() else ()
    print(f"{what} {name}: hard ratio {ratio:.4g}, q {q:.4g} (limit {lim:.4g}), worst at {where}")
    assert nbad == 0, f"{what} {name}: {nbad} elements outside the hard bound (worst {ratio:.3g}x at {where})"
    if tight:
        assert q <= lim, f"{what} {name}: q = |err| / (u32 S) reaches {q:.3g}, limit {lim:.3g} ({TIGHT_FACTOR} x the emulation)"


# ---------------------------------------------------------------------------------------------- input families
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def needle_positions(T, D):
    CH = chunk_len(D)
    return [p % T for p in (0, CH - 1, CH, 2 * CH - 1, T - 1)]


def make_inputs(family, B, H, T, D, P, scale, seed):
    """q, k, v, d_o (B, H, T, D), conv_w (D, 1, 3, 3), conv_b (D): f32, contiguous, on the CPU.
    diffuse      N(0, 1)
    peaked       q scaled so that neither softmax's scaled scores exceed a standard deviation of 5 and one reaches it
    needles      per (b, h, agent) one planted key leads the rest by ~24 in the scaled score, at 0, CH - 1, CH,
                 2 CH - 1 or T - 1 (mod T), another position per agent and head: the other chunks' factors underflow
    climb        k gains a component along a fixed direction growing by a step per chunk (3 in the scaled score), q
                 carries that direction: the running maximum moves in every chunk, the last chunk dominates
    large        a common component of 60 D^(1/4) along the unit diagonal on q and k, sign alternating by head: scaled
                 scores near 3600 that differ between keys by O(10)
    flat_q       all rows of q equal within a head: equal agents, stage 2 exactly uniform, its dS a pure cancellation
    conv_binade  conv weights and bias by per-channel powers of two over 2^-12 .. 2^12; v rows x 64 at tokens 0,
                 CH - 1, CH, T - 1 of the first and last head
    conv_zero    conv_w = 0, conv_b = 0"""
    g = _gen(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    q, k, v, d_o = n(B, H, T, D), n(B, H, T, D), n(B, H, T, D), n(B, H, T, D)
    cw, cb = n(D, 1, 3, 3) / 3, n(D)
    CH = chunk_len(D)
    mem, lens = pool_matrix(T, P, "cpu", torch.float32)
    pool = lambda x: (mem / lens.view(-1, 1)) @ x
    if family == "peaked":
        A = pool(q)
        sd1 = float(((A * scale) @ k.transpose(-1, -2)).std(unbiased=False))
        sd2 = float(((q * scale) @ A.transpose(-1, -2)).std(unbiased=False))
        f = min(5.0 / sd1 if sd1 > 1e-6 else 1e9, (5.0 / sd2) ** 0.5 if sd2 > 1e-6 else 1e9)
        q = q * (f if f < 1e8 else 1.0)
    elif family == "needles":
        A = pool(q)
        s = (A * scale) @ k.transpose(-1, -2)                                  # (B, H, P, T)
        pos = needle_positions(T, D)
        for b in range(B):
            for h in range(H):
                for i in range(P):
                    t = pos[(i + h + b) % len(pos)]
                    a = A[b, h, i]
                    lead = 24.0 + float(s[b, h, i].max() - s[b, h, i, t])
                    k[b, h, t] += a * (lead / (scale * float(a @ a) + 1e-30))
    elif family == "climb":
        u = n(D)
        u = u / u.norm()
        step = 3.0 / (2.0 * scale)
        k = k + (torch.arange(T) // CH).float().view(1, 1, T, 1) * step * u
        q = q + 2.0 * u
    elif family == "large":
        sign = torch.tensor([1.0 if h % 2 == 0 else -1.0 for h in range(H)]).view(1, H, 1, 1)
        c = 60.0 * D ** 0.25 / D ** 0.5
        q, k = q + sign * c, k + sign * c
    elif family == "flat_q":
        q = q[:, :, :1].expand(B, H, T, D).clone()
    elif family == "conv_binade":
        e = torch.round(torch.linspace(-12, 12, D))[torch.randperm(D, generator=g)]
        cw, cb = cw * torch.exp2(e).view(D, 1, 1, 1), cb * torch.exp2(e)
        for t in {0, (CH - 1) % T, CH % T, T - 1}:
            v[:, 0, t] *= 64.0
            if H > 1:
                v[:, H - 1, t] *= 64.0
    elif family == "conv_zero":
        cw, cb = torch.zeros_like(cw), torch.zeros_like(cb)
    elif family != "diffuse":
        raise ValueError(family)
    return tuple(x.contiguous() for x in (q, k, v, d_o, cw, cb))


# ---------------------------------------------------------------------------------------------- f32 emulation
MUTATIONS = ("chunk_dropped", "wrong_chunk_max", "chunk_last_token_unwritten", "halo_heads_swapped", "conv_not_padded",
             "hi_floor", "dA_not_divided", "delta1_neighbour", "reduce_row_missing", "p16_last_ignored",
             "second_pass_dropped")


def _emu_conv(x, w, flip=False, mut=None):
    B, H, T, D = x.shape
    if mut == "conv_not_padded":                                   # the rows at t = -1 and t = T repeat the edge
        xp = F.pad(F.pad(x, (0, 0, 1, 1), mode="replicate"), (0, 0, 0, 0, 1, 1))
    else:
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros_like(x)
    for a in range(3):
        for b in range(3):
            sa, sb = (2 - a, 2 - b) if flip else (a, b)
            if mut == "halo_heads_swapped":
                sa = 2 - sa
            out = out + xp[:, sa:sa + H, sb:sb + T, :] * w[:, 0, a, b]
    return out


def emu_reduce(part, drop_last=False):
    """agent_conv_reduce_kernel in f32: 64 strided partial sums over the rows, folded in order.  part (rows, X)."""
    if drop_last:
        part = part[:-1]
    rows, X = part.shape
    n = -(-rows // 64)
    p = F.pad(part, (0, 0, 0, n * 64 - rows)).view(n, 64, X)
    acc = torch.zeros(64, X, dtype=part.dtype)
    for i in range(n):
        acc = acc + p[i]
    t = torch.zeros(X, dtype=part.dtype)
    for j in range(64):
        t = t + acc[j]
    return t


def emulate(q, k, v, d_o, conv_w, conv_b, P, scale, mut=None):
    """The kernels' chain in f32 on the CPU ({name: tensor} for OUTPUTS); mut: a planted fault of MUTATIONS."""
    f32 = torch.float32
    q, k, v, g, w, cb = (x.to(f32) for x in (q, k, v, d_o, conv_w, conv_b))
    B, H, T, D = q.shape
    CH, NC = chunk_len(D), num_chunks(T, D)
    Tp = NC * CH
    scale = float(scale)
    lo, hi = bins(T, P)
    if mut == "hi_floor":
        hi = [max((i + 1) * T // P, lo[i] + 1) for i in range(P)]
    mem, lens = pool_matrix(T, P, "cpu", f32, (lo, hi))
    lens = lens.view(-1, 1)
    tr = lambda x: x.transpose(-1, -2)
    ch = lambda x: F.pad(x, (0, 0, 0, Tp - T)).view(B, H, NC, CH, x.shape[-1])          # (B, H, NC, CH, .), zero rows past T
    valid = (torch.arange(Tp) < T).view(1, 1, NC, 1, CH)

    def fold(parts):                                               # chunk order
        acc = torch.zeros_like(parts[:, :, 0])
        for c in range(NC):
            acc = acc + parts[:, :, c]
        return acc

    A = (mem @ q) / lens
    As = A * scale
    # stage 1, chunked
    kc, vc, qc, gc = ch(k), ch(v), ch(q), ch(g)
    s = torch.einsum("bhpd,bhctd->bhcpt", As, kc).masked_fill(~valid, float("-inf"))
    m_c = s.max(-1).values                                         # (B, H, NC, P)
    e = torch.exp(s - m_c.unsqueeze(-1))
    l_c = e.sum(-1)
    part = torch.einsum("bhcpt,bhctd->bhcpd", e, vc)
    M = m_c.max(2).values
    a_c = torch.exp(m_c - M.unsqueeze(2))
    if mut == "wrong_chunk_max":
        a_c = torch.roll(a_c, 1, 2)
    L = torch.zeros_like(M)
    sacc = torch.zeros_like(A)
    for c in range(NC):
        if mut == "chunk_dropped" and c == min(1, NC - 1) or mut == "second_pass_dropped" and c >= 64:
            continue                                               # (second pass: the combine kernel's chunks 64 ..)
        L = L + a_c[:, :, c] * l_c[:, :, c]
        sacc = sacc + a_c[:, :, c].unsqueeze(-1) * part[:, :, c]
    va = sacc / L.unsqueeze(-1)
    # stage 2
    s2 = q @ tr(As)
    e2 = torch.exp(s2 - s2.max(-1, keepdim=True).values)
    p2 = e2 / e2.sum(-1, keepdim=True)
    p2o = p2
    if mut == "p16_last_ignored" and P == 16:
        p2o = p2.clone()
        p2o[..., P - 1] = 0
    o = (cb + _emu_conv(v, w, mut=mut)) + p2o @ va
    if mut == "chunk_last_token_unwritten" and T >= CH:
        o = o.clone()
        o[:, :, CH - 1] = float("nan")
    # stage-2 backward
    sc = (q @ tr(A)) * scale
    eb = torch.exp(sc - sc.max(-1, keepdim=True).values)
    pb = eb / eb.sum(-1, keepdim=True)
    dp = g @ tr(va)
    dl = (pb * dp).sum(-1, keepdim=True)
    ds = pb * (dp - dl)
    dq = (ds * scale) @ A
    dVa = fold(torch.einsum("bhctp,bhctd->bhcpd", ch(pb), gc))
    dA2 = fold(scale * torch.einsum("bhctp,bhctd->bhcpd", ch(ds), qc))
    delta1 = (dVa * va).sum(-1)
    if mut == "delta1_neighbour":
        delta1 = torch.roll(delta1, 1, -1)
    # stage-1 backward
    pr = torch.exp(tr((k @ tr(A)) * scale) - M.unsqueeze(-1)) / L.unsqueeze(-1)          # (B, H, P, T)
    d1 = pr * (dVa @ tr(v) - delta1.unsqueeze(-1))
    dk = tr(d1 * scale) @ A
    dv = _emu_conv(g, w, flip=True, mut=mut) + tr(pr) @ dVa
    pa1 = scale * torch.einsum("bhctp,bhctd->bhcpd", ch(tr(d1)), kc)
    dA = dA2
    for c in range(NC):
        dA = dA + pa1[:, :, c]
    if mut != "dA_not_divided":
        dA = dA / lens
    dq = dq + tr(mem) @ dA
    # convolution gradients: per-(b, h, chunk) partials, then the reduction
    vp = F.pad(v, (0, 0, 1, 1, 1, 1))
    taps = torch.stack([ch(g * vp[:, a:a + H, b:b + T, :]).sum(3) for a in range(3) for b in range(3)], 3)   # (B, H, NC, 9, D)
    drop = mut == "reduce_row_missing"
    dw = emu_reduce(taps.reshape(B * H * NC, 9 * D), drop).view(9, D).t().reshape(D, 1, 3, 3)
    db = emu_reduce(gc.sum(3).reshape(B * H * NC, D), drop)
    return {"agents": A, "vagent": va, "M": M, "L": L, "o": o, "dq": dq, "dk": dk, "dv": dv, "dconv_w": dw, "dconv_b": db}
