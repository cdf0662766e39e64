"""The f32 attention core on the GPU, every dispatch path, held per element to the bounds of tests/attn_f32_ref.py:
every element of o, lse, dq, dk and dv, no exclusions, J = 1 included.

A path is a setting of the ops switches (PATHS); what it must launch is worked out from the dispatch in amk/ops.py and
csrc/attn_fwd.hip, attn_bwd.hip, attn_bwd_fused.hip (expected_kernels) and asserted twice: every bound case checks the
launch names ops.KERNEL_EVENTS records (forward flavour, kept scores or not, one-pass or recompute backward), and
test_path_launches_its_kernels runs the same call under the profiler and checks the kernels' template arguments.

Every path runs `diffuse` inputs x {none, both, dead_rows} x every shape (SHAPES: the smallest that cross the 32-row wave
tiles, the 64-key tiles, the 128-query workgroups and the 128 / 256 keys of a backward workgroup), j1_masked at one key
and dead_batch at (2, 1, 5, 300); one representative path per kernel file runs every other family and mask at
(1, 2, 130, 257).  ops.attention alternates between the two layouts from case to case; ops.attention_fused_kv runs once
per forward flavour.  The worst |got - ref| / bound per (path, tensor) is printed by test_zz_report."""
import pytest
import torch

import attn_f32_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 2, 33, 65), (1, 2, 130, 257), (1, 1, 257, 130), (2, 1, 5, 300)]
BIG = (1, 2, 130, 257)
BASE_MASKS = ("none", "both", "dead_rows")
OTHER_MASKS = ("key", "triu", "causal", "dead_batch", "j1_masked")
SWITCHES = ("ATTENTION_FORWARD", "ATTENTION_KEEP_SCORES", "ATTENTION_BACKWARD_KEYS", "DETERMINISTIC_ATTENTION_BACKWARD",
            "ATTENTION_BACKWARD_TWO_KERNEL", "ATTENTION_BACKWARD_X6")


def _path(D, fwd="f32", keep=True, keys=0, det=False, two=False, bwdx6="0", model="f32"):
    return dict(D=D, fwd=fwd, keep=keep, keys=keys, det=det, two=two, bwdx6=bwdx6, model=model)


PATHS = {
    # head dim 64: f32 forward (masked / plain by the case's mask), scores kept or not, one-pass backward at 128 / 256 keys
    "f32-kept-128": _path(64, keys=128),
    "f32-recompute-128": _path(64, keep=False, keys=128),
    "f32-kept-256": _path(64, keys=256),
    "f32-recompute-256": _path(64, keep=False, keys=256),
    # the same four forwards on split-bf16 MFMA, in front of the f32 one-pass backward
    "x6fwd-kept-128": _path(64, fwd="bf16x6", keys=128, model="x6fwd"),
    "x6fwd-recompute-256": _path(64, fwd="bf16x6", keep=False, keys=256, model="x6fwd"),
    # reproducible dq: direct stores (J <= keys per workgroup) or per-key-block partials + reduce
    "f32-repro-128": _path(64, keys=128, det=True),
    "f32-repro-recompute-256": _path(64, keep=False, keys=256, det=True),
    # the split-bf16 backward (kept scores, 256 keys), behind either forward
    "f32-x6bwd": _path(64, keys=256, bwdx6="1", model="x6bwd"),
    "x6fwd-x6bwd": _path(64, fwd="bf16x6", keys=256, bwdx6="1", model="x6"),
    # the two recompute kernels (attn_generic.h), all eight head dims; 32 / 128: one-pass too (128: kept where unmasked)
    "d64-two-kernel": _path(64, two=True),
    "d32-fused": _path(32),
    "d32-two-kernel": _path(32, two=True),
    "d128-fused-kept": _path(128),
    "d128-fused-recompute": _path(128, keep=False),
    "d128-two-kernel": _path(128, two=True),
    "d96": _path(96),
    "d160": _path(160),
    "d192": _path(192),
    "d224": _path(224),
    "d256": _path(256),
}
# one path per kernel file for the other families and masks: attn_fwd.hip + attn_bwd_fused.hip, attn_fwd_x6.hip +
# attn_bwd_fused_x6.hip, attn_generic.h at head dim 64 (attn_bwd.hip's instantiation), 128 and 256
REPRESENTATIVE = ("f32-kept-128", "x6fwd-x6bwd", "d64-two-kernel", "d128-fused-kept", "d256")
KNOWN = ("attn_fwd_kernel", "attn_fwd_plain_kernel", "attn_fwd_x6_kernel", "attn_fwd_x6_plain_kernel", "attn_split_kv_kernel",
         "attn_fwd_gen_kernel", "attn_fwd_gen_plain_kernel", "attn_bwd_delta_gen_kernel", "attn_bwd_dkdv_gen_kernel",
         "attn_bwd_dq_gen_kernel", "attn_bwd_fused_kernel", "attn_bwd_fused_x6_kernel", "attn_bwd_dq_reduce_kernel")


def _cases():
    for name in PATHS:
        for si, shape in enumerate(SHAPES):
            for mi, mask in enumerate(BASE_MASKS):
                yield name, "diffuse", mask, shape, ("bthd", "bhtd")[(si + mi) % 2]
        yield name, "diffuse", "j1_masked", SHAPES[0], "bhtd"
        yield name, "diffuse", "dead_batch", SHAPES[4], "bthd"
    for name in REPRESENTATIVE:
        for fi, family in enumerate(ref.FAMILIES[1:]):
            yield name, family, "none", BIG, ("bthd", "bhtd")[fi % 2]
            yield name, family, "both", BIG, ("bhtd", "bthd")[fi % 2]
        for mi, mask in enumerate(OTHER_MASKS):
            yield name, "diffuse", mask, BIG, ("bthd", "bhtd")[mi % 2]


def _id(case):
    name, family, mask, shape, layout = case
    return f"{name}-{family}-{mask}-{'x'.join(map(str, shape))}-{layout}"


@pytest.fixture
def switches():
    """Sets the ops switches of a path and puts back what was there."""
    from amk import ops

    old = {s: getattr(ops, s) for s in SWITCHES}
    old_events = ops.KERNEL_EVENTS

    def apply(P):
        ops.ATTENTION_FORWARD = P["fwd"]
        ops.ATTENTION_KEEP_SCORES = P["keep"]
        ops.ATTENTION_BACKWARD_KEYS = P["keys"]
        ops.DETERMINISTIC_ATTENTION_BACKWARD = P["det"]
        ops.ATTENTION_BACKWARD_TWO_KERNEL = P["two"]
        ops.ATTENTION_BACKWARD_X6 = P["bwdx6"]

    yield apply
    for s, v in old.items():
        setattr(ops, s, v)
    ops.KERNEL_EVENTS = old_events


def expected_kernels(P, km, cm, I, J):
    """What the dispatch must launch for this path and call: ({kernel: leading template arguments or None}, the launch
    names ops.KERNEL_EVENTS records).  Read from ops._attn_forward (keepable), ops._attn_backward, attn_fwd_impl
    (csrc/attn_fwd.hip), launch_attn_fwd_x6, launch_fwd_gen_dh / launch_bwd_gen_dh and launch_attn_bwd_fused."""
    D, det, two = P["D"], P["det"], P["two"]
    masked, causal = km is not None or cm is not None, cm is not None
    keepable = D == 64 or (D == 128 and not masked and not det)
    kept = P["keep"] and keepable and not two
    x6f = D == 64 and P["fwd"] == "bf16x6"
    k = {}
    if D == 64:
        base = "attn_fwd_x6" if x6f else "attn_fwd"
        if not masked:
            k[base + "_plain_kernel"] = [kept]
        else:
            k[base + "_kernel"] = [causal, kept] if x6f else [causal, not causal, kept]
        if x6f:
            k["attn_split_kv_kernel"] = None
    elif masked:
        k["attn_fwd_gen_kernel"] = [D, causal]
    else:
        k["attn_fwd_gen_plain_kernel"] = [D, kept]
    k["attn_bwd_delta_gen_kernel"] = [D]
    fused = not two and D in (32, 64, 128) and not (det and D != 64)
    if fused:
        keys = P["keys"] or (256 if J >= 256 else 128)
        if P["bwdx6"] == "1" and kept and D == 64 and keys == 256:
            k["attn_bwd_fused_x6_kernel"] = [int(det), causal]
        else:
            nw, qs = {32: (8, 2), 128: (4, 1)}.get(D, (8 if keys == 256 else 4, 1))
            k["attn_bwd_fused_kernel"] = [D, nw, qs, kept, int(det), causal]
        if det and J > (32 * 8 if keys == 256 else 32 * 4):
            k["attn_bwd_dq_reduce_kernel"] = None
    else:
        k["attn_bwd_dkdv_gen_kernel"] = [D, causal]
        k["attn_bwd_dq_gen_kernel"] = [D, causal]
    events = {("attn_fwd_x6" if x6f else "attn_fwd") + ("_keep_kernel" if kept else "_kernel"),
              "attn_bwd_dkdv+dq" if two else ("attn_bwd_fused_kernel(kept scores)" if kept else "attn_bwd_fused_kernel")}
    return k, events


def _template_forms(args):
    dem = "<" + ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in args)
    man = "I" + "".join(f"Lb{int(a)}E" if isinstance(a, bool) else f"Li{a}E" for a in args)
    return dem, man


_REFS = {}


def _reference(family, shape, mask, D, model):
    """Inputs, masks and the fp64 reference with its bounds; the fp64 core is computed once per (family, shape, mask, D)
    and shared by the product models."""
    B, H, I, J = shape
    key = (family, shape, mask, D)
    if key not in _REFS:
        seed = 131 * D + 7 * I + J + 3 * ref.FAMILIES.index(family)
        scale = D ** -0.5
        q, k, v, d_o = ref.make_inputs(family, B, H, I, J, D, scale, seed)
        km, cm = ref.make_masks(mask, B, I, J, seed)
        _REFS[key] = dict(inputs=(q, k, v, d_o), scale=scale, km=km, cm=cm,
                          core=ref.fp64_core(q, k, v, d_o, scale, km, cm), bounds={})
    c = _REFS[key]
    if model not in c["bounds"]:
        c["bounds"][model] = ref.reference(*c["inputs"], c["scale"], c["km"], c["cm"], model=model, core=c["core"])
    return c, c["bounds"][model]


def _run(device, monkeypatch, c, layout, fused_kv=False):
    """One forward and backward through ops.attention (or ops.attention_fused_kv): {"o", "lse", "dq", "dk", "dv"}."""
    from amk import ops

    seen = {}
    forward = ops._attn_forward

    def spy(*a, **kw):
        r = forward(*a, **kw)
        seen["stats"] = r[4]
        return r

    monkeypatch.setattr(ops, "_attn_forward", spy)
    q, k, v, d_o = c["inputs"]
    B, H, I, D = q.shape
    J = k.shape[2]
    km = None if c["km"] is None else c["km"].to(device)
    cm = None if c["cm"] is None else c["cm"].to(device)
    if fused_kv:
        q2 = q.permute(0, 2, 1, 3).reshape(B, I, H * D).to(device).requires_grad_(True)
        kv2 = torch.stack([k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)], dim=2).reshape(B, J, 2 * H * D).to(device).requires_grad_(True)
        o2 = ops.attention_fused_kv(q2, kv2, H, D, c["scale"], key_mask=km, causal_mask=cm)
        dq2, dkv2 = torch.autograd.grad((o2 * d_o.permute(0, 2, 1, 3).reshape(B, I, H * D).to(device)).sum(), [q2, kv2])
        dkv = dkv2.view(B, J, 2, H, D)
        got = dict(o=o2.view(B, I, H, D).permute(0, 2, 1, 3), dq=dq2.view(B, I, H, D).permute(0, 2, 1, 3),
                   dk=dkv[:, :, 0].permute(0, 2, 1, 3), dv=dkv[:, :, 1].permute(0, 2, 1, 3))
    else:
        def to_dev(t):
            t = t.to(device)
            if layout == "bthd":   # (B, T, H, D) storage viewed as (B, H, T, D): the projection layout
                t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
            return t.requires_grad_(True)

        qd, kd, vd = to_dev(q), to_dev(k), to_dev(v)
        o = ops.attention(qd, kd, vd, c["scale"], key_mask=km, causal_mask=cm)
        dq, dk, dv = torch.autograd.grad((o * d_o.to(device)).sum(), [qd, kd, vd])
        got = dict(o=o, dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    got["lse"] = ref.lse_of(seen["stats"])
    return got


def _bound_case(device, monkeypatch, switches, name, family, mask, shape, layout, fused_kv=False):
    from amk import ops

    P = PATHS[name]
    c, R = _reference(family, shape, mask, P["D"], P["model"])
    switches(P)
    ops.KERNEL_EVENTS = {}
    got = _run(device, monkeypatch, c, layout, fused_kv)
    launched = set(ops.KERNEL_EVENTS)
    ops.KERNEL_EVENTS = None
    _, events = expected_kernels(P, c["km"], c["cm"], shape[2], shape[3])
    assert launched == events, (name, launched, events)
    res = ref.assert_within(got, R, path=name, what=f"{family}/{mask}/{shape}/{layout}")
    print(name, family, mask, shape, layout, {n: f"{w:.3f}" for n, (_, w) in res.items()})


@pytest.mark.parametrize("case", list(_cases()), ids=_id)
def test_every_element_within_its_bound(device, monkeypatch, switches, case):
    _bound_case(device, monkeypatch, switches, *case)


@pytest.mark.parametrize("D,mask", [(32, "none"), (32, "causal"), (128, "causal")], ids=lambda x: str(x))
def test_kept_scores_backward_that_ops_never_asks_for(device, switches, D, mask):
    """The library keeps scores at head dims 32 and 128 where the call has no mask (csrc/attn_fwd.hip:541-544; launch_fwd_gen_dh,
    csrc/attn_generic.h:852: attn_fwd_gen_plain_kernel<D, true>), and its one-pass backward reads kept scores at those head
    dims with or without a causal mask (csrc/attn_bwd_fused.hip:497 and :511-512).  amk/ops.py keeps none at head dim 32
    and none under a mask (`keepable` in ops._attn_forward), so attn_fwd_gen_plain_kernel<32, true> and
    attn_bwd_fused_kernel<32, 8, 2, true, 0, false / true> and <128, 4, 1, true, 0, true> run through the C ABI only.
    Kept scores are the raw scores, before any mask, so the scores of the unmasked forward serve the masked problem: o
    and the row statistics come from amk_attn_fwd under the case's own mask, the backward from amk_attn_bwd_kept on both,
    and every element is held to the family's bounds (attn_f32_ref, model f32)."""
    from amk import lib, ops

    switches(_path(D, keep=False))
    L, nan = lib.load(), float("nan")
    B, H, I, J = BIG
    c, R = _reference("diffuse", BIG, mask, D, "f32")
    bthd = lambda t: t.to(device).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)   # noqa: E731  (the dense dq layout)
    q, k, v, d_o = (bthd(t) for t in c["inputs"])
    cm = ops._mask_u8(None if c["cm"] is None else c["cm"].to(device), (I, J), "causal_mask")
    assert c["km"] is None and (cm is not None) == (mask == "causal")
    qv, kv, vv = (ops._as_kernel_view(t) for t in (q, k, v))
    o0, stats0 = ops._new_bthd(B, H, I, D, qv), torch.full((B, H, I, 2), nan, device=device)
    scores = torch.full((L.amk_attn_scores_bytes(B, H, I, J) // 4,), nan, device=device)
    rc = L.amk_attn_fwd_keep(ops._ptr(qv), ops._ptr(kv), ops._ptr(vv), ops._ptr(o0), ops._ptr(stats0), ops._ptr(scores),
                             ops._NULL, ops._NULL, B, H, I, J, D, *ops._strides4(qv), *ops._strides4(kv), *ops._strides4(vv),
                             *ops._strides4(o0), float(c["scale"]), ops._stream())
    lib.check(rc, "amk_attn_fwd_keep")
    qv, kv, vv, o, stats, kept = ops._attn_forward(q, k, v, None, cm, c["scale"])      # the case's own mask; nothing kept
    assert kept is None
    if mask == "none":      # the keeping forward's own o and statistics (it subtracts a running maximum, the plain one a lazy
        o, stats = o0, stats0      # reference, csrc/attn_fwd.hip:287-296: the two differ in the last bits)
    dq, dk, dv = (torch.full_like(t, nan) for t in (qv, kv, vv))
    assert dq.stride() == (I * H * D, D, H * D, 1)
    ops._attn_backward(qv, kv, vv, o, stats, d_o, dq, dk, dv, None, cm, c["scale"], stages=ops.ATTN_BWD_FAST, scores=scores)
    torch.cuda.synchronize()
    got = dict(o=o, lse=ref.lse_of(stats), dq=dq, dk=dk, dv=dv)
    res = ref.assert_within(got, R, path=f"d{D}-kept-abi", what=f"diffuse/{mask}/{BIG}")
    print(D, mask, {n: f"{w:.3f}" for n, (_, w) in res.items()})


# one attention_fused_kv case per forward flavour: f32 and split-bf16 x masked and plain x kept and not, the generic
# forward masked and plain, and head dim 128's keeping forward; its backward writes dk and dv into one buffer
FUSED_KV = [("f32-kept-128", "none"), ("f32-kept-128", "both"), ("f32-recompute-256", "none"), ("f32-recompute-256", "both"),
            ("x6fwd-kept-128", "none"), ("x6fwd-x6bwd", "both"), ("x6fwd-recompute-256", "none"),
            ("x6fwd-recompute-256", "both"), ("d96", "none"), ("d96", "both"), ("d128-fused-kept", "none")]


@pytest.mark.parametrize("name,mask", FUSED_KV, ids=lambda x: str(x))
def test_fused_kv_entry_within_its_bound(device, monkeypatch, switches, name, mask):
    _bound_case(device, monkeypatch, switches, name, "diffuse", mask, BIG, "bthd", fused_kv=True)


def _launch_cases():
    for name, P in PATHS.items():
        for mask in ("none", "key", "both"):
            yield name, mask, BIG
        if P["det"] or (P["D"] == 64 and not P["keys"] and not P["two"]):
            yield name, "none", SHAPES[1]    # J = 65: one key block (direct dq stores; 128 keys per workgroup by default)


@pytest.mark.parametrize("name,mask,shape", list(_launch_cases()), ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_path_launches_its_kernels(device, monkeypatch, switches, name, mask, shape):
    """The kernels the profiler sees for a path are exactly the ones expected_kernels works out, template arguments
    (head dim, waves, kept scores, reproducible dq, causal) included."""
    from torch.profiler import ProfilerActivity, profile

    P = PATHS[name]
    c, _ = _reference("diffuse", shape, mask, P["D"], P["model"])
    switches(P)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        _run(device, monkeypatch, c, "bthd")
    names = sorted({e.name for e in prof.events() if "attn_" in e.name})
    want, _ = expected_kernels(P, c["km"], c["cm"], shape[2], shape[3])
    ran = {base for base in KNOWN if any(base in n for n in names)}
    assert ran == set(want), (name, mask, sorted(ran), sorted(want), names)
    for base, args in want.items():
        if args is None:
            continue
        dem, man = _template_forms(args)
        hits = [n for n in names if base in n]
        assert all(n[n.index(base) + len(base):].startswith((dem, man)) for n in hits), (base, args, hits)


def test_zz_report():
    """The worst |got - ref| / bound per (path, tensor) over this process's cases (run with -s to see it)."""
    assert ref.WORST, "no bound case ran before the report"
    print("\npath".ljust(28) + "".join(n.rjust(9) for n in ref.NAMES))
    for name in PATHS:
        if any((name, n) in ref.WORST for n in ref.NAMES):
            print(name.ljust(27) + "".join(f"{ref.WORST.get((name, n), float('nan')):9.4f}" for n in ref.NAMES))
    assert max(ref.WORST.values()) <= 1.0
