"""An allocation poisoner for the stale-memory tests ("Stale memory").

``poisoned_empty(fill)`` replaces ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and
``torch.Tensor.new_empty`` with wrappers that allocate as before and then fill the new tensor's whole storage with one
byte value, so that an element a kernel reads without having written it shows up as a *value* in the result:

    "nan"   every byte 0xFF: f32 0xFFFFFFFF, bf16 0xFFFF and f64 read as NaN
    "big"   every byte 0x7F: f32 0x7F7F7F7F = 3.39e38, bf16 0x7F7F the same, f64 1.38e306 -- large and finite

amk looks these names up on the torch module at call time, so the patch reaches every allocation site of amk/ops.py,
amk/dense.py and amk/optim.py; torch's own C++ allocations are not affected.  The fill is ordinary stream work: inside
a graph capture it becomes a node of the graph, and every replay poisons again.

What is filled: f32, bf16 and f64 tensors on a GPU (on any device with devices="all", for the CPU tests).  Integer, bool
and index tensors are left as allocated -- a stale value there could become a wild address, and nothing here is meant
to make a kernel fault.  A uint8 buffer is filled only when the call site is on UINT8_FLOAT_SITES: byte workspaces that
hold floating-point data only.
"""
import contextlib
import os
import sys

import torch

FILL_BYTE = {"nan": 0xFF, "big": 0x7F}
FLOAT_DTYPES = (torch.float32, torch.bfloat16, torch.float64)

# (file, function) of the torch.empty(..., dtype=torch.uint8) calls whose buffer holds floating-point data only, with the
# source line that shows it.  These are all the uint8 allocations of amk (masks come from .to(torch.uint8), not from empty).
UINT8_FLOAT_SITES = {
    # the split-bf16 attention forward's workspace: "__bf16* out = reinterpret_cast<__bf16*>(p.x6_ws) + ..." -- the pre-pass
    # writes K planes and V^T planes, 24 KB each per 64-key tile (csrc/attn_fwd_x6.hip:420, layout at :139-140), and the
    # forward reads them back as bf16 fragments (:143-159)
    ("ops.py", "_attn_forward"): "csrc/attn_fwd_x6.hip:420",
    # the per-call plane buffer of gemm_x6_nt: amk_gemm_x6_split hands it to split_planes_kernel as
    # static_cast<__bf16*>(planes) (csrc/gemm_x6.hip:303); 3 * N * padded_k(K) bf16 elements (:291)
    ("ops.py", "gemm_x6_nt"): "csrc/gemm_x6.hip:303",
}


def _caller_site(depth):
    f = sys._getframe(depth)
    return os.path.basename(f.f_code.co_filename), f.f_code.co_name


@contextlib.contextmanager
def poisoned_empty(fill, devices="gpu"):
    """Patch the four allocators for the duration of the block; the originals come back on exit, also after an exception.
    devices: "gpu" (only device tensors are filled) or "all" (CPU tensors too: the helper's own tests)."""
    if fill not in FILL_BYTE:
        raise ValueError(f"poisoned_empty: fill must be 'nan' or 'big', got {fill!r}")
    if devices not in ("gpu", "all"):
        raise ValueError(f"poisoned_empty: devices must be 'gpu' or 'all', got {devices!r}")
    byte = FILL_BYTE[fill]
    orig = dict(empty=torch.empty, empty_like=torch.empty_like, empty_strided=torch.empty_strided,
                new_empty=torch.Tensor.new_empty)

    def poison(t, site):
        if not (t.is_cuda or devices == "all") or t.numel() == 0 or t.layout != torch.strided:
            return t
        if t.dtype in FLOAT_DTYPES or (t.dtype == torch.uint8 and site in UINT8_FLOAT_SITES):
            # the new tensor owns its storage: fill all of it, padding between strided rows included
            raw = orig["empty"](0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
            raw.fill_(byte)
        return t

    def empty(*args, **kwargs):
        return poison(orig["empty"](*args, **kwargs), _caller_site(2))

    def empty_like(*args, **kwargs):
        return poison(orig["empty_like"](*args, **kwargs), _caller_site(2))

    def empty_strided(*args, **kwargs):
        return poison(orig["empty_strided"](*args, **kwargs), _caller_site(2))

    def new_empty(self, *args, **kwargs):
        return poison(orig["new_empty"](self, *args, **kwargs), _caller_site(2))

    torch.empty, torch.empty_like, torch.empty_strided = empty, empty_like, empty_strided
    torch.Tensor.new_empty = new_empty
    try:
        yield
    finally:
        torch.empty, torch.empty_like, torch.empty_strided = orig["empty"], orig["empty_like"], orig["empty_strided"]
        torch.Tensor.new_empty = orig["new_empty"]


# ---------------------------------------------------------------------------- the comparison of the two fills
def run_both_fills(case, devices="gpu"):
    """case() -> dict of tensors, run once under each fill from identical inputs (the case seeds its own inputs)."""
    out = {}
    for fill in ("nan", "big"):
        with poisoned_empty(fill, devices=devices):
            res = case()
        out[fill] = {k: v.detach().clone() for k, v in res.items() if v is not None}
    return out["nan"], out["big"]


def assert_fill_independent(nan_run, big_run, what, tolerant=(), bound=None, allow_nan=()):
    """Every tensor of the two runs finite and bitwise equal.  tolerant: names whose equality is replaced by
    bound(name, a, b) (float-atomic paths); allow_nan: names that are documented to be NaN in both runs."""
    assert set(nan_run) == set(big_run), what
    for name, a in nan_run.items():
        b = big_run[name]
        if name in allow_nan:
            assert torch.isnan(a).all() and torch.isnan(b).all(), f"{what}: {name} is documented NaN"
            continue
        if a.is_floating_point():
            for fill, t in (("nan", a), ("big", b)):
                bad = int((~torch.isfinite(t)).sum())
                assert bad == 0, f"{what}: {name} has {bad} non-finite elements of {t.numel()} under the {fill!r} fill"
        if name in tolerant:
            bound(name, a, b)
            continue
        if not torch.equal(a, b):
            diff = int((a != b).sum())
            raise AssertionError(f"{what}: {name} differs between the fills in {diff} of {a.numel()} elements: "
                                 f"the result depends on memory the op never wrote")
