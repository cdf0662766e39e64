"""A red-zone allocator for the out-of-bounds tests ("Red zones"), next to tests/poison.py.

``redzoned_empty(fill)`` replaces ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and
``torch.Tensor.new_empty`` -- the four names poison.py patches -- with wrappers that put every new tensor between two
canary margins, and ``check()`` of the object the context yields says whether anything wrote into a margin.  The
zero-initialising ``torch.zeros``, ``torch.zeros_like`` and ``torch.Tensor.new_zeros`` are wrapped in the same way (margins
by the rules below, the interior zero as before): GradReducer's buckets and FlatAdam's flat parameter, moment and shadow
buffers are allocated with them, and those are the buffers whose neighbour is another parameter.

    backing = one uint8 buffer of front + span + back bytes        (span: the byte length of the tensor's own storage)
    tensor  = the dtype, shape, strides and storage offset the unpatched allocator chose, on backing[front:front + span]

    front = back = min(max(4096, round_up(span, 512)), 1 MiB)

The front margin is a multiple of 512 bytes, so the tensor keeps the 512-byte alignment torch's caching allocator gives
every block and each ``data_ptr() % 16`` gate of amk takes the branch it takes without the patch.  The back margin begins
at the tensor's last byte: the rounding slack that hides a one-row overrun in an ordinary run is canary here.  The size is
a choice, not a measurement: one whole tensor on either side for anything under 1 MiB, so a store at a wrong tile index of
the same buffer still lands in canary.

The tensor handed out is what ``backing[front:front + span].view(dtype).as_strided(shape, strides, offset)`` addresses,
made with ``Tensor.set_`` on the backing storage and not as a view: an autograd view of a buffer would make every in-place
op on an op's output, and every custom Function that returns one, answer for a base tensor that amk never sees.

Fill (``fill`` as in poison.py: "nan" = 0xFF, "big" = 0x7F):

  * f32, bf16 and f64 tensors, and uint8 workspaces allocated on poison.UINT8_FLOAT_SITES: the whole backing buffer is
    filled, interior included, so a red-zone run is a superset of a poison run; the margins' value differs between the two
    fills, so an element read past the end of a buffer reaches the result as a value that the comparison of the fills sees
    (poison.assert_fill_independent).
  * every other dtype (integer, bool, other uint8): the interior is left exactly as the allocator returned it, and BOTH
    MARGINS ARE ZERO under both fills.  A stale index must not become a wild address, and index 0 is valid wherever a row
    exists: nothing here may make a kernel fault.  The price: a stray write of zeros into an integer margin is not seen.

Caller inputs: while the context is active ``torch.Tensor.to`` and ``torch.Tensor.cuda`` are wrapped.  A call on a CPU
tensor whose result is a tensor on a covered device returns a red-zoned copy of that result (``guarded_copy``): same
margins, same fill rule, zero margins for integer and bool.  ``nn.Module.to`` goes through the same wrapper (its
parameters are moved under no_grad and assigned with ``param.data = ...``), so a module built on the CPU and moved inside
the context has red-zoned parameters.  A result that requires grad (a differentiable move of a CPU leaf) is passed through
unguarded: a copy would cut it from its graph.  Every other call goes straight to the original.

Registry: the context keeps (backing, front, span, margin byte, call site, dtype, shape) of every buffer with a strong
reference until it exits, so no red zone is recycled before it is checked.  One consequence: ops._attn_forward hangs the
release of its kept-scores accounting on the storage of the scores, which now lives until the context exits -- the bytes
are released then and not at free; at the sizes of the tests the budget of a quarter of device memory is never near.

What check() cannot see: a write of the margin's own byte value (hence run_both always checks under both fills), a write
beyond the margin, zeros written into an integer margin, a read past the end that a select discards, anything torch or a
vendor library allocates for itself, and inputs that reach the device by any other road than .to / .cuda in the context.
"""
import collections
import contextlib

import torch

from poison import FILL_BYTE, FLOAT_DTYPES, UINT8_FLOAT_SITES, _caller_site

MARGIN_MIN, MARGIN_MAX = 4096, 1 << 20
CHECKED = collections.Counter()      # buffers / margin bytes that check() has compared so far in this process

Entry = collections.namedtuple("Entry", "backing front span byte site dtype shape")


def margin(span):
    """Bytes of canary on either side of a tensor whose storage is `span` bytes long."""
    return min(max(MARGIN_MIN, -(-span // 512) * 512), MARGIN_MAX)


class RedZones:
    """What redzoned_empty yields: the registry, check(), and guarded_copy bound to this context."""

    def __init__(self, fill, devices, orig):
        self.fill, self.devices, self.byte, self._orig = fill, devices, FILL_BYTE[fill], orig
        self.registry = []

    def covers(self, t):
        return (isinstance(t, torch.Tensor) and (t.is_cuda or self.devices == "all") and t.numel() > 0
                and t.layout == torch.strided and not t.is_quantized)

    def guard(self, t, site, zero=False):
        """A tensor of t's dtype, shape, strides and storage offset between two margins.  t is fresh from an allocator: it
        owns its storage, whose length is the span.  The interior is filled (float rule) or as allocated (integer rule);
        zero: it is zeroed afterwards (the zero-initialising allocators)."""
        span = t.untyped_storage().nbytes()
        item = t.element_size()
        front = back = margin(span)
        backing = self._orig["empty"](front + span + back, dtype=torch.uint8, device=t.device)
        if t.dtype in FLOAT_DTYPES or (t.dtype == torch.uint8 and site in UINT8_FLOAT_SITES):
            byte = self.byte
            backing.fill_(byte)
        else:
            byte = 0
            backing[:front].zero_()
            backing[front + span:].zero_()
        if zero:
            backing[front:front + span].zero_()
        out = self._orig["empty"](0, dtype=t.dtype, device=t.device)
        out.set_(backing.untyped_storage(), front // item + t.storage_offset(), t.shape, t.stride())
        self.registry.append(Entry(backing, front, span, byte, site, t.dtype, tuple(t.shape)))
        return out.requires_grad_(t.requires_grad)

    def guarded_copy(self, t, device=None, site=None):
        """t moved to `device` (default: where it is) as a red-zoned copy, whether or not the device is a covered one."""
        res = self._orig["to"](t.detach(), device) if device is not None else t.detach()
        if res.numel() == 0 or res.layout != torch.strided:
            return res
        out = self.guard(self._orig["empty_like"](res), site or _caller_site(2))
        out.copy_(res)
        return out

    def check(self):
        """Both margins of every buffer made so far against their byte; one AssertionError that names every damaged one."""
        if torch.cuda.is_available() and any(e.backing.is_cuda for e in self.registry):
            torch.cuda.synchronize()
        flags = collections.defaultdict(list)
        for i, e in enumerate(self.registry):      # on the device: one bool per margin, one transfer per device
            b = e.backing
            flags[b.device].append((i, "front", (b[:e.front] != e.byte).any()))
            flags[b.device].append((i, "back", (b[e.front + e.span:] != e.byte).any()))
            CHECKED["buffers"] += 1
            CHECKED["margin_bytes"] += b.numel() - e.span
        damaged = []
        for rows in flags.values():
            hit = torch.stack([f for _, _, f in rows]).cpu().tolist()
            damaged += [(i, side) for (i, side, _), h in zip(rows, hit) if h]
        lines = []
        for i, side in sorted(damaged):
            e = self.registry[i]
            zone = e.backing[:e.front] if side == "front" else e.backing[e.front + e.span:]
            at = (zone != e.byte).nonzero().flatten()
            first, last = int(at[0]), int(at[-1])
            if side == "front":      # relative to the tensor's first byte: -1 is the byte just before it
                first, last, rel = first - e.front, last - e.front, "start"
            else:                    # relative to the tensor's end: +0 is the first byte past it
                rel = "end"
            lines.append(f"{e.site[0]}:{e.site[1]}: {e.dtype} {e.shape}: {side} margin damaged, {at.numel()} bytes in "
                         f"{first:+d}..{last:+d} relative to the tensor's {rel} (span {e.span} bytes, margin value "
                         f"0x{e.byte:02X})")
        if lines:
            raise AssertionError(f"red zones under the {self.fill!r} fill, {len(lines)} damaged of "
                                 f"{2 * len(self.registry)} margins:\n  " + "\n  ".join(lines))


_ACTIVE = []
# what is patched: name -> (owner, is a method, zero-initialising).  The four names of poison.py; the three zero-initialising
# allocators, because GradReducer's buckets and FlatAdam's flat parameter, moment and shadow buffers come from torch.zeros
# and torch.zeros_like (amk/dp.py, amk/optim.py) -- the buffers whose neighbour is another parameter; and the two moves.
ALLOCATORS = dict(empty=(torch, False, False), empty_like=(torch, False, False), empty_strided=(torch, False, False),
                  new_empty=(torch.Tensor, True, False), zeros=(torch, False, True), zeros_like=(torch, False, True),
                  new_zeros=(torch.Tensor, True, True))
MOVES = ("to", "cuda")


def guarded_copy(t, device=None):
    """RedZones.guarded_copy of the innermost active redzoned_empty context."""
    if not _ACTIVE:
        raise RuntimeError("guarded_copy: no redzoned_empty context is active")
    return _ACTIVE[-1].guarded_copy(t, device, _caller_site(2))


@contextlib.contextmanager
def redzoned_empty(fill, devices="gpu"):
    """Patch the allocators and Tensor.to / Tensor.cuda for the duration of the block; the originals come back on exit,
    also after an exception.  devices: "gpu" (only device tensors get red zones) or "all" (CPU tensors too, and a .to() of
    a CPU tensor always returns a red-zoned copy: the helper's own tests).  Yields the RedZones object."""
    if fill not in FILL_BYTE:
        raise ValueError(f"redzoned_empty: fill must be 'nan' or 'big', got {fill!r}")
    if devices not in ("gpu", "all"):
        raise ValueError(f"redzoned_empty: devices must be 'gpu' or 'all', got {devices!r}")
    found = {name: getattr(owner, name) for name, (owner, _, _) in ALLOCATORS.items()}
    found.update({name: getattr(torch.Tensor, name) for name in MOVES})
    orig = _ACTIVE[-1]._orig if _ACTIVE else found      # nested: allocate with the real ones, not through the outer context
    rz = RedZones(fill, devices, orig)

    def allocator(name, zero):
        def wrapper(*args, **kwargs):
            t = orig[name](*args, **kwargs)
            return rz.guard(t, _caller_site(2), zero) if rz.covers(t) else t
        return wrapper

    def move(name):
        def wrapper(self, *args, **kwargs):
            res = orig[name](self, *args, **kwargs)
            if isinstance(self, torch.Tensor) and self.device.type == "cpu" and rz.covers(res) and not res.requires_grad:
                return rz.guarded_copy(res, None, _caller_site(2))
            return res
        return wrapper

    for name, (owner, _, zero) in ALLOCATORS.items():
        setattr(owner, name, allocator(name, zero))
    for name in MOVES:
        setattr(torch.Tensor, name, move(name))
    _ACTIVE.append(rz)
    try:
        yield rz
    finally:
        _ACTIVE.remove(rz)
        for name, (owner, _, _) in ALLOCATORS.items():
            setattr(owner, name, found[name])
        for name in MOVES:
            setattr(torch.Tensor, name, found[name])
        rz.registry.clear()


def run_both(case, devices="gpu"):
    """The red-zone counterpart of poison.run_both_fills: case() -> dict of tensors, run once under each fill from identical
    inputs, check() before each context is left.  Returns the two result dicts, cloned."""
    out = {}
    for fill in ("nan", "big"):
        with redzoned_empty(fill, devices=devices) as rz:
            res = case()
            out[fill] = {k: v.detach().clone() for k, v in res.items() if v is not None}
            rz.check()
    return out["nan"], out["big"]
