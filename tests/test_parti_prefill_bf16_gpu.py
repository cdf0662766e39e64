"""Prompted KV-cached decoding under bf16 autocast on the GPU: ``prefill`` on a bf16 decode state (amk_attn_prefill_bf16,
the step's bf16 arithmetic on n rows) and the steps that follow it against the fp64 logits, relative to the causal
forward under the same autocast -- the caps of tests/test_parti_decode_bf16_gpu.py, 1.5 max and 1.25 rms.  The test
prints the ratios it measures; DESIGN.md section 4i records them."""
import pytest
import torch

from test_parti_decode_bf16_gpu import BF16, MAX_CAP, NAMES, RMS_CAP, _autocast, _Case, _dev

pytestmark = pytest.mark.gpu


def _prefill_then_steps(c, state, n):
    """(B, T, V): ``prefill`` of the first n tokens with every row's logits, then teacher-forced steps to the end."""
    m = c.m
    tokens = c.ids[:, :n]
    rows = m.prefill(state, tokens, all_logits=True)
    first = rows.shape[1]                                 # Parti: n + 1 rows behind the start token
    rest = [m.next_logits(state, c.prev(t)) for t in range(first, c.T)]
    return torch.cat([rows] + [r.unsqueeze(1) for r in rest], dim=1)


@pytest.mark.parametrize("name", NAMES)
def test_prefill_then_steps_under_autocast(device, name):
    from amk import ops

    c = _Case(name, device)
    with _autocast():
        fwd = c.forward_logits()
    fmax, frms = _dev(fwd.float(), c.ref)
    for n in (1, 33, 65, c.T - 1):
        with _autocast():
            state = c.begin()
            ops.KERNEL_EVENTS = {}
            try:
                logits = _prefill_then_steps(c, state, n)
                torch.cuda.synchronize()
                names = set(ops.KERNEL_EVENTS)
            finally:
                ops.KERNEL_EVENTS = None
        assert state.dtype == BF16 and all(t.dtype == BF16 for t in state.self_kv + state.cross_kv)
        assert logits.dtype == torch.float32 and tuple(logits.shape) == (c.B, c.T, c.V)
        assert bool(torch.isfinite(logits).all())
        dmax, drms = _dev(logits, c.ref)
        print(f"{name} n {n}: prefill + steps max {dmax:.3e} rms {drms:.3e}; causal forward under autocast max {fmax:.3e} "
              f"rms {frms:.3e}; ratio max {dmax / fmax:.3f} rms {drms / frms:.3f}; kernels {sorted(names)}")
        assert dmax <= MAX_CAP * fmax, (n, dmax, fmax)
        assert drms <= RMS_CAP * frms, (n, drms, frms)
        assert "attn_prefill" in names and not any(k.startswith("attn_fwd") for k in names), names
        assert state.host_pos == c.T and int(state.pos.item()) == c.T


@pytest.mark.parametrize("name", NAMES)
def test_a_state_built_under_autocast_prefills_outside_it(device, name):
    c = _Case(name, device)
    n = 33
    with _autocast():
        inside = _prefill_then_steps(c, c.begin(), n)
        state = c.begin()
    outside = _prefill_then_steps(c, state, n)           # no autocast here: the bf16 state carries everything it reads
    assert outside.dtype == torch.float32
    assert torch.equal(inside, outside)
    with _autocast():                                    # the last row alone (the step's head, on the row GEMM)
        last = c.m.prefill(c.begin(), c.ids[:, :n])
        fmax, _ = _dev(c.forward_logits().float(), c.ref)
    assert last.dtype == torch.float32 and tuple(last.shape) == (c.B, c.V)
    row = n if c.parti else n - 1
    dmax, _ = _dev(last, c.ref[:, row])
    print(f"{name}: last row alone max {dmax:.3e}; causal forward under autocast, all rows, max {fmax:.3e}")
    assert dmax <= MAX_CAP * fmax, (dmax, fmax)
