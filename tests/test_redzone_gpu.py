"""No kernel writes or reads outside the buffers amk allocates: every case of tests/test_stale_memory_gpu.py -- every
autograd entry point of amk.ops and the plain entry points next to them (the prefill attention on both cache types and the
guided logits head under both stores of its GEMM among them), on every forced path -- run under the red-zone allocator of
tests/redzone.py, once per fill, under the case's own switches and environment.  CASES is imported, so a family added to
the stale-memory sweep -- its guard, test_every_launcher_is_swept there, asks for one per new launcher -- runs here too.  Every torch.empty / empty_like /

empty_strided / new_empty of amk, and every input the case moves to the device, lies between two canary margins that begin
at the buffer's first and last byte.  For every case

  * check() passes in both runs: no margin of any output, workspace, saved tensor or input has a byte changed;
  * the results of the two runs are finite and BITWISE equal (poison.assert_fill_independent, with the stale-memory test's
    handling of the float-atomic rows: bounded, then bitwise in the reproducible mode).  The margins hold NaN in one run
    and 3.39e38 in the other, so an element read past the end of an input or a workspace and folded into a result shows
    here, as does -- the interiors are filled as poison.py fills them -- anything the stale-memory test sees.

The cases' references and the spy on the forced path are not repeated: tests/test_stale_memory_gpu.py holds them; this
file is about the ends of the buffers.  Two tests hold the method itself on the device (a stand-in overrun is caught; the
patch reaches amk's allocation sites), and one eager GAN step with the gradient penalty runs under the context: the one
place where the optimizer's flat buffers, the reducer's buckets and the double backward allocate next to each other.

Nothing here faults: every stand-in write stays inside a backing buffer the test owns, integer buffers keep their contents
and get zero margins.  What the method cannot see is listed in tests/redzone.py and DESIGN.md ("Red zones")."""
import pytest
import torch

from poison import assert_fill_independent
from redzone import redzoned_empty, run_both
from test_stale_memory_gpu import _PAIR_BOUND, _env, _switches, ATOMIC, CASES      # the names only: no test function is imported

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_no_access_outside_the_buffers(device, case):
    from amk import ops

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.backends.cudnn, "benchmark", False)
        mp.setattr(ops, "_SAMPLE_CALLS", ops._SAMPLE_CALLS)      # (the seeded sampling cases set it: put back afterwards)
        with _switches(**case.switches), _env(case.env):
            nan_run, big_run = run_both(lambda: case.fn(device))      # check() inside, under each fill
            row = ATOMIC[case.atomic] if case.atomic else None
            assert_fill_independent(nan_run, big_run, case.id, tolerant=row["tensors"] if row else (),
                                    bound=_PAIR_BOUND.get(case.atomic), allow_nan=case.allow_nan)
            if row is not None:      # the same case without atomics: bitwise, every tensor
                if row["repro"] == "torch_det":
                    old = torch.are_deterministic_algorithms_enabled()
                    torch.use_deterministic_algorithms(True)
                    try:
                        a, b = run_both(lambda: case.fn(device))
                    finally:
                        torch.use_deterministic_algorithms(old)
                else:
                    with _switches(**row["repro"]):
                        a, b = run_both(lambda: case.fn(device))
                assert_fill_independent(a, b, case.id + " (reproducible mode)", allow_nan=case.allow_nan)


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_a_stand_in_overrun_is_caught_on_the_device(device, fill):
    """Torch indexing stands in for an op whose tail store goes one element too far.  The write lands in the back margin of
    the op's own buffer: inside memory this test owns."""
    def op(n, extra):
        out = torch.empty(n, device=device)
        out.as_strided((n + extra,), (1,)).fill_(1.0)
        return out

    with redzoned_empty(fill) as rz:
        op(33, 0)
        rz.check()
        op(33, 1)
        with pytest.raises(AssertionError) as err:
            rz.check()
    msg = str(err.value)
    assert "test_redzone_gpu.py:op: torch.float32 (33,): back margin damaged, 4 bytes in +0..+3 relative to the tensor's end" in msg, msg
    assert "1 damaged of 4 margins" in msg, msg


def test_a_stand_in_read_past_an_input_is_caught_on_the_device(device):
    src = torch.arange(1.0, 34.0)

    def op(extra):
        x = src.to(device)
        return dict(y=x.as_strided((33 + extra,), (1,)).sum().reshape(1))

    good = run_both(lambda: op(0))
    assert_fill_independent(*good, "sum of n elements")
    assert float(good[0]["y"]) == float(src.sum())
    with pytest.raises(AssertionError, match="non-finite|differs between the fills"):
        assert_fill_independent(*run_both(lambda: op(1)), "sum of n + 1 elements")


def test_the_patch_reaches_the_allocation_sites_of_amk(device):
    """ops.layer_norm at the family's edge shape: the registry holds its output and its two statistics, allocated in
    amk/ops.py, and the inputs the case moved -- all 512-byte aligned as the caching allocator leaves them."""
    case = next(c for c in CASES if c.family == "layer_norm" and c.kind == "edge")
    with redzoned_empty("nan") as rz:
        res = case.fn(device)
        M, D = res["y"].shape
        mine = [e for e in rz.registry if e.site[0] == "ops.py"]
        moved = [e for e in rz.registry if e.site[0] == "test_stale_memory_gpu.py"]
        assert sum(e.shape == (M, D) and e.dtype == torch.float32 for e in mine) >= 2, mine       # y, and dx in the backward
        assert sum(e.shape == (M,) and e.dtype == torch.float32 for e in mine) >= 2, mine          # mean and rstd
        assert sum(e.shape == (M, D) for e in moved) >= 2 and sum(e.shape == (D,) for e in moved) >= 2, moved   # x, cy; gamma, beta
        assert all(e.backing.is_cuda and (e.backing.data_ptr() + e.front) % 512 == 0 for e in rz.registry)
        assert res["y"].data_ptr() in {e.backing.data_ptr() + e.front for e in mine}
        rz.check()


def test_gan_step_with_gradient_penalty(device):
    """One eager step of the GAN-step helper of tests/test_stale_memory_step_gpu.py (gp_lambda = 10, f32, no perceptual
    term: its smallest configuration), model, discriminator, trainer and inputs all built inside the context."""
    from test_stale_memory_step_gpu import _parts, _trainer, CONFIGS

    cfg = CONFIGS[0]
    assert cfg == (None, False, False)
    with pytest.MonkeyPatch.context() as mp, redzoned_empty("nan") as rz:
        model, discr, per, img, eta = _parts(device, cfg, mp)
        tr = _trainer(model, discr, per, cfg)
        logs = {k: v.detach().clone() for k, v in tr.step(img, eta=eta).items()}
        assert len(rz.registry) > 100, len(rz.registry)
        rz.check()
    assert "d_loss" in logs
    for k, v in logs.items():
        assert bool(torch.isfinite(v).all()), f"{k} is not finite: {v}"
