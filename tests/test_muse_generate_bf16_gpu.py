"""The masked-token parallel decode under bf16 autocast (amk.models.muse.parallel_decode, MUSE.generate,
MaskGitTransformer.generate) on the guided logits head: ops.guided_logits (amk_cfg_layernorm_bf16 +
amk_gemm_bf16_f32out) between the decoder's hidden states and amk_sample_step.

On the fixture of the reference's own MUSE.generate run (tests/golden/muse_generate_small.npz: dim 64, 256 codes, 16
tokens, 6 steps, its context and the Gumbel noise it drew):
  1. the decode runs under autocast (it raised "amk kernels compute in fp32" before the head existed, and still does with
     AMK_GUIDED_HEAD=0) and returns ids in [0, V);
  2. every step's ids are torch's sampling chain on that step's traced f32 logits and the same noise;
  3. the guided logits, teacher-forced at the fixture's decoder inputs, deviate from the fp64 restatement of the reference
     no more than the module path under the same autocast does (caps 1.5 on the maximum, 1.25 on the rms: the ones
     tests/test_parti_decode_bf16_gpu.py holds its decode to); the ratios are printed;
  4. outside autocast the decode is the f32 one, id for id the reference's run, and launches neither new kernel;
  5. the ids do not depend on what freshly allocated memory holds."""
import functools
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from util import GOLDEN, load_golden, weights_of

pytestmark = pytest.mark.gpu
MAX_CAP, RMS_CAP = 1.5, 1.25
TIE_ROWS_PER_1000 = 1
NEW_KERNELS = ("cfg_layernorm_bf16", "gemm_bf16_f32out")


def _autocast():
    return torch.autocast("cuda", dtype=torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _fixture():
    fx = load_golden("muse_generate_small")
    with open(os.path.join(GOLDEN, "golden_meta.json")) as f:
        meta = json.load(f)["muse_generate_small"]
    return fx, meta


class _Case:
    def __init__(self, device):
        from amk.models.muse import BidirectionalDecoder

        fx, meta = _fixture()
        self.fx, self.cfg, self.steps = fx, meta["cfg"], meta["timesteps"]
        self.V, self.n = self.cfg["codebook_size"], self.cfg["num_patches"]
        self.dec = BidirectionalDecoder(**self.cfg).to(device).eval()
        self.dec.load_state_dict({k: v.to(device) for k, v in weights_of(fx).items()}, strict=True)
        self.ctx = torch.from_numpy(fx["context"]).to(device)
        self.gumbel = torch.from_numpy(fx["gumbel"]).to(device)

    def decode(self, **kw):
        from amk.models.muse import parallel_decode

        return parallel_decode(self.dec, self.ctx, self.V, self.n, self.steps, gumbel=self.gumbel, **kw)


def _events(fn):
    from amk import ops

    ops.KERNEL_EVENTS = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {n: len(v) for n, v in ops.KERNEL_EVENTS.items()}
    finally:
        ops.KERNEL_EVENTS = None


# ---------------------------------------------------------------------------------------------- 1. it runs
def test_parallel_decode_runs_under_autocast(device):
    c = _Case(device)
    with _autocast():
        ids, ev = _events(lambda: c.decode())
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (c.ctx.shape[0], c.n)
    assert bool(((ids >= 0) & (ids < c.V)).all())
    launches = {k: sum(v for n, v in ev.items() if n.startswith(k)) for k in NEW_KERNELS}
    assert launches == {k: c.steps for k in NEW_KERNELS}, ev


def test_models_generate_under_autocast(device):
    from amk.models import MUSE, ViTVQGAN
    from amk.models.maskgit import MaskGitTransformer

    torch.manual_seed(0)
    vq = ViTVQGAN(dict(dim=64, img_size=32, patch_size=8, n_heads=1, d_head=64, depth=1, mlp_dim=64, dropout=0.0),
                  dict(codebook_size=64, codebook_dim=32))
    muse = MUSE(dim=64, vq=vq, text_dim=24, n_heads=1, d_head=64, depth=2, mult=4).to(device)
    text_hidden = torch.randn(2, 7, 24, device=device)
    with _autocast():
        out, ev = _events(lambda: muse.generate(text_hidden, timesteps=6))
    assert tuple(out.shape) == (2, 3, 32, 32) and bool(torch.isfinite(out.float()).all())
    assert sum(v for n, v in ev.items() if n.startswith("gemm_bf16_f32out")) == 6, ev

    vq = ViTVQGAN(dict(dim=64, img_size=32, patch_size=4, n_heads=2, d_head=64, depth=1, mlp_dim=96, dropout=0.0),
                  dict(codebook_size=256, codebook_dim=32))
    m = MaskGitTransformer(dim=128, vq=vq, vocab_size=256, n_heads=2, d_head=64, dec_depth=2, mult=4, dropout=0.0).to(device).eval()
    trace, logits_trace = [], []
    with _autocast():
        out, ev = _events(lambda: m.generate(batch=2, timesteps=6, trace=trace, logits_trace=logits_trace))
    assert tuple(out.shape) == (2, 3, 32, 32) and bool(torch.isfinite(out.float()).all())
    assert sum(v for n, v in ev.items() if n.startswith("cfg_layernorm_bf16")) == 6, ev
    assert len(trace) == 6 and len(logits_trace) == 6
    assert all(t.dtype == torch.float32 and tuple(t.shape) == (2, vq.num_patches, 256) for t in logits_trace)
    assert bool((trace[0] == m.mask_token_id).all())


def test_vocabulary_past_the_samplers_range_takes_the_torch_chain(device, monkeypatch):
    """V = 36872 (a multiple of 8 above amk_sample_step's 36864): the guided f32 logits go through the torch chain."""
    from amk import ops
    from amk.models.muse import BidirectionalDecoder, parallel_decode

    V, n = 36872, 4
    torch.manual_seed(1)
    dec = BidirectionalDecoder(dim=64, codebook_size=V, n_heads=1, d_head=64, depth=1, mult=4, dropout=0.0, num_patches=n).to(device).eval()
    ctx = torch.randn(2, 5, 64, device=device)

    def no_sampler(*args, **kw):
        raise AssertionError("amk_sample_step does not take this V")

    monkeypatch.setattr(ops, "sample_step", no_sampler)
    logits_trace = []
    with _autocast():
        ids, ev = _events(lambda: parallel_decode(dec, ctx, V, n, 3, logits_trace=logits_trace))
    assert tuple(ids.shape) == (2, n) and bool(((ids >= 0) & (ids < V)).all())
    assert len(logits_trace) == 3 and all(t.dtype == torch.float32 and tuple(t.shape) == (2, n, V) for t in logits_trace)
    assert sum(v for k, v in ev.items() if k.startswith("gemm_bf16_f32out")) == 3, ev


_CHILD = """
import json, os, sys, torch
from amk import ops
from amk.models.muse import BidirectionalDecoder, parallel_decode
from util import GOLDEN, load_golden, weights_of
assert ops.GUIDED_HEAD is False
fx = load_golden("muse_generate_small")
meta = json.load(open(os.path.join(GOLDEN, "golden_meta.json")))["muse_generate_small"]
cfg = meta["cfg"]
dev = torch.device("cuda:0")
dec = BidirectionalDecoder(**cfg).to(dev).eval()
dec.load_state_dict({k: v.to(dev) for k, v in weights_of(fx).items()}, strict=True)
try:
    with torch.autocast("cuda", dtype=torch.bfloat16):
        parallel_decode(dec, torch.from_numpy(fx["context"]).to(dev), cfg["codebook_size"], cfg["num_patches"], meta["timesteps"],
                        gumbel=torch.from_numpy(fx["gumbel"]).to(dev))
    print("RAN")
except RuntimeError as e:
    print("REFUSED:", e)
"""


def test_switch_off_still_refuses(device):
    """AMK_GUIDED_HEAD is read once per process: a fresh child with it at 0 gets the refusal the decode gave before."""
    env = dict(os.environ, AMK_GUIDED_HEAD="0", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "REFUSED: amk kernels compute in fp32; got torch.bfloat16" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------- 2. each step is its own sampler
def test_each_step_is_torchs_chain_on_its_own_logits(device, monkeypatch):
    from amk import ops

    c = _Case(device)
    calls = []
    real = ops.sample_step

    def recording(logits, ids, mask=None, null_logits=None, **kw):
        before = ids.clone()
        scores = real(logits, ids, mask=mask, null_logits=null_logits, **kw)
        calls.append(dict(logits=logits, before=before, after=ids.clone(), mask=mask.clone(), null=null_logits, tau=kw["tau"],
                          gumbel=kw["gumbel"]))
        return scores

    monkeypatch.setattr(ops, "sample_step", recording)
    trace, logits_trace = [], []
    with _autocast():
        final = c.decode(trace=trace, logits_trace=logits_trace)
    assert len(calls) == c.steps == len(trace) == len(logits_trace)
    k = math.ceil((1 - 0.9) * c.V)
    rows = left_out = 0
    for t, call in enumerate(calls):
        lg = logits_trace[t]
        assert call["null"] is None and call["logits"] is lg and lg.dtype == torch.float32
        assert torch.equal(call["before"], trace[t]) and torch.equal(call["gumbel"], c.gumbel[t])
        assert torch.equal(call["mask"], trace[t] == c.V), "the step's mask is the mask ids entering the decoder"
        val, ind = lg.topk(k, dim=-1)
        tie = (lg >= val[..., -1:]).sum(-1) > k       # the kernel keeps every logit >= the keep-th, topk exactly k
        rows += tie.numel()
        left_out += int(tie.sum())
        if t == c.steps - 1:
            assert call["tau"] == 0.0
            want = torch.zeros_like(call["before"])   # tau 0: the reference's softmax is NaN everywhere, argmax 0
        else:
            filt = torch.full_like(lg, float("-inf")).scatter_(2, ind, val)
            want = F.softmax((filt + call["gumbel"]) / call["tau"], dim=-1).argmax(dim=-1)
        want = torch.where(call["mask"], want, call["before"])
        same = (call["after"] == want) | tie
        assert bool(same.all()), f"step {t}: {int((~same).sum())} ids differ from torch's chain on the traced logits"
    assert torch.equal(final, calls[-1]["after"])
    assert left_out * 1000 <= TIE_ROWS_PER_1000 * rows, f"{left_out} of {rows} rows tie at the keep-th logit"


# ---------------------------------------------------------------------------------------------- 3. accuracy
def _dev(got, ref):
    e = got.detach().double().cpu() - ref
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


def test_guided_logits_accuracy_against_fp64(device):
    """Teacher-forced at the fixture's ids_in[t].  Measured on an MI355X: guided head max 7.17e-3,
    rms 1.63e-3; module path max 9.35e-3, rms 1.77e-3; ratios 0.767 / 0.919."""
    from amk import ops

    c = _Case(device)
    w64 = {k: v.double() for k, v in weights_of(c.fx).items()}
    ctx64 = torch.from_numpy(c.fx["context"]).double()
    h, d, depth = c.cfg["n_heads"], c.cfg["d_head"], c.cfg["depth"]
    ref, new, old = [], [], []
    fn, head = c.dec.final_norm, c.dec.linear.weight
    null_ctx = torch.zeros_like(c.ctx)
    for t in range(c.steps):
        ids = torch.from_numpy(c.fx["ids_in"][t])
        l = ref_cpu.bidirectional_decoder(ids, ctx64, w64, h, d, depth)
        null = ref_cpu.bidirectional_decoder(ids, torch.zeros_like(ctx64), w64, h, d, depth)
        ref.append(null + 3 * (l - null))
        idd = ids.to(device)
        with torch.no_grad(), _autocast():
            new.append(ops.guided_logits(c.dec.hidden(idd, context=c.ctx), fn.gamma, fn.beta, head,
                                         null_h=c.dec.hidden(idd, context=null_ctx), cfg_scale=3.0))
            lm, nm = c.dec(idd, context=c.ctx), c.dec(idd, context=null_ctx)
            assert lm.dtype == torch.bfloat16
            old.append(nm.float() + 3 * (lm.float() - nm.float()))
    ref, new, old = torch.stack(ref), torch.stack(new), torch.stack(old)
    assert new.dtype == torch.float32 and bool(torch.isfinite(new).all())
    nmax, nrms = _dev(new, ref)
    omax, orms = _dev(old, ref)
    print(f"guided head: max {nmax:.3e} rms {nrms:.3e}; module path under autocast: max {omax:.3e} rms {orms:.3e}; "
          f"ratio max {nmax / omax:.3f} rms {nrms / orms:.3f}; max |ref| {float(ref.abs().max()):.3f}")
    assert nmax <= MAX_CAP * omax, (nmax, omax)
    assert nrms <= RMS_CAP * orms, (nrms, orms)


# ---------------------------------------------------------------------------------------------- 4. f32 untouched
def test_f32_decode_is_the_reference_run_and_skips_the_head(device):
    c = _Case(device)
    trace, logits_trace = [], []
    ids, ev = _events(lambda: c.decode(trace=trace, logits_trace=logits_trace))
    for t, got in enumerate(trace):
        assert torch.equal(got.cpu(), torch.from_numpy(c.fx["ids_in"][t])), f"decoder input at step {t}"
    assert torch.equal(ids.cpu(), torch.from_numpy(c.fx["final_ids"]))
    assert not logits_trace and not any(n.startswith(NEW_KERNELS) for n in ev), ev


# ---------------------------------------------------------------------------------------------- 5. stale memory
def test_ids_do_not_depend_on_stale_memory(device):
    import poison

    c = _Case(device)

    def case():
        with _autocast():
            return {"ids": c.decode()}

    nan_run, big_run = poison.run_both_fills(case)
    poison.assert_fill_independent(nan_run, big_run, "parallel_decode under autocast")
