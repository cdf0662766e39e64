"""The KV-cached decode at model level under the allocation poisoner (tests/poison.py) and the red-zone allocator
(tests/redzone.py): what tests/test_stale_memory_step_gpu.py is for the GAN step.  The self-attention caches and the decode
workspace of Decoder.init_state come from torch.empty (amk/models/transformer.py:207-212), so both allocators reach them.

A tiny Parti and a tiny Transformer (dim 64, depth 2, 2 heads of 32, capacity 80), each built inside the context: ``prefill``
of a 66-token prefix -- self-attention crosses the 64-key chunk of csrc/attn_prefill.hip -- then 6 eager sample steps on
seeded Gumbel noise (``next_logits`` and a draw; Parti draws through amk_sample_step).  Once in f32, once under bf16 autocast
with the bf16 state.  Under both poison fills and under both red-zone fills:

  * the token ids, every step's logits and the valid rows of every layer's cache are finite and BITWISE equal between the
    fills, and check() passes under each red-zone fill;
  * the f32 logits lie inside the bound tests/test_parti_prefill_gpu.py holds the prefill and its steps to: TOL_OUT
    against the fp64 restatement of tests/parti_ref.py on the model's own weights and the tokens the run drew.

And the masked-token parallel decode of MUSE.generate under bf16 autocast on the guided logits head (MUSE.generate's body
with parallel_decode's logits_trace): ids and every step's guided f32 logits bitwise equal between the fills.

Nothing is captured here: graph replay under poison is held by tests/test_stale_memory_step_gpu.py.  Nothing is meant to
fault: integer and index buffers are never filled."""
import functools

import pytest
import torch

import parti_ref
from poison import assert_fill_independent, run_both_fills
from redzone import run_both
from test_parti_gpu import TOL_OUT, StubVQ
from util import assert_close

pytestmark = pytest.mark.gpu

DIM, HEADS, D_HEAD, DEPTH, V, CAPACITY = 64, 2, 32, 2, 64, 80
B, PREFIX, STEPS = 2, 66, 6
RUNNERS = {"poison": run_both_fills, "redzone": run_both}


def _autocast(on):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(on))


def _noise(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return -torch.empty(*shape).exponential_(generator=g).log()


def _prefix(seed):
    return torch.randint(3, V, (B, PREFIX), generator=torch.Generator().manual_seed(seed))      # (no start / end token ids)


def _valid_rows(state):
    """Rows 0 .. pos - 1 of every layer's self-attention cache: the rows beyond hold whatever the allocator left."""
    return {f"cache{i}": kv[:, :state.host_pos] for i, kv in enumerate(state.self_kv)}


def _build_parti(device):
    from amk.models import Parti

    torch.manual_seed(0)
    return Parti(DIM, StubVQ(V, PREFIX + STEPS + 1), None, None, 77, HEADS, D_HEAD, DEPTH).to(device).eval()


def _parti_case(device, bf16, keep=None):
    def case():
        m = _build_parti(device)
        text = torch.randn(B, 7, DIM, generator=torch.Generator().manual_seed(1)).to(device)
        gumbel = _noise((STEPS + 1, B, V), 2).to(device)
        prefix = _prefix(3).to(device)
        token = torch.zeros((B, 1), dtype=torch.long, device=device)
        logits, ids = [], []
        with torch.no_grad(), _autocast(bf16):
            state = m.begin_decode(text, capacity=CAPACITY)
            assert state.dtype == (torch.bfloat16 if bf16 else torch.float32)
            row = m.prefill(state, prefix)                    # the start token and the prefix: rows 0 .. 66
            for i in range(STEPS + 1):                        # the prefill's draw, then six steps
                logits.append(row.clone())
                m._draw(row, token, gumbel[i], 1.0, 0.9)
                ids.append(token[:, 0].clone())
                if i < STEPS:
                    row = m.next_logits(state, token)
        assert state.host_pos == PREFIX + 1 + STEPS
        if keep is not None:
            keep["weights"] = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        return dict(ids=torch.stack(ids, dim=1), logits=torch.stack(logits), **_valid_rows(state))
    return case


def _build_transformer(device):
    from amk.models import Transformer

    torch.manual_seed(0)
    return Transformer(DIM, V, HEADS, D_HEAD, DEPTH, DEPTH, V).to(device).eval()


def _transformer_case(device, bf16, keep=None):
    def case():
        m = _build_transformer(device)
        src = torch.randint(3, V, (B, 9), generator=torch.Generator().manual_seed(4)).to(device)
        gumbel = _noise((STEPS + 1, B, V), 5).to(device)
        tgt = torch.cat((torch.ones(B, 1, dtype=torch.long), _prefix(6)[:, :PREFIX - 1]), dim=1).to(device)   # start token + 65
        logits, ids = [], []
        with torch.no_grad(), _autocast(bf16):
            state = m.begin_decode(src, capacity=CAPACITY)
            assert state.dtype == (torch.bfloat16 if bf16 else torch.float32)
            row = m.prefill(state, tgt)                       # rows 0 .. 65
            for i in range(STEPS + 1):
                logits.append(row.clone())
                token = (row + gumbel[i]).argmax(dim=-1)
                ids.append(token)
                if i < STEPS:
                    row = m.next_logits(state, token)
        assert state.host_pos == PREFIX + STEPS
        if keep is not None:
            keep["weights"] = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        return dict(ids=torch.stack(ids, dim=1), logits=torch.stack(logits), **_valid_rows(state))
    return case


def _w64(weights):
    return {k: v.double() for k, v in weights.items() if v.dtype.is_floating_point}


@functools.lru_cache(maxsize=None)
def _fp64_logits(model, ids):
    """fp64 logits (steps + 1, B, V) of the rows the run produced, on the model's own weights (built on the CPU from the same
    seed: the constructors draw on the CPU) and the tokens it drew (ids: a tuple of tuples, the cache's key)."""
    drawn = torch.tensor(ids, dtype=torch.long)
    if model == "parti":
        w = _w64(_build_parti("cpu").state_dict())
        text = torch.randn(B, 7, DIM, generator=torch.Generator().manual_seed(1)).double()
        # row t of the logits is the token at position t given the tokens before it: rows 66 .. 72 (the last id is no input)
        rows = parti_ref.parti_logits(text, torch.cat((_prefix(3), drawn), dim=1), w, HEADS, D_HEAD, DEPTH)[:, PREFIX:]
    else:
        w = _w64(_build_transformer("cpu").state_dict())
        src = torch.randint(3, V, (B, 9), generator=torch.Generator().manual_seed(4))
        tgt = torch.cat((torch.ones(B, 1, dtype=torch.long), _prefix(6)[:, :PREFIX - 1], drawn[:, :STEPS]), dim=1)
        rows = parti_ref.transformer_logits(src, tgt, w, HEADS, D_HEAD, DEPTH, DEPTH)[:, PREFIX - 1:]
    assert rows.shape[1] == STEPS + 1
    return rows.transpose(0, 1).contiguous()


@pytest.mark.parametrize("runner", sorted(RUNNERS))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("model", ["parti", "transformer"])
def test_prefill_and_sample_steps_do_not_depend_on_the_fill(device, model, dtype, runner):
    keep = {}
    case = (_parti_case if model == "parti" else _transformer_case)(device, dtype == "bf16", keep)
    nan_run, big_run = RUNNERS[runner](case)                  # redzone.run_both: check() inside, under each fill
    torch.cuda.synchronize()
    assert_fill_independent(nan_run, big_run, f"{model} {dtype} decode under {runner}")
    assert tuple(nan_run["ids"].shape) == (B, STEPS + 1) and tuple(nan_run["logits"].shape) == (STEPS + 1, B, V)
    assert nan_run["logits"].dtype == torch.float32
    assert int(nan_run["ids"].min()) >= 0 and int(nan_run["ids"].max()) < V
    if dtype == "f32":
        build = _build_parti if model == "parti" else _build_transformer
        for k, v in build("cpu").state_dict().items():       # the reference's weights are the run's
            assert torch.equal(v, keep["weights"][k]), k
        ref = _fp64_logits(model, tuple(map(tuple, nan_run["ids"].cpu().tolist())))
        for i in range(STEPS + 1):
            assert_close(nan_run["logits"][i], ref[i], TOL_OUT, f"{model}: logits of step {i} ({runner})")


@pytest.mark.parametrize("runner", sorted(RUNNERS))
def test_muse_generate_under_autocast_does_not_depend_on_the_fill(device, runner):
    from amk.models import MUSE, ViTVQGAN
    from amk.models.muse import parallel_decode

    timesteps = 6

    def case():
        torch.manual_seed(0)
        vq = ViTVQGAN(dict(dim=64, img_size=32, patch_size=8, n_heads=1, d_head=64, depth=1, mlp_dim=64, dropout=0.0),
                      dict(codebook_size=64, codebook_dim=32))
        muse = MUSE(dim=64, vq=vq, text_dim=24, n_heads=1, d_head=64, depth=2, mult=4).to(device).eval()
        text_hidden = torch.randn(2, 7, 24, generator=torch.Generator().manual_seed(1)).to(device)
        n = muse.vq.num_patches
        gumbel = _noise((timesteps, 2, n, 64), 2).to(device)
        logits_trace = []
        with torch.no_grad(), _autocast(True):
            ids = parallel_decode(muse.decoder, muse._context(text_hidden), muse.mask_token_id, n, timesteps,
                                  fused_sampling=muse.fused_sampling, gumbel=gumbel, logits_trace=logits_trace)
        assert len(logits_trace) == timesteps, "the decode did not run on the guided logits head"
        return dict(ids=ids, **{f"logits{i}": t for i, t in enumerate(logits_trace)})

    nan_run, big_run = RUNNERS[runner](case)
    torch.cuda.synchronize()
    assert_fill_independent(nan_run, big_run, f"MUSE generate under {runner}")
    assert nan_run["logits0"].dtype == torch.float32
    assert int(nan_run["ids"].min()) >= 0 and int(nan_run["ids"].max()) < 64
