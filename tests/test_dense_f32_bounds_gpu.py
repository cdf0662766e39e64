"""amk_gemm_f32 and amk_row_stats (csrc/gemm_f32.hip) on the MI355X, held element by element to the two tiers of
tests/dense_f32_ref.py (the hard f32 bound and 4 x the CPU emulation's q) against fp64 references computed on the
device, on every dispatch path: the plain NT kernel, the persistent NT walk with more tiles than workgroups (two and
three tiles per workgroup, ragged and full tiles draining under each other, consecutive tiles of one workgroup in
different column segments), NN with the segment seam inside a step, TN over the chunk counts of tn_chunks() and the
seams of tn_reduce_kernel's 8-way loop, row_stats at the edges of its NCH dispatch and past the grid wrap.  The case
list is generated from the device's CU count (cases(cus)); tests/test_dense_f32_bounds.py proves without a GPU that it
reaches every kernel instance and condition for 256 and 304 CUs.

Every output is written into a NaN canvas with guard rows and guard columns (ldc > N): through `out=` where the Python
entry has one, otherwise the fresh tensor is checked and an equal call through the C ABI descriptor writes into a
padded canvas and must give the same bits.  After the call the guards are untouched bit for bit, the result holds no
NaN and every element is inside both tiers.  No element is left out of a check (the `under` allowance of the saturate
family apart, see dense_f32_ref.py).

Bitwise invariants: a rerun; the rows of a result against a call with 128 more rows; the two-projection launch against
two launches; gemm_tn with y2 against two calls where the chunking is the same; ops.linear and ops.swiglu_ffn against
the dense.* calls they are made of; NT at K = 100 (the walk) against K = 96 (the plain kernel) on the same data.

The environment switches are statics of the process, so each runs in a fresh child process (this file run as a
script: `python test_dense_f32_bounds_gpu.py <out.npz>` runs reduced_cases() with the same canvases and bounds and
saves the results), one child at a time, nothing started after a child fails.  From the source: gemm_nt_kernel<32> and
NtWalk contract index 32 kt + 16 hf + 4 s4 + x in the same order, start from zero accumulators and apply bias,
residual and the SwiGLU gate by the same expressions, so AMK_DENSE_WALK=0 equals the default bit for bit;
AMK_DENSE_STAGGER only delays workgroups; AMK_DENSE_BK=16 contracts in another order (16 kt + 8 hf + 4 s4 + x) and
AMK_DENSE_TN_SLOTS changes the chunks: these two are held to the bounds only.
The worst hard ratio and q / limit per kernel are printed after the run (pytest -s)."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "attention-models_amd"), os.path.join(_root, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import ctypes
import subprocess

import numpy as np
import pytest
import torch

import dense_f32_ref as ref

pytestmark = pytest.mark.gpu

NANBITS = 0x7FC0BEEF
SWITCHES = ("AMK_DENSE_BK", "AMK_DENSE_WALK", "AMK_DENSE_STAGGER", "AMK_DENSE_TN_SLOTS")
RAGGED = [(1, 4, 4), (5, 8, 36), (128, 128, 32), (130, 64, 40), (257, 300, 24), (1000, 192, 256), (333, 260, 1368),
          (96, 516, 64), (2048, 32, 256), (2048, 256, 32)]          # the sizes of tests/test_dense_gpu.py


# ---------------------------------------------------------------------------------------------- the case list
def _factor(t):
    """(row tiles, column tiles) with product t, as square as t allows (t prime: (t, 1))."""
    best = (t, 1)
    d = 2
    while d * d <= t:
        if t % d == 0:
            best = (t // d, d)
        d += 1
    return best


def find_tn_m(N, K, cus, nchunk, last=None, lo=1, hi=70000):
    """The smallest M in [lo, hi) for which tn_chunks gives `nchunk` chunks and `last` rows in the last one."""
    for M in range(lo, hi):
        nc, spc = ref.tn_chunks(M, N, K, cus)
        if nc == nchunk and (last is None or M - (nc - 1) * spc * 32 == last):
            return M
    raise AssertionError(f"no M gives nchunk {nchunk} / last {last} for N {N} K {K} on {cus} CUs")


def cases(cus):
    """The GPU case list for a device of `cus` compute units: a list of dicts (kind: nt, nt2, swiglu, nn, nn_bwd, tn,
    stats)."""
    slots = 2 * cus
    out = []

    def C(kind, id, family, **kw):
        out.append(dict(kind=kind, id=id, family=family, **kw))

    # ---- NT walk: more tiles than workgroup slots
    mt, nt = _factor(slots + 1)
    if nt == 1:
        mt, nt = slots + 1, 1
    C("nt", "walk_between", "offset", M=128 * 18 + 1, N=128 * (-(-(slots + 96) // 19)) - 60, K=100, mode="ln_bias_resid")
    C("nt", "walk_above2", "binade", M=128 * 32 + 127, N=128 * (-(-(2 * slots + 32) // 33)), K=128, mode="bias")
    C("nt", "walk_grid_plus1", "outlier_rows", M=128 * (mt - 1) + 1, N=128 * nt - 60, K=132, mode="resid")
    C("nt", "walk_k1368", "cancel", M=128 * 18 + 127, N=128 * (-(-(slots + 96) // 19)) - 124, K=1368, mode="plain")
    C("nt", "walk_ln_m127", "spike", M=128 * 16 + 127, N=128 * (-(-(slots + 40) // 17)) - 4, K=128, mode="ln")
    n2t = 11
    C("nt2", "walk_two", "unit", M=128 * (slots // (8 + n2t) + 1) + 1, N=1024, N2=128 * n2t - 84, K=128, ln=False)
    C("nt2", "walk_two_ln", "constant", M=128 * (slots // (3 + 2) + 1) + 127, N=384, N2=128 + 4, K=260, ln=True)
    for H, keep, b12, fam, K, ln in [(1280, True, True, "saturate", 128, False), (1348, False, True, "binade", 256, True),
                                     (1316, True, False, "cancel", 100, False), (1316, False, False, "unit", 132, True)]:
        ntn = -(-H // 64)
        C("swiglu", f"walk_swiglu_h{H}_{int(keep)}{int(b12)}", fam, M=128 * (slots // ntn + 1) + (1 if keep else 127), H=H, K=K,
          keep=keep, b12=b12, ln=ln)
    # ---- both sides of K > 96 on the same data
    C("nt", "k96_k100", "unit", M=300, N=260, K=100, mode="bias", k96=True)
    # ---- NT plain kernel (K <= 96) and small walks, ragged sizes, strides
    modes = ["plain", "bias", "resid", "ln", "ln_bias_resid"]
    # (offset, constant and spike are the families of the LayerNorm fold and of row_stats: they go with ln alone)
    fam_of = lambda i, ln: (ref.LN_FAMILIES[i % 6] if ln else ref.GEMM_FAMILIES[i % 4])
    for i, (M, N, K) in enumerate(RAGGED + [(200, 132, 36), (129, 252, 60), (1, 260, 96), (1, 128, 256), (260, 4, 100),
                                            (140, 124, 28)]):
        C("nt", f"nt_{M}x{N}x{K}", fam_of(i, i % 5 >= 3) if K > 4 else "unit", M=M, N=N, K=K, mode=modes[i % 5])
    C("nt", "nt_lda_k4", "binade", M=257, N=132, K=64, mode="ln_bias_resid", stride="k+4")
    C("nt", "nt_lda_2k", "outlier_rows", M=130, N=260, K=160, mode="resid", stride="2k")
    C("nt", "nt_coloff", "cancel", M=300, N=124, K=92, mode="bias", stride="coloff")
    C("nt2", "two_small", "binade", M=300, N=128, N2=256, K=64, ln=True)
    C("nt2", "two_ragged", "outlier_rows", M=64, N=256, N2=100, K=40, ln=False)
    for H, keep, b12, fam, K, ln in [(64, True, True, "unit", 32, False), (100, True, True, "saturate", 40, True),
                                     (36, False, True, "outlier_rows", 256, True), (68, True, False, "cancel", 96, False),
                                     (1368, True, True, "binade", 256, False)]:
        C("swiglu", f"swiglu_h{H}_k{K}", fam, M=129 if H == 36 else 300, H=H, K=K, keep=keep, b12=b12, ln=ln)
    # ---- NN
    for i, (M, N, K) in enumerate([s for s in RAGGED if s[1] % 4 == 0] + [(200, 132, 36), (129, 252, 60), (1, 260, 100),
                                                                         (140, 124, 28), (300, 4, 132)]):
        C("nn", f"nn_{M}x{N}x{K}", ref.GEMM_FAMILIES[i % 4] if K > 4 else "unit", M=M, N=N, K=K, K2=0)
    C("nn", "nn_lda_k4", "binade", M=257, N=132, K=64, K2=0, stride="k+4")
    C("nn", "nn_coloff", "cancel", M=130, N=260, K=160, K2=0, stride="coloff")
    C("nn", "nn_lda_2k", "outlier_rows", M=300, N=124, K=92, K2=0, stride="2k")
    for (M, K1, K2, N), fam in zip([(300, 64, 128, 256), (1000, 512, 1024, 256), (70, 40, 24, 36), (257, 36, 8, 128),
                                    (129, 100, 60, 132)], ["unit", "cancel", "binade", "outlier_rows", "cancel"]):
        C("nn", f"nn_seg_{K1}_{K2}", fam, M=M, N=N, K=K1, K2=K2)
    for (M, H, K), fam in zip([(100, 64, 32), (300, 100, 40), (1000, 1368, 256), (257, 132, 100), (130, 260, 64), (129, 36, 28)],
                              ["unit", "cancel", "saturate", "saturate", "cancel", "binade"]):
        C("nn_bwd", f"nn_bwd_h{H}_k{K}", fam, M=M, H=H, K=K)
    # ---- TN: chunk counts and seams from tn_chunks for this device
    for nchunk, last, fam, ln in [(1, None, "unit", True), (2, None, "binade", False), (8, None, "cancel", False), (8, 33, "offset", True),
                                  (9, 1, "outlier_rows", True), (9, 33, "unit", False), (15, None, "spike", True)]:
        M = find_tn_m(256, 128, cus, nchunk, last, lo=200 if nchunk == 1 else 1)
        C("tn", f"tn_chunks{nchunk}_last{last}", fam, M=M, N=256, K=128, N2=0, ln=ln, bias=(nchunk, last) != (8, None), out=nchunk in (2, 9))
    C("tn", "tn_max_chunks", "unit", M=256 * cus, N=128, K=128, N2=0, ln=False, bias=True, out=True)
    C("tn", "tn_tiles16", "binade", M=5000, N=512, K=512, N2=0, ln=True, bias=True, out=False)
    C("tn", "tn_tiles20", "cancel", M=5000, N=512, K=640, N2=0, ln=False, bias=False, out=False)
    for i, (M, N, K) in enumerate([s for s in RAGGED if s[1] % 4 == 0] + [(200, 132, 36), (129, 252, 60), (1, 260, 100),
                                                                         (255, 124, 28), (300, 4, 132)]):
        C("tn", f"tn_{M}x{N}x{K}", fam_of(i, i % 2 == 1) if K > 4 else "unit", M=M, N=N, K=K, N2=0, ln=i % 2 == 1, bias=i % 3 != 2, out=False)
    C("tn", "tn_lda_k4", "outlier_rows", M=700, N=132, K=64, N2=0, ln=True, bias=True, out=False, stride="k+4")
    C("tn", "tn_lda_2k", "binade", M=1000, N=124, K=92, N2=0, ln=False, bias=True, out=False, stride="2k")
    C("tn", "tn_coloff", "unit", M=2049, N=260, K=160, N2=0, ln=False, bias=True, out=False, stride="coloff")
    for (M, N1, N2, K), fam in zip([(3000, 128, 256, 64), (5000, 512, 1024, 256), (700, 256, 100, 40), (2081, 128, 36, 132)],
                                   ["unit", "binade", "cancel", "outlier_rows"]):
        C("tn", f"tn_two_{N1}_{N2}", fam, M=M, N=N1, K=K, N2=N2, ln=N2 != 256, bias=N2 != 1024, out=N2 == 100)
    # ---- row_stats
    for D in (4, 256, 260, 1024, 1028, 4096):
        for j, M in enumerate((1, 5)):
            for fam in ref.LN_FAMILIES[j::2]:
                C("stats", f"stats_{M}x{D}_{fam}", fam, M=M, D=D)
    for fam in ref.LN_FAMILIES:
        C("stats", f"stats_wrap_{fam}", fam, M=65541, D=4)
        C("stats", f"stats_300x256_{fam}", fam, M=300, D=260 if fam == "spike" else 256)
    return out


def reduced_cases(cus):
    """About a dozen cases over the three products and all epilogues for the child processes of the switches."""
    slots = 2 * cus
    R = []

    def C(kind, id, family, **kw):
        R.append(dict(kind=kind, id=id, family=family, **kw))

    C("nt", "r_walk", "binade", M=128 * ((slots + 2) // 2) + 1, N=256 - 4, K=128, mode="ln_bias_resid")
    C("nt", "r_plain", "cancel", M=257, N=300, K=24, mode="bias")
    C("nt", "r_resid", "outlier_rows", M=333, N=260, K=1368, mode="resid")
    C("nt", "r_none", "unit", M=130, N=64, K=100, mode="plain")
    C("nt2", "r_two", "unit", M=300, N=128, N2=228, K=132, ln=True)
    C("swiglu", "r_swiglu", "saturate", M=300, H=100, K=132, keep=True, b12=True, ln=True)
    C("swiglu", "r_swiglu_nokeep", "binade", M=129, H=36, K=64, keep=False, b12=False, ln=False)
    C("nn", "r_nn", "binade", M=257, N=300, K=100, K2=0)
    C("nn", "r_nn_seg", "cancel", M=300, N=132, K=36, K2=100)
    C("nn_bwd", "r_nn_bwd", "saturate", M=300, H=100, K=40)
    C("tn", "r_tn", "outlier_rows", M=2001, N=256, K=128, N2=0, ln=True, bias=True, out=True)
    C("tn", "r_tn_two", "cancel", M=3000, N=128, K=64, N2=100, ln=False, bias=True, out=False)
    C("tn", "r_tn_one_chunk", "unit", M=255, N=132, K=36, N2=0, ln=False, bias=True, out=False)
    return R


def case_path(c, cus, bk=32, walk=True, tn_slots=0):
    """expected_path of the case's launch."""
    k = c["kind"]
    if k == "nt":
        epi = "resid" if "resid" in c["mode"] else "bias"
        return ref.expected_path("nt", epi, c["M"], c["N"], c["K"], 0, "ln" in c["mode"], cus, bk, walk)
    if k == "nt2":
        return ref.expected_path("nt", "bias", c["M"], c["N"] + c["N2"], c["K"], c["N"], c["ln"], cus, bk, walk)
    if k == "swiglu":
        return ref.expected_path("nt", "swiglu", c["M"], c["H"], c["K"], 0, c["ln"], cus, bk, walk)
    if k == "nn":
        return ref.expected_path("nn", "bias", c["M"], c["N"], c["K"] + c["K2"], c["K"] if c["K2"] else 0, False, cus, bk)
    if k == "nn_bwd":
        return ref.expected_path("nn", "swiglu_bwd", c["M"], c["H"], c["K"], 0, False, cus, bk)
    if k == "tn":
        return ref.expected_path("tn", "bias", c["M"], c["N"] + c["N2"], c["K"], c["N"] if c["N2"] else 0, c["ln"], cus, bk,
                                 tn_slots=tn_slots)
    return ref.expected_path("row_stats", None, c["M"], c["D"], 0)


def case_features(c, cus):
    """{kernel instance and condition names} that the case reaches on a device of `cus` CUs (default switches)."""
    P = case_path(c, cus)
    k, slots = c["kind"], 2 * cus
    F = {P["instance"], f"{k} family {c['family']}"}
    if c.get("stride"):
        F.add(f"{k} stride {c['stride']}")
    if c["M"] == 1:
        F.add(f"{k} M=1")
    if k in ("nt", "nt2", "swiglu"):
        K = c["K"]
        if P["kernel"] == "nt_walk":
            t = P["tiles"]
            if slots < t < 2 * slots and t % P["grid"]:
                F.add("walk tiles in (slots, 2 slots)")
            if t > 2 * slots:
                F.add("walk tiles > 2 slots")
            if t == P["grid"] + 1:
                F.add("walk tiles = grid + 1")
            if P["max_tiles"] >= 2:
                F |= {f"walk M%128={c['M'] % 128}", f"walk K={K}", f"walk K%32={K % 32}", f"walk {k} {c.get('mode', '')}".strip()}
                if k == "nt2":
                    F.add("walk segment change" + (" ragged" if c["N2"] % 128 else ""))
                if k == "swiglu":
                    F.add(f"walk swiglu H%64={c['H'] % 64} keep={int(c['keep'])} b12={int(c['b12'])}")
        else:
            F |= {f"plain {k} {c.get('mode', '')}".strip(), f"plain K%32={K % 32}"}
        if k == "nt":
            F.add(f"nt N%128={c['N'] % 128}")
            if c.get("k96"):
                F.add("K=96 against K=100")
        if k == "swiglu":
            F.add(f"swiglu H%64={c['H'] % 64}")
    elif k == "nn":
        F |= {f"nn N%128={c['N'] % 128}", f"nn K%32={(c['K'] + c['K2']) % 32}"}
        if c["K2"] and c["K"] % 32:
            F.add("nn seam inside a step")
    elif k == "tn":
        nc, spc = P["nchunk"], P["steps_per_chunk"]
        last = c["M"] - (nc - 1) * spc * 32
        F |= {f"tn nchunk {nc}", f"tn bias {int(c['bias'])}", f"tn out {int(c['out'])}", "tn tiles <= 16" if P["tiles"] <= 16 else "tn tiles > 16"}
        if nc > 1 and last in (1, 33):
            F.add(f"tn last chunk {last}")
        if nc == cus:
            F.add("tn nchunk max")
        if nc == 1 and c["M"] < 256:
            F.add("tn M < 256 no workspace")
        if c["N2"]:
            F.add("tn two gradients" + (" ragged" if c["N2"] % 128 else ""))
    elif k == "stats":
        F |= {f"stats D={c['D']}", f"stats M={c['M']}"}
        if P["max_tiles"] > 1:
            F.add("stats grid wrap")
    return F


# ---------------------------------------------------------------------------------------------- running a case
class Canvas:
    """A (rows, cols) result inside a buffer of NaNs of one bit pattern: `guard` rows before and after, ld - cols guard
    columns."""

    def __init__(self, rows, cols, dev, pad=4, guard=3):
        self.ld = ld = cols + pad
        self.buf = torch.full(((rows + 2 * guard) * ld,), NANBITS, dtype=torch.int32, device=dev)
        self.view = self.buf.view(torch.float32)[guard * ld:(guard + rows) * ld].view(rows, ld)[:, :cols]
        self.mask = torch.zeros(rows + 2 * guard, ld, dtype=torch.bool, device=dev)
        self.mask[guard:guard + rows, :cols] = True

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf.view(-1, self.ld)[~self.mask] == NANBITS).all()), f"{what}: guard elements were written"
        return self.view


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


_LD = {"a": "lda", "a2": "lda2", "w": "ldw", "w2": "ldw2", "c": "ldc", "c2": "ldc2", "resid": "ldr", "ab": "ldab", "gate": "ldg"}


def make_desc(op, epi, M, N, K, split=0, **t):
    """(descriptor, the tensors it points to) for the C ABI."""
    from amk.lib import GemmDesc

    d = GemmDesc(op=op, epilogue=epi, m=M, n=N, k=K, split=split)
    for name, x in t.items():
        if x is None:
            continue
        setattr(d, name, _p(x))
        if name in _LD:
            setattr(d, _LD[name], x.stride(0))
    return d, t


def run_desc(d, keep, dev):
    """amk_gemm_f32 on the descriptor; returns the return code."""
    from amk import lib

    L = lib.load()
    n = L.amk_gemm_f32_ws_bytes(ctypes.byref(d))
    ws = torch.empty(max(n // 4, 1), device=dev, dtype=torch.float32)
    rc = L.amk_gemm_f32(ctypes.byref(d), _p(ws) if n else ctypes.c_void_p(0), n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _strided(t, how, dev):
    """The matrix t as a row-strided view on the device: "k+4" / "2k" leading dimension, "coloff" a 16-byte aligned
    column offset inside wider rows; the surroundings hold NaN."""
    M, K = t.shape
    if how is None:
        return t.to(dev)
    ld, off = {"k+4": (K + 4, 0), "2k": (2 * K, 0), "coloff": (K + 12, 8)}[how]
    big = torch.full((M, ld), float("nan"), device=dev)
    big[:, off:off + K] = t.to(dev)
    return big[:, off:off + K]


def _ln_of(a, D, dev):
    from amk import dense

    mean, rstd = dense.row_stats(a)
    return (mean, rstd, D["gamma"].to(dev), D["beta"].to(dev))


_LN_FIELDS = ("ln_mean", "ln_rstd", "ln_gamma", "ln_beta")


def _ln_args(ln):
    return dict(zip(_LN_FIELDS, ln)) if ln else {}


def _nt_inputs(c, dev, seed):
    """(data, a, w, bias, ln) of an nt / nt2 / swiglu case on the device."""
    if c["kind"] == "swiglu":
        D = ref.make_swiglu(c["family"], c["M"], c["H"], c["K"], seed)
    else:
        D = ref.make_nt(c["family"], c["M"], c["N"] + c.get("N2", 0), c["K"], seed)
    a = _strided(D["a"], c.get("stride"), dev)
    use_ln = c.get("ln", False) or "ln" in c.get("mode", "")
    return D, a, D["w"].to(dev), D["bias"].to(dev), (_ln_of(a, D, dev) if use_ln else None)


def _run_nt(c, dev, P, seed):
    from amk import dense

    what, M, N = c["id"], c["M"], c["N"]
    D, a, w, bias, ln = _nt_inputs(c, dev, seed)
    b = bias if "bias" in c["mode"] else None
    r = _strided(D["resid"], c.get("stride"), dev) if "resid" in c["mode"] else None
    R = ref.ref_nt(a, w, b, r, ln)
    cv = Canvas(M, N, dev, pad=12)
    out = dense.gemm_nt(a, w, b, resid=r, ln=ln, out=cv.view)
    assert out is cv.view
    got = cv.check(what).clone()
    ref.assert_within(got, R, "c", P["kernel"], what)
    cv2 = Canvas(M, N, dev, pad=0)
    dense.gemm_nt(a, w, b, resid=r, ln=ln, out=cv2.view)
    assert torch.equal(cv2.check(what + " rerun"), got), f"{what}: a rerun into ldc = N differs"
    if c.get("k96"):   # the plain kernel on the first 96 columns of the same data (columns 96.. of a are zero)
        a0 = a.clone()
        a0[:, 96:] = 0.0
        walk_out = dense.gemm_nt(a0, w, b)
        plain_out = dense.gemm_nt(a0[:, :96], w[:, :96], b)
        ref.assert_within(plain_out, ref.ref_nt(a0[:, :96], w[:, :96], b), "c", "nt", what + " K=96")
        assert torch.equal(walk_out, plain_out), f"{what}: K = 100 with a zero tail differs from K = 96"
    return {"c": got}


def _run_nt2(c, dev, P, seed):
    from amk import dense
    from amk.lib import EPI_BIAS, GEMM_NT

    what, M, K, N1, N2, kern = c["id"], c["M"], c["K"], c["N"], c["N2"], P["kernel"]
    D, a, w, bias, ln = _nt_inputs(c, dev, seed)
    w1, w2, b1, b2 = w[:N1], w[N1:], bias[:N1].clone(), bias[N1:].clone()
    R = ref.ref_nt2(a, w1, b1, w2, b2, ln)
    cv = Canvas(M, N1, dev, pad=4)
    c1, c2 = dense.gemm_nt(a, w1, b1, w2=w2, bias2=b2, ln=ln, out=cv.view)
    ref.assert_within(cv.check(what), R, "c", kern, what)
    ref.assert_within(c2, R, "c2", kern, what)
    # the same launch through the descriptor: both outputs in canvases of different leading dimensions
    v1, v2 = Canvas(M, N1, dev, pad=8), Canvas(M, N2, dev, pad=20)
    d, keep = make_desc(GEMM_NT, EPI_BIAS, M, N1 + N2, K, N1, a=a, w=w1, w2=w2, c=v1.view, c2=v2.view, bias=b1, bias2=b2, **_ln_args(ln))
    assert run_desc(d, keep, dev) == 0
    assert torch.equal(v1.check(what + " desc"), c1) and torch.equal(v2.check(what + " desc c2"), c2)
    s1, s2 = dense.gemm_nt(a, w1, b1, ln=ln), dense.gemm_nt(a, w2, b2, ln=ln)
    assert torch.equal(s1, c1) and torch.equal(s2, c2), f"{what}: the two-projection launch differs from two launches"
    return {"c": c1.clone(), "c2": c2}


def _run_swiglu(c, dev, P, seed):
    from amk import dense
    from amk.lib import EPI_SWIGLU, GEMM_NT

    what, M, K, H = c["id"], c["M"], c["K"], c["H"]
    D, a, w, bias, ln = _nt_inputs(c, dev, seed)
    b12 = bias if c["b12"] else None
    R = ref.ref_nt_swiglu(a, w, b12, ln)
    g, ab = dense.gemm_nt_swiglu(a, w, b12, ln=ln, keep_ab=c["keep"])
    ref.assert_within(g, R, "g", "nt_swiglu", what)
    if c["family"] != "saturate":
        assert not bool(R["under_g"].any()), f"{what}: the under allowance is used outside the saturate family"
    vg = Canvas(M, H, dev, pad=4)
    vab = Canvas(M, 2 * H, dev, pad=8) if c["keep"] else None
    d, keep = make_desc(GEMM_NT, EPI_SWIGLU, M, H, K, 0, a=a, w=w, gate=vg.view, c=vab.view if vab else None, bias=b12, **_ln_args(ln))
    d.ldc = vab.ld if vab else 2 * H
    assert run_desc(d, keep, dev) == 0
    assert torch.equal(vg.check(what + " desc"), g), f"{what}: the padded gate differs"
    if not c["keep"]:
        assert ab is None
        return {"g": g}
    ref.assert_within(ab, R, "ab", P["kernel"], what)
    assert torch.equal(vab.check(what + " desc ab"), ab)
    return {"g": g, "ab": ab}


def _run_nn(c, dev, P, seed):
    from amk import dense
    from amk.lib import EPI_BIAS, GEMM_NN

    what, M, N, K, K2 = c["id"], c["M"], c["N"], c["K"], c["K2"]
    D = ref.make_nn(c["family"], M, N, K, seed, K2)
    a, w = _strided(D["a"], c.get("stride"), dev), D["w"].to(dev)
    a2, w2 = (D["a2"].to(dev), D["w2"].to(dev)) if K2 else (None, None)
    got = dense.gemm_nn(a, w, a2=a2, w2=w2)
    ref.assert_within(got, ref.ref_nn(a, w, a2, w2), "c", "nn", what)
    cv = Canvas(M, N, dev, pad=12)
    d, keep = make_desc(GEMM_NN, EPI_BIAS, M, N, K + K2, K if K2 else 0, a=a, w=w, a2=a2, w2=w2, c=cv.view)
    assert run_desc(d, keep, dev) == 0
    assert torch.equal(cv.check(what + " desc"), got), f"{what}: the padded result differs"
    return {"c": got}


def _run_nn_bwd(c, dev, P, seed):
    from amk import dense
    from amk.lib import EPI_SWIGLU_BWD, GEMM_NN

    what, M, H, K = c["id"], c["M"], c["H"], c["K"]
    D = ref.make_swiglu_bwd(c["family"], M, H, K, seed)
    dy, w3, ab = D["dy"].to(dev), D["w3"].to(dev), _strided(D["ab"], "k+4", dev)
    R = ref.ref_nn_swiglu_bwd(dy, w3, ab)
    got = dense.gemm_nn(dy, w3, swiglu_ab=ab)
    ref.assert_within(got, R, "dab", "nn_swiglu_bwd", what)
    if c["family"] != "saturate":
        assert not bool(R["under_dab"].any()), f"{what}: the under allowance is used outside the saturate family"
    cv = Canvas(M, 2 * H, dev, pad=8)
    d, keep = make_desc(GEMM_NN, EPI_SWIGLU_BWD, M, H, K, 0, a=dy, w=w3, ab=ab, c=cv.view)
    assert run_desc(d, keep, dev) == 0
    assert torch.equal(cv.check(what + " desc"), got), f"{what}: the padded result differs"
    return {"dab": got}


def _run_tn(c, dev, P, seed, bk):
    from amk import dense
    from amk.lib import EPI_BIAS, GEMM_TN

    what, M, N1, N2, K, bias = c["id"], c["M"], c["N"], c["N2"], c["K"], c["bias"]
    D = ref.make_tn(c["family"], M, N1, K, seed, N2)
    y, x = _strided(D["y"], c.get("stride"), dev), _strided(D["x"], c.get("stride"), dev)
    y2 = D["y2"].to(dev) if N2 else None
    ln = _ln_of(x, D, dev) if c["ln"] else None
    R = ref.ref_tn(y, x, y2, ln, bias, P["steps_per_chunk"], P["nchunk"], bk)
    o1 = o2 = ob = None
    if c["out"]:       # out= / out2= / bias_out=: contiguous views (what _out demands) with guard rows around them
        o1 = Canvas(N1, K, dev, pad=0)
        o2 = Canvas(N2, K, dev, pad=0) if N2 else None
        ob = Canvas(1, N1 + N2, dev, pad=0) if bias else None
    dw, dw2, db = dense.gemm_tn(y, x, y2=y2, ln=ln, want_bias=bias, out=o1.view if o1 else None,
                                out2=o2.view if o2 else None, bias_out=ob.view[0] if ob else None)
    for cvs in (o1, o2, ob):
        if cvs is not None:
            cvs.check(what + " out=")
    ref.assert_within(dw, R, "dw", "tn_dw", what)
    if N2:
        ref.assert_within(dw2, R, "dw2", "tn_dw", what)
    if bias:
        ref.assert_within(db, R, "db", "tn_db", what)
    else:
        assert db is None
    # through the descriptor: padded leading dimensions, guards around the bias gradient (this is the rerun check too)
    v1 = Canvas(N1, K, dev, pad=8)
    v2 = Canvas(N2, K, dev, pad=4) if N2 else None
    vb = Canvas(1, N1 + N2, dev, pad=4) if bias else None
    d, keep = make_desc(GEMM_TN, EPI_BIAS, M, N1 + N2, K, N1 if N2 else 0, a=y, w=x, a2=y2, c=v1.view, c2=v2.view if v2 else None,
                        dbias=vb.view[0] if vb else None, **_ln_args(ln))
    assert run_desc(d, keep, dev) == 0
    assert torch.equal(v1.check(what + " desc"), dw), f"{what}: the padded gradient differs"
    res = {"dw": dw.clone()}
    if N2:
        assert torch.equal(v2.check(what + " desc dw2"), dw2)
        res["dw2"] = dw2.clone()
    if bias:
        assert torch.equal(vb.check(what + " desc db")[0], db)
        res["db"] = db.clone()
    return res


def _run_stats(c, dev, P, seed):
    from amk import dense, lib

    what, M, Dm = c["id"], c["M"], c["D"]
    x = ref.make_act(c["family"], M, Dm, seed).to(dev)
    R = ref.ref_row_stats(x)
    mean, rstd = dense.row_stats(x)
    ref.assert_within(mean, R, "mean", "row_stats_mean", what)
    ref.assert_within(rstd, R, "rstd", "row_stats_rstd", what)
    vm, vr = Canvas(1, M, dev, pad=4 + (-M) % 4), Canvas(1, M, dev, pad=4 + (-M) % 4)
    rc = lib.load().amk_row_stats(_p(x), M, Dm, 1e-5, _p(vm.view), _p(vr.view), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert torch.equal(vm.check(what + " mean")[0], mean) and torch.equal(vr.check(what + " rstd")[0], rstd)
    return {"mean": mean, "rstd": rstd}


def run_case(c, dev, cus, bk=32, walk=True, tn_slots=0):
    """Runs the case with canvases, checks guards, bounds and the rerun; returns {name: result tensor}."""
    P = case_path(c, cus, bk, walk, tn_slots)
    seed = sum(map(ord, c["id"]))
    if c["kind"] == "tn":
        return _run_tn(c, dev, P, seed, bk)
    run = {"nt": _run_nt, "nt2": _run_nt2, "swiglu": _run_swiglu, "nn": _run_nn, "nn_bwd": _run_nn_bwd, "stats": _run_stats}
    return run[c["kind"]](c, dev, P, seed)


# ---------------------------------------------------------------------------------------------- the tests
def _cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


@pytest.fixture(scope="module")
def report():
    """Prints the worst hard ratio and q / limit per kernel after the module's tests (visible with -s)."""
    yield
    print("\nworst hard ratio, q / limit per kernel:", {k: [round(v, 4) for v in w] for k, w in ref.WORST.items()})


@pytest.mark.parametrize("case_id", [c["id"] for c in cases(256)])   # (the ids are the same for every CU count)
def test_case(device, report, case_id):
    cus = _cus(device)
    (c,) = [c for c in cases(cus) if c["id"] == case_id]
    run_case(c, device, cus)


def test_case_list_reaches_every_path_on_this_device(device):
    cus = _cus(device)
    got = set().union(*(case_features(c, cus) for c in cases(cus)))
    assert not (required_features(cus) - got), sorted(required_features(cus) - got)


def required_features(cus):
    """What the case list must reach on a device of `cus` CUs."""
    F = {f"nt_walk<{e},{ln}>" for e in ("bias", "resid", "swiglu") for ln in (0, 1)}
    F |= {f"nt<32,{e},{ln}>" for e in ("bias", "resid", "swiglu") for ln in (0, 1)}
    F |= {"nn<32,bias>", "nn<32,swiglu_bwd>", "tn<32,0>", "tn<32,1>", "row_stats<1>", "row_stats<4>", "row_stats<16>"}
    F |= {"walk tiles in (slots, 2 slots)", "walk tiles > 2 slots", "walk tiles = grid + 1", "walk M%128=1", "walk M%128=127",
          "walk K=100", "walk K=128", "walk K%32=4", "walk K=1368", "walk nt bias", "walk nt plain", "walk nt resid",
          "walk nt ln_bias_resid", "walk segment change ragged", "K=96 against K=100"}
    F |= {f"walk swiglu H%64={h} keep={k} b12={b}" for h, k, b in ((0, 1, 1), (4, 0, 1), (36, 1, 0), (36, 0, 0))}
    F |= {f"{k} N%128={r}" for k in ("nt", "nn") for r in (4, 124)} | {f"nn K%32={r}" for r in (4, 28)} | {f"plain K%32={r}" for r in (4, 28)}
    F |= {"nt M=1", "nn M=1", "tn M=1", "nt stride k+4", "nt stride 2k", "nt stride coloff", "nn stride k+4", "nn stride 2k", "nn stride coloff",
          "tn stride k+4", "tn stride 2k", "tn stride coloff", "nn seam inside a step", "nn_bwd family cancel", "nn_bwd family saturate",
          "swiglu family saturate"}
    F |= {f"tn nchunk {n}" for n in (1, 2, 8, 9, 15)} | {"tn nchunk max", "tn last chunk 1", "tn last chunk 33", "tn tiles <= 16",
                                                         "tn tiles > 16", "tn two gradients ragged", "tn bias 0", "tn bias 1", "tn out 0",
                                                         "tn out 1", "tn M < 256 no workspace"}
    F |= {f"stats D={d}" for d in (4, 256, 260, 1024, 1028, 4096)} | {"stats M=1", "stats M=5", "stats M=65541", "stats grid wrap"}
    F |= {f"stats family {f}" for f in ref.LN_FAMILIES}
    return F


@pytest.mark.parametrize("kind,M,N,K,mode", [("nt", 2305, 3700, 128, "ln_bias_resid"), ("nt", 300, 260, 64, "bias"), ("nn", 300, 260, 100, None)])
def test_rows_do_not_depend_on_the_other_rows(device, kind, M, N, K, mode):
    """M against M + 128 rows: the first M rows are the same bits (the walk hands the tiles to other workgroups)."""
    from amk import dense

    if kind == "nt":
        D = ref.make_nt("binade", M + 128, N, K, 7)
        a, w, b, r = (D[n].to(device) for n in ("a", "w", "bias", "resid"))
        ln = _ln_of(a, D, device) if "ln" in mode else None
        big = dense.gemm_nt(a, w, b, resid=r if "resid" in mode else None, ln=ln)
        small = dense.gemm_nt(a[:M], w, b, resid=r[:M] if "resid" in mode else None, ln=tuple(t[:M] for t in ln[:2]) + ln[2:] if ln else None)
    else:
        D = ref.make_nn("binade", M + 128, N, K, 7)
        a, w = D["a"].to(device), D["w"].to(device)
        big, small = dense.gemm_nn(a, w), dense.gemm_nn(a[:M], w)
    assert torch.equal(big[:M], small)


@pytest.mark.parametrize("M0,N1,N2,K", [(2048, 128, 256, 64), (700, 256, 100, 40), (5000, 512, 1024, 256), (255, 128, 36, 132)])
def test_tn_two_gradients_equal_two_calls(device, M0, N1, N2, K):
    """Where tn_chunks cuts the joint launch and a single launch alike, they are the same sums in the same order.  M is
    the first one from M0 on for which that holds on this device for at least one of the two gradients."""
    from amk import dense

    cus = _cus(device)
    cuts = lambda M: [ref.tn_chunks(M, n, K, cus) for n in (N1 + N2, N1, N2)]
    M = next(M for M in range(M0, M0 + 4096) if cuts(M)[0] in cuts(M)[1:])
    joint, one, two = cuts(M)
    D = ref.make_tn("outlier_rows", M, N1, K, 9, N2)
    y, y2, x = D["y"].to(device), D["y2"].to(device), D["x"].to(device)
    dw, dw2, db = dense.gemm_tn(y, x, y2=y2, want_bias=True)
    if joint == one:
        s, _, sb = dense.gemm_tn(y, x, want_bias=True)
        assert torch.equal(s, dw) and torch.equal(sb, db[:N1])
    if joint == two:
        s, _, sb = dense.gemm_tn(y2, x, want_bias=True)
        assert torch.equal(s, dw2) and torch.equal(sb, db[N1:])


def test_ops_compose_from_dense_calls(device, monkeypatch):
    """ops.linear and ops.swiglu_ffn in f32 are the dense.* calls of their autograd functions, bit for bit."""
    from amk import dense, ops

    monkeypatch.setattr(ops, "DENSE_MODE", "amk")
    g = torch.Generator().manual_seed(3)
    n = lambda *s: torch.randn(*s, generator=g).to(device)
    x, w, b, dy = n(3, 100, 256), n(516, 256) / 16, n(516), n(3, 100, 516)
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    out = ops.linear(xr, wr, br)
    out.backward(dy)
    x2, dy2 = x.view(-1, 256), dy.view(-1, 516)
    assert torch.equal(out.view(-1, 516), dense.gemm_nt(x2, w, b))
    assert torch.equal(xr.grad.view(-1, 256), dense.gemm_nn(dy2, w))
    dw, _, db = dense.gemm_tn(dy2, x2, want_bias=True)
    assert torch.equal(wr.grad, dw) and torch.equal(br.grad, db)

    w12, b12, w3, b3, do = n(2 * 684, 256) / 16, n(2 * 684), n(256, 684) / 26, n(256), n(3, 100, 256)
    ps = [t.clone().requires_grad_() for t in (x, w12, b12, w3, b3)]
    out = ops.swiglu_ffn(*ps)
    out.backward(do)
    gate, ab = dense.gemm_nt_swiglu(x2, w12, b12, keep_ab=True)
    assert torch.equal(out.view(-1, 256), dense.gemm_nt(gate, w3, b3))
    d2 = do.view(-1, 256)
    d_ab = dense.gemm_nn(d2, w3, swiglu_ab=ab)
    dw3, _, db3 = dense.gemm_tn(d2, gate, want_bias=True)
    dw12, _, db12 = dense.gemm_tn(d_ab, x2, want_bias=True)
    for got, want in zip([p.grad for p in ps], [dense.gemm_nn(d_ab, w12).view(3, 100, 256), dw12, db12, dw3, db3]):
        assert torch.equal(got, want)


def test_refusals_by_return_code(device):
    """split not a multiple of 128, K % 4, misaligned pointers: refused (nothing is launched)."""
    from amk.lib import EPI_BIAS, GEMM_NT, GEMM_TN

    t = lambda *s: torch.zeros(*s, device=device)
    a, w, w2, cc, c2 = t(64, 64), t(192, 64), t(64, 64), t(64, 192), t(64, 64)
    ok, keep = make_desc(GEMM_NT, EPI_BIAS, 64, 192, 64, 128, a=a, w=w, w2=w2, c=cc, c2=c2)
    assert run_desc(ok, keep, device) == 0
    bad, keep = make_desc(GEMM_NT, EPI_BIAS, 64, 192, 64, 64, a=a, w=w, w2=w2, c=cc, c2=c2)
    assert run_desc(bad, keep, device) != 0
    bad, keep = make_desc(GEMM_TN, EPI_BIAS, 64, 192, 64, 64, a=cc, w=a, a2=c2, c=t(192, 64), c2=t(64, 64))
    assert run_desc(bad, keep, device) != 0
    bad, keep = make_desc(GEMM_NT, EPI_BIAS, 64, 192, 62, 0, a=a, w=w, c=cc)
    assert run_desc(bad, keep, device) != 0
    big = t(64 * 64 + 4)
    for name in ("a", "w", "c"):
        args = dict(a=a, w=w[:64], c=c2)
        args[name] = big[1:1 + 64 * 64].view(64, 64)
        bad, keep = make_desc(GEMM_NT, EPI_BIAS, 64, 64, 64, 0, **args)
        assert run_desc(bad, keep, device) != 0, name


# ---------------------------------------------------------------------------------------------- the switches
def _child_config():
    e = os.environ
    bk = 16 if e.get("AMK_DENSE_BK") == "16" else 32
    walk = not e.get("AMK_DENSE_WALK", "1").startswith("0")
    slots = int(e.get("AMK_DENSE_TN_SLOTS", "0") or 0)
    return bk, walk, slots


def child_main(path):
    """Runs reduced_cases() under this process's switches with canvases and bounds; saves every result."""
    dev = torch.device("cuda:0")
    cus = _cus(dev)
    bk, walk, slots = _child_config()
    out = {}
    for c in reduced_cases(cus):
        for name, t in run_case(c, dev, cus, bk, walk, slots).items():
            out[f"{c['id']}.{name}"] = t.cpu().numpy()
    np.savez(path, **out)
    print("worst:", {k: [round(v, 4) for v in w] for k, w in ref.WORST.items()})


def _run_child(tmp_path, name, var=None, value=None):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if var:
        env[var] = value
    path = str(tmp_path / f"{name}.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), path]
    r = subprocess.run(cmd, env=env, timeout=900, capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"child {name} ({var}={value}) failed with {r.returncode}:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


@pytest.mark.parametrize("var,value,bitwise", [("AMK_DENSE_WALK", "0", "all"), ("AMK_DENSE_STAGGER", "3,2", "all"), ("AMK_DENSE_BK", "16", None),
                                               ("AMK_DENSE_TN_SLOTS", "6", "not_tn")])
def test_switch_in_a_child_process(device, tmp_path, var, value, bitwise):
    """The child holds every case to the bounds and canvases under the switch; the parent compares the bits the source
    promises with a child under the default settings (one child at a time; nothing is started after a failure)."""
    cus = _cus(device)
    if var == "AMK_DENSE_TN_SLOTS":
        c = [c for c in reduced_cases(cus) if c["id"] == "r_tn"][0]
        assert case_path(c, cus, tn_slots=int(value))["nchunk"] != case_path(c, cus)["nchunk"], "the value must change nchunk"
    base = _run_child(tmp_path, "default")
    got = _run_child(tmp_path, "switch", var, value)
    assert set(got) == set(base)
    for key in sorted(base):
        if bitwise == "all" or (bitwise == "not_tn" and not key.startswith("r_tn")):
            assert _same_bits(got[key], base[key]), f"{var}={value}: {key} differs from the default's bits"


if __name__ == "__main__":
    child_main(sys.argv[1])
