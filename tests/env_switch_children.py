"""What the children of tests/test_env_switches_gpu.py run: one function per tuning switch that the library reads once per
process (csrc/attn_decode.hip:207, csrc/gemm_bf16.hip:453-478, csrc/gemm_x6_tn.hip:237, csrc/moe.hip:1424 and :1521).  The
parent sets the variable in the child's environment; the child runs the family's existing check -- its fp64 reference and
per-element bound from tests/*_ref.py, told the forced tile or chunk where the bound depends on it -- at shapes chosen so
that the forced value gives a tile / chunk / shape combination the default rule does not, and raises on a violation.

    python -c "import env_switch_children as c; c.main('decode_keys')"      (sys.path as tests/conftest.py sets it)
"""
import contextlib
import os

import torch

F32, BF16 = torch.float32, torch.bfloat16


def _device():
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible")
    return torch.device("cuda:0")


def _forced(name):
    v = os.environ.get(name)
    if v is None:
        raise SystemExit(f"{name} is not set in this process: the parent did not pass it")
    return int(v)


# ---------------------------------------------------------------------------------------------- AMK_ATTN_DECODE_KEYS
def decode_keys():
    """ops.attention_decode, f32 and bf16 caches, append and read mode, against attn_decode_ref / attn_decode_bf16_ref (the
    check of the stale-memory sweep's decode family): (B, H, D, cap, n) = (2, 2, 64, 300, 129) masked and (1, 2, 96, 77, 65),
    and n -- the kernel sees n + 1 keys in append mode -- on either side of the forced chunk size.  The references do not
    model the chunking: their bounds hold for any split of the keys."""
    from amk import ops
    from test_stale_memory_gpu import _decode_fn, _decode_ref

    dev, keys = _device(), _forced("AMK_ATTN_DECODE_KEYS")
    assert keys in (32, 128)
    for (B, H, D, cap, n0, masked) in ((2, 2, 64, 300, 129, True), (1, 2, 96, 77, 65, False)):
        # the workspace grows with the chunks per row: sized in this process, with the forced value
        floats = ops.attention_decode_ws_floats(B, H, D, cap)
        assert floats >= B * H * -(-cap // keys) * (D + 2), (floats, keys)
        for n in sorted({n0, keys - 2, keys - 1, keys, keys + 1, 2 * keys - 1, 2 * keys}):
            if n + 1 > cap:
                continue
            for dt in (F32, BF16):
                got = _decode_fn(B, H, D, cap, n, dt, masked)(dev)
                torch.cuda.synchronize()
                _decode_ref(B, H, D, cap, n, masked, dt)(got, dev)
                print(f"decode keys {keys}: B{B} H{H} D{D} cap{cap} n{n} {dt} inside the bound")


# ---------------------------------------------------------------------------------------------- AMK_TN16_TK, AMK_TN16_WGS
def _tn16(shapes, tk=None, wgs=1):
    """The TN check of tests/test_bf16_dense_bounds_gpu.py (test_tn_bounds) with bf16_dense_ref's bound, the reference's
    chunking told the forced tile width / workgroups per CU.  Every family is held to the per-element bound; the test's second
    figure, 2e-5 of the result's largest element, is asked of the family the shape has in that test's TN_CASES, as there.  (It
    is no bound: the `cancel` family's results are 1 / 64 of their terms.  At (1000, 256, 256) under AMK_TN16_WGS=4, where
    the forced chunking is the default's and the launch therefore the default's own, that family is inside its per-element
    bound and outside the 2e-5.)"""
    import bf16_dense_ref as ref
    from test_bf16_dense_bounds_gpu import GF, TN_CASES, _b16, _cus, _tn_kernel_names
    from util import rel_err

    dev = _device()
    for (M, N, K) in shapes:
        i = TN_CASES.index((M, N, K))
        for fam in GF[:4]:
            y, x = ref.make_tn(fam, M, N, K, 100 + i)
            (dw, db), names = _tn_kernel_names(dev, _b16(y, dev), _b16(x, dev))
            width = ref.tn_tile_k(N, K, tk)
            assert names and all(f"<2, {width // 64}>" in n or f"ILi2ELi{width // 64}E" in n for n in names), (width, names)
            R = ref.ref_tn(y, x, _cus(), tk=tk, wgs=wgs)
            ref.assert_within({"dw": dw, "db": db}, R, ("dw", "db"), f"tn {fam} {M}x{N}x{K} tk {tk} wgs {wgs}", key="tn")
            if fam == GF[i % 4]:
                assert rel_err(dw, R["dw"]) < 2e-5 and rel_err(db, R["db"]) < 2e-5
            print(f"tn16 tk {tk} wgs {wgs}: {fam} {M}x{N}x{K} on the {width}-wide tile inside the bound")


def tn16_tk():
    import bf16_dense_ref as ref

    tk = _forced("AMK_TN16_TK")
    shape = {256: (65, 136, 264), 128: (1000, 1024, 512)}[tk]       # the default rule gives the other width there
    assert ref.tn_tile_k(*shape[1:]) == 384 - tk
    _tn16([shape], tk=tk)


def tn16_wgs():
    """(1000, 256, 256): with 16 steps of 64 rows the cap of 8 steps per chunk decides the chunking at either setting, so
    this shape holds the switch's read path alone; at (40000, 264, 136) four workgroups per CU cut the rows into 70 chunks
    where the default makes 42 (at 256 CUs), and the bound follows through tn_chunks(wgs=)."""
    import bf16_dense_ref as ref
    from test_bf16_dense_bounds_gpu import _cus

    wgs = _forced("AMK_TN16_WGS")
    assert wgs == 4
    assert ref.tn_chunks(40000, 264, 136, _cus(), wgs=wgs) != ref.tn_chunks(40000, 264, 136, _cus())
    _tn16([(1000, 256, 256), (40000, 264, 136)], wgs=wgs)


# ---------------------------------------------------------------------------------------------- AMK_X6_TN_TK
def x6_tn_tk():
    """dense.gemm_x6_tn against gemm_x6_tn_ref (tests/test_gemm_x6_tn_gpu.py's check), geometry and bound told the forced
    tile: 128 on the 708 x 260 gradient (the default's eight-wave case), 256 on a 12 x 52 one (70 rows)."""
    import dense_f32_ref as R32
    import gemm_x6_tn_ref as T
    from amk import dense
    from test_gemm_x6_tn_gpu import check

    dev, tk = _device(), _forced("AMK_X6_TN_TK")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    cases = {128: [(33, 708, 260), (333, 708, 260), (1100, 708, 260)], 256: [(70, 12, 52), (1, 12, 52), (600, 12, 52)]}[tk]
    for M, N, K in cases:
        assert T.tile_k(N, K) == 384 - tk                           # the default rule gives the other width there
        geo = T.geometry(M, N, K, cus, tk=tk)
        assert dense.x6_tn_chunks(M, N, K) == geo[0], (dense.x6_tn_chunks(M, N, K), geo)
        for family in T.FAMILIES:
            D = R32.make_tn(family, M, N, K, seed=7 * M + N + K)
            R = T.ref_tn(D["y"], D["x"], geo=geo)
            dw, _, db = dense.gemm_x6_tn(D["y"].to(dev), D["x"].to(dev), want_bias=True)
            what = f"x6 tn tk {tk}: {family} M{M} N{N} K{K} chunks {geo[0]}"
            check(dw, R, "dw", what)
            check(db, R, "db", what)
            again = dense.gemm_x6_tn(D["y"].to(dev), D["x"].to(dev), want_bias=True)
            assert torch.equal(again[0], dw) and torch.equal(again[2], db), f"{what}: not reproducible"


# ---------------------------------------------------------------------------------------------- AMK_MOE_SHORT, AMK_MOE_WGRAD_SPLIT
def _moe(cases, entry_of, want):
    """The grouped-GEMM bound check of tests/test_moe_bounds_gpu.py (test_grouped_gemms) on cases for which the default
    rule, as tests/moe_ref.py models it, takes `want`; this process runs the fallback kernels instead."""
    import moe_ref
    import test_moe_bounds_gpu as M

    dev = _device()
    slots = M._slots()
    for c in cases:
        counts, P = M._case_counts(c)
        for entry in entry_of(c):
            name = moe_ref.expected_path(entry, P, c["E"], c["N"], c["Kd"], 0, counts, slots)
            assert want in name, f"{c['id']} {entry}: the default rule picks {name}, not {want}"
        M.test_grouped_gemms(dev, c, lambda narrow: contextlib.nullcontext())
        print(f"moe {c['id']}: inside the bound on the fallback of {want}")


def moe_short():
    """csrc/moe.hip:1459: the default takes the 32-pair tiles where the outputs fit one 64-wide tile, the contraction is 256
    or longer and the tiles are few.  The smallest such shapes (one pair; 4 outputs), and the tile edges."""
    import test_moe_bounds_gpu as M

    assert _forced("AMK_MOE_SHORT") == 0
    cases = [M.C("short_nt_smallest", "unit", ("counts", [1]), 1, 4, 256, entries=("nt",)),
             M.C("short_nt_edges", "expert_scale", ("counts", [0, 1, 31, 33, 65, 0]), 6, 64, 256, 2, 2, entries=("nt",)),
             M.C("short_nn_smallest", "unit", ("counts", [1]), 1, 256, 4, entries=("nn",)),
             M.C("short_nn_edges", "binade", ("counts", [0, 1, 31, 33, 65, 0]), 6, 256, 64, 2, 2, entries=("nn",))]
    _moe(cases, lambda c: c["entries"], "short>")


def moe_wgrad_split():
    """csrc/moe.hip:1523: the default cuts the pairs of a tile in two where the tiles fill at most half the workgroup slots
    and an expert has 256 pairs or more on average.  The smallest such shapes on each wide tile."""
    import test_moe_bounds_gpu as M

    assert _forced("AMK_MOE_WGRAD_SPLIT") == 0
    cases = [M.C("split_64x128_smallest", "unit", ("counts", [256]), 1, 64, 128, entries=("wgrad",)),
             M.C("split_128x64", "expert_scale", ("counts", [255, 258]), 2, 128, 64, 2, 2, entries=("wgrad",)),
             M.C("split_128x128", "binade", ("counts", [300, 0, 513]), 3, 128, 128, 2, 2, entries=("wgrad",))]
    _moe(cases, lambda c: ("wgrad", "wgrad_noscale"), "rsplit 2")


CHILDREN = {"decode_keys": decode_keys, "tn16_tk": tn16_tk, "tn16_wgs": tn16_wgs, "x6_tn_tk": x6_tn_tk,
            "moe_short": moe_short, "moe_wgrad_split": moe_wgrad_split}


def main(name):
    CHILDREN[name]()
    torch.cuda.synchronize()
    print(f"{name}: ok")
