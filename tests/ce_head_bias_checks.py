"""What tests/test_ce_head_bias_gpu.py (f32) and tests/test_ce_head_bias_bf16_gpu.py (bf16 autocast) share: the op with
a bias against both tiers of tests/ce_head_bias_ref.py.  A Head carries the mode; every check_* is one test's body."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ce_head_bias_ref as ref

D_LOSS = 0.7
BF16 = torch.bfloat16
PATTERNS = ["all", "first", "last", "last_tile", "random64", "edges"]
VALID_COUNTS = [1, 15, 16, 17, 31, 32, 33, 129]   # around the 16-row stage of dw and the 32 row groups of ce_bwd_db
GRAPH_PATTERNS = ("first", "last_tile", "all", "none", "random64")


def _same(a, b):
    return torch.equal(a, b) or (bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()))


class Head:
    def __init__(self, bf16):
        self.bf16 = bf16
        self.k_small, self.k_big = (40, 264) if bf16 else (36, 260)
        self.ks = [8, 40, 64, 264] if bf16 else [4, 36, 64, 260]
        self.worst = {}   # name -> [hard ratio, q / (TIGHT_FACTOR Q_EMU)]

    # ------------------------------------------------------------------------------------------ the op
    def op(self, x, w, b, target, ignore_index=-1, d_loss=D_LOSS):
        """(loss f32, dx in x's dtype, dw f32, db f32); b None: the biasless op (db None).  Under bf16: x bf16, w bf16
        values held by an f32 master weight, the bias f32."""
        from amk import ops

        xg, wg = x.detach().clone().requires_grad_(), w.detach().float().requires_grad_()
        bg = b.detach().clone().requires_grad_() if b is not None else None
        kw = {} if bg is None else dict(bias=bg)
        if self.bf16:
            with torch.autocast("cuda", dtype=BF16):
                loss = ops.linear_cross_entropy(xg, wg, target, ignore_index, **kw)
        else:
            loss = ops.linear_cross_entropy(xg, wg, target, ignore_index, **kw)
        (loss * d_loss).backward()
        assert loss.dtype == torch.float32 and xg.grad.dtype == x.dtype and wg.grad.dtype == torch.float32
        assert bg is None or (bg.grad.dtype == torch.float32 and bg.grad.shape == b.shape)
        return loss.detach(), xg.grad, wg.grad, (bg.grad if bg is not None else None)

    def reference(self, x, w, b, t, ignore_index=-1):
        return ref.reference(x, w, b, t, ignore_index, D_LOSS, bf16=self.bf16)

    def hold(self, got, R, what):
        for name, g in zip(ref.NAMES, got):
            nbad, ratio, q = ref.measures(g, R, name)
            limit = ref.TIGHT_FACTOR * ref.Q_EMU[self.bf16][name]
            tight = q / limit
            print(f"{what} {name}: hard ratio {ratio:.4f}, q {q:.4f} ({tight:.4f} of the tight limit)")
            w = self.worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], ratio), max(w[1], tight)
            assert nbad == 0, f"{what} {name}: {nbad} elements outside the hard bound (worst {ratio:.3f} x)"
            assert tight <= 1.0, f"{what} {name}: q {q:.3f} above {ref.TIGHT_FACTOR} x Q_EMU = {limit}"

    def inputs(self, family, bfam, M, V, K, pattern, device, seed=0):
        target = ref.make_target(M, V, pattern, seed=seed)
        x, w = ref.make_inputs(family, M, V, K, target, seed=seed + K, bf16=self.bf16)
        b = ref.make_bias(bfam, x, w, target, seed=seed + V)
        return x.to(device), w.to(device), b.to(device), target.to(device)

    def sweep_cases(self):
        """The seeded sweep of the biasless tests (every M, V and K of the tile-edge lists at least once) with the bias
        families rotating, plus the three large cases with a unit bias."""
        Ms, Vs, Ks = [1, 127, 128, 129, 300], [1, 4, 127, 128, 129, 1000], self.ks
        g = torch.Generator().manual_seed(7)
        n = max(len(Ms), len(Vs), len(Ks))
        cols = []
        for vals in (Ms, Vs, Ks):
            order = [vals[i] for i in torch.randperm(len(vals), generator=g).tolist()]
            cols.append([order[i % len(order)] for i in range(n)])
        fams, bfams = ref.FAMILIES, ref.BIAS_FAMILIES[1:]
        cases = [(cols[0][i], cols[1][i], cols[2][i], fams[i % len(fams)], bfams[i % len(bfams)]) for i in range(n)]
        cases += [(300, 8192, 64, "unit", "unit"), (129, 128, 1024, "peaked", "unit"), (300, 8192, 1024, "climb", "unit")]
        return cases

    # ------------------------------------------------------------------------------------------ the checks
    def check_case(self, device, M, V, K, family, bfam, pattern=None, seed=None, what="case"):
        pattern = pattern or ("all" if M == 1 else "random64")
        x, w, b, t = self.inputs(family, bfam, M, V, K, pattern, device, seed=M + V if seed is None else seed)
        self.hold(self.op(x, w, b, t), self.reference(x, w, b, t), f"{what} {M}x{V}x{K} {family} x {bfam} {pattern}")

    def check_valid_count(self, device, n):
        M, V, K = 300, 1000, self.k_big
        x, w, b, t = self.inputs("unit", "unit", M, V, K, "all", device)
        keep = torch.randperm(M, generator=torch.Generator().manual_seed(n))[:n].to(device)
        t2 = torch.full_like(t, -1)
        t2[keep] = t[keep]
        self.hold(self.op(x, w, b, t2), self.reference(x, w, b, t2), f"{n} valid rows")

    def check_boundaries(self, device):
        """Targets on both sides of every slice / tile boundary, four tiles per slice; a dominant bias whose largest
        entries sit on the boundary words."""
        M, V, K = 300, 8192, self.k_small
        ns, vper = ref.slices(M, V)
        assert vper // ref.TILE == 4 and ns == 16
        x, w, b, t = self.inputs("unit", "dominant", M, V, K, "edges", device)
        top = float(b.abs().max())
        for j, v in enumerate((0, 127, 128, vper - 1, vper, V - 1)):
            b[v] = top + 10.0 * (j + 1)
        self.hold(self.op(x, w, b, t), self.reference(x, w, b, t), "boundaries")

    def check_zero_bias(self, device):
        M, V, K = 300, 1000, self.k_big
        x, w, b, t = self.inputs("unit", "zero", M, V, K, "random64", device)
        got, plain = self.op(x, w, b, t), self.op(x, w, None, t)
        assert all(torch.equal(a, p) for a, p in zip(got[:3], plain[:3]))
        self.hold(got, self.reference(x, w, b, t), "zero bias")

    def check_no_valid_row(self, device):
        x, w, b, t = self.inputs("unit", "unit", 300, 1000, self.k_big, "none", device)
        loss, dx, dw, db = self.op(x, w, b, t)
        assert bool(torch.isnan(loss)) and not bool(dx.any()) and not bool(dw.any()) and not bool(db.any())

    def check_out_of_range(self, device):
        M, V, K = 300, 500, 64
        x, w, b, t = self.inputs("unit", "unit", M, V, K, "random64", device)
        valid = (t >= 0).nonzero().flatten()
        bad = t.clone()
        bad[valid[3]], bad[valid[-1]], bad[valid[40]] = V, 2 * V - 1, -7
        got = self.op(x, w, b, bad)
        R = self.reference(x, w, b, bad)
        assert bool(torch.isnan(got[0])) and R["poisoned"]
        for r in (valid[3], valid[-1], valid[40]):
            assert not bool(got[1][r].any())
        self.hold(got, R, "out of range")
        # the same dw and db as with those rows dropped, up to the mean's divisor (count includes them)
        dropped = t.clone()
        dropped[valid[3]] = dropped[valid[-1]] = dropped[valid[40]] = -1
        Rd = self.reference(x, w, b, dropped)
        scale = Rd["count"] / R["count"]
        assert ref.measures(got[2].double() / scale, Rd, "dw")[0] == 0
        assert ref.measures(got[3].double() / scale, Rd, "db")[0] == 0

    def check_bias_tail(self, device, V):
        """The bias as a view of a longer buffer whose tail holds NaN: nothing at or past b[V] is used; a misaligned
        view goes through the copy and gives the same numbers."""
        M, K = 129, self.k_small
        x, w, b, t = self.inputs("unit", "unit", M, V, K, "random64", device, seed=V)
        tight = self.op(x, w, b, t)
        full = torch.full((V + 256,), float("nan"), device=device)
        full[:V] = b
        assert full[:V].data_ptr() % 16 == 0
        shifted = torch.full((V + 256,), float("nan"), device=device)
        shifted[1:V + 1] = b
        assert shifted[1:V + 1].data_ptr() % 16 != 0
        for view in (full[:V], shifted[1:V + 1]):
            got = self.op(x, w, view, t)
            assert all(torch.equal(a, p) for a, p in zip(got, tight))
        assert bool(torch.isfinite(tight[0])) and bool(torch.isfinite(tight[3]).all())
        self.hold(tight, self.reference(x, w, b, t), f"bias tail V={V}")

    def raw(self, x, w, b, t, ignore_index, d_loss, dx, dw, db):
        from amk import lib as amk_lib

        L = amk_lib.load()
        P = lambda a: ctypes.c_void_p(a.data_ptr())
        M, K = x.shape
        V = w.shape[0]
        dev = x.device
        loss, lse = torch.empty((), device=dev), torch.empty(M, device=dev)
        rows, count = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        sfx = "bf16_" if self.bf16 else ""
        nf = getattr(L, f"amk_ce_head_{sfx}fwd_ws_bytes")(M, V, K)
        nb = getattr(L, f"amk_ce_head_{sfx}bwd_ws_bytes")(M, V, K)
        ws = torch.empty(max(nf, nb) // 4 + 4, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        amk_lib.check(getattr(L, f"amk_ce_head_bias_{sfx}fwd")(P(x), x.stride(0), P(w), w.stride(0), P(b), P(t), ignore_index, M, V,
                                                               K, P(loss), P(lse), P(rows), P(count), P(ws), nf, st), "fwd")
        d = torch.tensor([d_loss], device=dev)
        amk_lib.check(getattr(L, f"amk_ce_head_bias_{sfx}bwd")(P(x), x.stride(0), P(w), w.stride(0), P(b), P(t), ignore_index, M, V,
                                                               K, P(d), P(lse), P(rows), P(count), P(dx), dx.stride(0), P(dw),
                                                               dw.stride(0), P(db), P(ws), nb, st), "bwd")
        return loss

    def check_padded_layouts(self, device):
        """Padded ldx / ldw / lddx / lddw and a db buffer longer than V: nothing is written outside the views."""
        M, V, K = 129, 127, self.k_small
        x, w, b, t = self.inputs("unit", "unit", M, V, K, "random64", device)
        SENT = 12345.0
        xb, wb = torch.full((M, K + 8), SENT, device=device, dtype=x.dtype), torch.full((V, K + 8), SENT, device=device, dtype=w.dtype)
        xb[:, :K], wb[:, :K] = x, w
        dxb = torch.full((M, K + 16), SENT, device=device, dtype=x.dtype)
        dwb, dbb = torch.full((V, K + 8), SENT, device=device), torch.full((V + 129,), SENT, device=device)
        loss = self.raw(xb[:, :K], wb[:, :K], b, t, -1, D_LOSS, dxb[:, :K], dwb[:, :K], dbb)
        assert bool((dxb[:, K:] == SENT).all()) and bool((dwb[:, K:] == SENT).all()) and bool((dbb[V:] == SENT).all())
        got = (loss, dxb[:, :K], dwb[:, :K], dbb[:V])
        self.hold(got, self.reference(x, w, b, t), "padded")
        plain = self.op(x, w, b, t)
        assert all(torch.equal(a, g.contiguous()) for a, g in zip(plain, got))      # the layout changes no bit

    def check_run_to_run(self, device):
        x, w, b, t = self.inputs("peaked", "dominant", 300, 1000, self.k_big, "random64", device)
        a, c = self.op(x, w, b, t), self.op(x, w, b, t)
        assert all(torch.equal(p, q) for p, q in zip(a, c))

    def check_graph_capture(self, device):
        """Forward + backward captured once on a single stream; replays with targets of different valid counts equal the
        eager results bitwise, db included."""
        from amk import ops
        from amk.graphs import GraphedStep

        M, V, K = 300, 1000, 64
        x, w, b, t0 = self.inputs("unit", "unit", M, V, K, "random64", device)
        xg, wg, bg = x.clone().requires_grad_(), w.float().requires_grad_(), b.clone().requires_grad_()

        def fn(t):
            if self.bf16:
                with torch.autocast("cuda", dtype=BF16):
                    loss = ops.linear_cross_entropy(xg, wg, t, -1, bias=bg)
            else:
                loss = ops.linear_cross_entropy(xg, wg, t, -1, bias=bg)
            dx, dw, db = torch.autograd.grad(loss * D_LOSS, (xg, wg, bg))
            return loss, dx, dw, db

        step = GraphedStep(fn, [t0])
        for pattern in GRAPH_PATTERNS:
            t = ref.make_target(M, V, pattern, seed=3).to(device)
            out = [o.clone() for o in step.replay(t)]
            eager = self.op(x, w, b, t)
            for a, e in zip(out, eager):
                assert _same(a, e), pattern

    def check_reducer(self, device):
        from amk import ops
        from amk.dp import GradReducer

        M, V, K = 129, 256, 64
        x, w0, b0, t = self.inputs("unit", "unit", M, V, K, "random64", device)
        plain = self.op(x, w0, b0, t, d_loss=1.0)
        w, b = torch.nn.Parameter(w0.float().clone()), torch.nn.Parameter(b0.clone())
        red = GradReducer([w, b], direct_grads=True)
        if not red.direct_grads:
            pytest.skip("AMK_DIRECT_GRADS=0 in the environment")
        red.begin(sync=True)
        xg = x.clone().requires_grad_()
        if self.bf16:
            with torch.autocast("cuda", dtype=BF16):
                loss = ops.linear_cross_entropy(xg, w, t, -1, bias=b)
        else:
            loss = ops.linear_cross_entropy(xg, w, t, -1, bias=b)
        loss.backward()
        red.finish(detach_unused=False)
        assert sum(sum(bk.direct) for bk in red.buckets) == 2
        views = {v.data_ptr() for bk in red.buckets for v in bk.views}
        assert w.grad.data_ptr() in views and b.grad.data_ptr() in views
        assert torch.equal(w.grad, plain[2]) and torch.equal(b.grad, plain[3]) and torch.equal(xg.grad, plain[1])

    def check_library_path(self, device, family, bfam):
        """F.linear + F.cross_entropy under autocast round the bias and every logit to bf16 before the softmax: the two
        losses differ by at most 2^-8 mean_r max_v |z_rv| plus the fused head's own bound, and the fused loss is no
        further from fp64 than the library's."""
        x, w, b, t = self.inputs(family, bfam, 129, 1000, self.k_big, "random64", device)
        R = self.reference(x, w, b, t)
        fused = self.op(x, w, b, t)[0].double()
        with torch.autocast("cuda", dtype=BF16):
            lib = F.cross_entropy(F.linear(x, w.float(), b), t, ignore_index=-1).double()
        cap = 2.0 ** -8 * R["zmax"] + float(R["bound_loss"])
        ef, el = abs(float(fused - R["loss"])), abs(float(lib - R["loss"]))
        print(f"{family} x {bfam}: fused off by {ef:.3e}, library by {el:.3e}, hard bound {float(R['bound_loss']):.3e}, "
              f"|fused - lib| {abs(float(fused - lib)):.3e} of the cap {cap:.3e}")
        assert abs(float(fused - lib)) <= cap
        assert ef <= el

    def report(self, capsys, label):
        with capsys.disabled():
            print(f"\n{label} worst (hard ratio, q / (4 Q_EMU)):", {k: (round(a, 4), round(c, 4)) for k, (a, c) in self.worst.items()})
        assert not self.worst or set(self.worst) == set(ref.NAMES)
