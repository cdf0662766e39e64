"""Fold a rocprofv3 kernel trace of bench.py into one step's table: device time and launches per kernel, for the last full
step of the trace (the kernels between the optimizer launches two groups back and the last optimizer group: discriminator
phase + generator phase), and the sums of the families the Linear layers run on.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 5 --warmup 3 --no-variants ...
    python tools/fold_step_trace.py DIR [--top 30]
"""
import argparse
import csv
import glob
import os
import re
import sys

FAMILIES = [
    ("x6 Linear GEMMs (gemm_x6_nt_kernel)", r"gemm_x6_nt_kernel"),
    ("x6 Linear GEMMs, K <= 256 (gemm_x6_short_k_kernel)", r"gemm_x6_short_k_kernel"),
    ("plane split (split_table_kernel)", r"split_table_kernel"),
    ("per-call split (split_planes_kernel)", r"split_planes_kernel"),
    ("f32 NT (gemm_nt_dkernel / gemm_nt_kernel)", r"amk_dense.*gemm_nt_"),
    ("f32 NN (gemm_nn_kernel)", r"amk_dense.*gemm_nn_"),
    ("f32 TN + reduce (weight gradients)", r"amk_dense.*(gemm_tn_|tn_reduce)"),
    ("x6 TN + reduce (weight gradients)", r"gemm_x6_tn_kernel|x6_tn_reduce_kernel"),
    ("library GEMMs (Cijk_*)", r"^Cijk_"),
    ("attention (attn_*)", r"attn_"),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--top", type=int, default=30)
    a = ap.parse_args()
    files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {a.dir}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    opt = [i for i, r in enumerate(rows) if "adam_flat" in r[2]]
    groups = []
    for i in opt:   # optimizer launches less than 16 kernels apart are one optimizer step (one launch per bucket)
        if groups and i - groups[-1][-1] < 16:
            groups[-1].append(i)
        else:
            groups.append([i])
    if len(groups) < 3:
        sys.exit("fewer than three optimizer groups in the trace")
    lo, hi = groups[-3][-1] + 1, groups[-1][-1] + 1
    step = rows[lo:hi]
    per = {}
    for s, e, n in step:
        t = per.setdefault(n, [0, 0])
        t[0] += 1
        t[1] += e - s
    busy = sum(t[1] for t in per.values())
    print(f"last full step: {len(step)} kernels, busy {busy / 1e6:.2f} ms, span {(step[-1][1] - step[0][0]) / 1e6:.2f} ms")
    for title, pat in FAMILIES:
        sel = [(n, t) for n, t in per.items() if re.search(pat, n)]
        print(f"  {title:46s} {sum(t[0] for _, t in sel):5d} launches {sum(t[1] for _, t in sel) / 1e6:8.3f} ms")
    print(f"kernels by device time (top {a.top}):")
    for n, t in sorted(per.items(), key=lambda kv: -kv[1][1])[:a.top]:
        print(f"  {n[:96]:96s} {t[0]:5d} {t[1] / 1e6:8.3f} ms")
