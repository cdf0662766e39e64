"""Fold the four rocprofv3 --pmc passes (tools/README.md) into profiles/rNN_pmc_kernels_bB.json.

    python tools/pmc_digest.py --sq A.csv --fetch B.csv --write C.csv --atomic D.csv --batch 32 --out profiles/r01_pmc_kernels_b32.json

Per kernel (amk_* kernels only; averages over the launches of a pass):
  hbm_bytes_per_launch = (2*FETCH_SIZE + WRITE_SIZE) * 1024   (FETCH_SIZE / WRITE_SIZE are KiB; gfx950 reports
                         half of a wide coalesced read stream, MI355X_MICROARCH.md)
  atomic bytes         = TCC_EA0_ATOMIC_sum * 64
  clock_GHz            = GRBM_GUI_ACTIVE / duration          (GRBM_GUI_ACTIVE sums the 8 XCDs: / 8)
  mfma_busy_frac       = SQ_VALU_MFMA_BUSY_CYCLES / (4 * 256 * cycles)   (per SIMD)
  valu_per_mfma        = (SQ_INSTS_VALU - SQ_INSTS_MFMA) / SQ_INSTS_MFMA   (SQ_INSTS_VALU counts the MFMAs too:
                         the fused backward's loop has 152 other VALU instructions per 192 MFMA in the ISA,
                         the counter ratio is 1.79)
"""
import argparse
import csv
import json
import re
from collections import defaultdict


def short(name):
    """Kernel name without namespace / arguments; the template variants bench.py reports separately keep
    their bench.py names: attn_fwd_kernel<.., .., true> = attn_fwd_keep_kernel (writes the scores),
    attn_bwd_fused_kernel<.., KEPT = true, ..> = attn_bwd_fused_kernel(kept scores); its head dims 32 / 128 keep the
    head dim in the name, and so does attn_bwd_fused_gen_kernel, their kernel in CSVs from before the merge."""
    m = re.search(r"(\w+_kernel)(<[^>]*>)?", name)
    if not m:
        return name
    base, targs = m.group(1), (m.group(2) or "").replace(" ", "")
    if base in ("attn_bwd_fused_kernel", "attn_bwd_fused_gen_kernel"):
        # <DH, NW, QS, KEPT, DQ, CAUSAL>; older CSVs: <NW, KEPT, DQ[, CAUSAL]> (head dim 64), gen <DH, NW, QS, KEPT, CAUSAL>
        t = targs.strip("<>").split(",")
        old64 = base == "attn_bwd_fused_kernel" and len(t) < 6
        dh, kept = ("64", t[1:2]) if old64 else (t[0], t[3:4])
        return "attn_bwd_fused_kernel" + ("" if dh == "64" else f"<{dh}>") + ("(kept scores)" if kept == ["true"] else "")
    if base == "attn_fwd_kernel" and targs.endswith(",true>"):
        return "attn_fwd_keep_kernel"
    if base == "attn_fwd_plain_kernel":   # the unmasked forward (round 4): <KEEP>
        return "attn_fwd_keep_kernel" if targs == "<true>" else "attn_fwd_kernel"
    return base


def fold(path, only=None):
    acc = defaultdict(lambda: defaultdict(list))
    dur = defaultdict(list)
    seen = set()
    for r in csv.DictReader(open(path)):
        if "amk_" not in r["Kernel_Name"]:
            continue
        if only and not any(o in r["Kernel_Name"] for o in only):
            continue
        k = short(r["Kernel_Name"])
        acc[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
        if r["Dispatch_Id"] not in seen:
            seen.add(r["Dispatch_Id"])
            dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {c: sum(v) / len(v) for c, v in cs.items()} for k, cs in acc.items()}, {k: sum(v) / len(v) for k, v in dur.items()}


def main():
    ap = argparse.ArgumentParser()
    for n in ("sq", "fetch", "write", "atomic", "out"):
        ap.add_argument("--" + n, required=True)
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--about", default="")
    a = ap.parse_args()
    sq, dur = fold(a.sq)
    out = {}
    for k, c in sq.items():
        d = dict(c)
        for path, key, name in ((a.fetch, "FETCH_SIZE", "FETCH_SIZE_KiB"), (a.write, "WRITE_SIZE", "WRITE_SIZE_KiB"),
                                (a.atomic, "TCC_EA0_ATOMIC_sum", "TCC_EA0_ATOMIC_sum")):
            vals, _ = fold(path)
            d[name] = vals.get(k, {}).get(key, 0.0)
        d["hbm_bytes_per_launch"] = (2 * d["FETCH_SIZE_KiB"] + d["WRITE_SIZE_KiB"]) * 1024
        d["avg_us_profiled"] = dur[k]
        cycles = d.get("GRBM_GUI_ACTIVE", 0.0) / 8
        if cycles:
            d["clock_GHz"] = cycles / (dur[k] * 1e3)
            if d.get("SQ_INSTS_MFMA"):
                d["mfma_busy_frac"] = d["SQ_VALU_MFMA_BUSY_CYCLES"] / (4 * 256 * cycles)
                d["valu_per_mfma"] = (d["SQ_INSTS_VALU"] - d["SQ_INSTS_MFMA"]) / d["SQ_INSTS_MFMA"]
        out[k] = d
    # (Round 2 first priced the kept-scores backward's score stream at its known size -- the x2 FETCH_SIZE correction
    # is calibrated for wide coalesced streams and the tiles are read 16 B per lane -- because the guide's formula gave
    # 1.38x the algorithmic bytes.  With the key blocks of a slice walking q / dO in step the formula itself gives
    # 1.13x, so the figure reported is the guide's formula for every kernel; the score stream's size is kept as a note.)
    kept, fkeep, ffwd = (out.get(k) for k in ("attn_bwd_fused_kernel(kept scores)", "attn_fwd_keep_kernel", "attn_fwd_kernel"))
    if kept and fkeep and ffwd:
        kept["score_stream_bytes"] = (fkeep["WRITE_SIZE_KiB"] - ffwd["WRITE_SIZE_KiB"]) * 1024
    about = a.about or ("rocprofv3 --pmc passes over `python tools/kbench.py --batch %d --iters 5` on one MI355X; separate passes "
                        "(SQ+GRBM set, FETCH_SIZE, WRITE_SIZE, TCC_EA0_ATOMIC_sum) as MI355X_MICROARCH.md prescribes; folded by "
                        "tools/pmc_digest.py" % a.batch)
    json.dump({"_about": about, "batch": a.batch, "kernels": out}, open(a.out, "w"), indent=1)
    for k, d in sorted(out.items()):
        print(f"{k:28s} {d['avg_us_profiled']:9.1f} us  hbm {d['hbm_bytes_per_launch']/1e6:8.1f} MB  clock {d.get('clock_GHz', 0):.2f} GHz"
              f"  mfma busy {d.get('mfma_busy_frac', 0):.2f}  valu/mfma {d.get('valu_per_mfma', 0):.2f}")


if __name__ == "__main__":
    main()
