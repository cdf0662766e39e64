#!/usr/bin/env python3
"""Launch coverage of the shipped kernels: which __global__ instances of libamk.so the GPU test suite launches.

Two inputs, no GPU code of its own:

  shipped    the `.amdhsa_kernel <symbol>` lines of attention-models_amd/csrc/build/*.s (`make -C attention-models_amd/csrc
             asm`; the cross-compiler alone makes them).  Nothing else of those files is read.
  launched   kernel names of rocprofv3 CSVs, one directory per test file or small group of test files:
                 rocprofv3 --kernel-trace --stats -M --output-format csv -d DIR/<label> -- python -m pytest <files> -m gpu -q
             Either CSV of a run serves: *_kernel_trace.csv (column Kernel_Name, one row per launch) or *_kernel_stats.csv
             (column Name, one row per kernel).  -M keeps the names mangled, so both sides are compared as the symbols the
             compiler emitted (the profiler's ".kd" suffix dropped); the demangler (c++filt or llvm-cxxfilt, if there is
             one) only makes the record readable.

    python tools/kernel_coverage.py --asm attention-models_amd/csrc/build --baseline DIR0 --traces DIR1 [--traces DIR2 ...]
        [--groups FILE] [--reasons FILE] [--header FILE] -o profiles/kernel_coverage.txt

  --baseline  runs of the suite before a change (its launched count is the record's "before"); --traces add to it ("after").
  --groups    lines `<label> <test file> ...`: the test files behind each run directory's label.
  --reasons   lines `<regex on the demangled name> <TAB> <reason>` for instances no run launches; the first match wins.  An
              instance without a reason is printed as UNACCOUNTED and the exit status is 1.
  --header    text put on top of the record (commit, exact commands).
"""
import argparse
import csv
import glob
import io
import os
import re
import shutil
import subprocess
import sys

_KERNEL_LINE = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$")


def parse_asm(text):
    """Kernel symbols of one device assembly file, in order: the operands of its .amdhsa_kernel lines, nothing else."""
    out = []
    for line in text.splitlines():
        if ".amdhsa_kernel" not in line:
            continue
        m = _KERNEL_LINE.match(line)
        if m:
            out.append(m.group(1))
    return out


def strip_kd(name):
    name = name.strip()
    return name[:-3] if name.endswith(".kd") else name


def parse_csv(text):
    """{kernel name: launches} of one rocprofv3 CSV: a kernel trace (Kernel_Name, one row per launch) or kernel statistics
    (Name, Calls).  Any other CSV gives {}."""
    rows = csv.reader(io.StringIO(text))
    try:
        head = next(rows)
    except StopIteration:
        return {}
    out = {}
    if "Kernel_Name" in head:
        col = head.index("Kernel_Name")
        for r in rows:
            if len(r) > col:
                n = strip_kd(r[col])
                out[n] = out.get(n, 0) + 1
    elif "Name" in head and "Calls" in head:
        col, calls = head.index("Name"), head.index("Calls")
        for r in rows:
            if len(r) > max(col, calls):
                n = strip_kd(r[col])
                out[n] = out.get(n, 0) + int(r[calls])
    return out


def shipped(asm_dir):
    """{device file: [symbols]} over asm_dir/*.s; files without a kernel are left out."""
    out = {}
    for path in sorted(glob.glob(os.path.join(asm_dir, "*.s"))):
        with open(path) as f:
            syms = parse_asm(f.read())
        if syms:
            out[os.path.splitext(os.path.basename(path))[0] + ".hip"] = syms
    return out


def launched(trace_dir):
    """{label: {kernel name: launches}} over trace_dir/<label>/**/*.csv."""
    out = {}
    for label in sorted(os.listdir(trace_dir)):
        sub = os.path.join(trace_dir, label)
        if not os.path.isdir(sub):
            continue
        names = {}
        for path in sorted(glob.glob(os.path.join(sub, "**", "*.csv"), recursive=True)):
            with open(path, newline="") as f:
                # statistics and trace of one run would count a launch twice: the counts are informative only
                for n, c in parse_csv(f.read()).items():
                    names[n] = max(names.get(n, 0), c)
        out[label] = names
    return out


def demangle(symbols):
    """{symbol: readable name} through c++filt / llvm-cxxfilt; the symbols themselves where neither is there."""
    symbols = list(symbols)
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not symbols:
        return {s: s for s in symbols}, None
    res = subprocess.run([tool], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True)
    lines = res.stdout.splitlines()
    if len(lines) != len(symbols):
        return {s: s for s in symbols}, None
    return {s: re.sub(r"^void ", "", d) for s, d in zip(symbols, lines)}, os.path.basename(tool)


def read_groups(path):
    out = {}
    if path:
        with open(path) as f:
            for line in f:
                parts = line.split()
                if parts and not parts[0].startswith("#"):
                    out[parts[0]] = parts[1:]
    return out


def read_reasons(path):
    out = []
    if path:
        with open(path) as f:
            for line in f:
                if line.strip() and not line.startswith("#"):
                    rx, _, reason = line.rstrip("\n").partition("\t")
                    out.append((re.compile(rx.strip()), reason.strip()))
    return out


def coverage(ship, runs):
    """{symbol: first label that launches it} for the shipped symbols, labels in sorted order."""
    where = {}
    all_syms = {s for syms in ship.values() for s in syms}
    for label in sorted(runs):
        for n in runs[label]:
            if n in all_syms and n not in where:
                where[n] = label
    return where


def report(ship, before, after, groups, reasons, header=""):
    """(text of the record, number of unaccounted instances)."""
    all_syms = [s for syms in ship.values() for s in syms]
    names, tool = demangle(all_syms)
    w_before = coverage(ship, before)
    merged = {("before:" + k): v for k, v in before.items()}
    merged.update({("now:" + k): v for k, v in after.items()})
    w_after = coverage(ship, merged)
    out = []
    if header:
        out += [header.rstrip("\n"), ""]
    out.append(f"shipped instances: {len(all_syms)} in {len(ship)} device files")
    out.append(f"launched by the suite before: {len(w_before)}    after: {len(w_after)}    not launched: {len(all_syms) - len(w_after)}")
    out.append("names compared mangled (rocprofv3 -M against the .amdhsa_kernel symbols); shown through "
               + (tool or "no demangler: mangled"))
    out.append("")
    out.append(f"{'device file':28s} {'shipped':>7s} {'before':>7s} {'after':>7s}")
    for f, syms in ship.items():
        out.append(f"{f:28s} {len(syms):7d} {sum(s in w_before for s in syms):7d} {sum(s in w_after for s in syms):7d}")
    unaccounted = 0
    out += ["", "== not launched =="]
    for f, syms in ship.items():
        miss = [s for s in syms if s not in w_after]
        if not miss:
            continue
        out.append(f"{f}:")
        for s in miss:
            why = next((r for rx, r in reasons if rx.search(names[s])), None)
            if why is None:
                unaccounted += 1
                why = "UNACCOUNTED"
            out.append(f"  {names[s]}\n      {why}")
    out += ["", "== launched: instance <- one run that launches it (new: only the runs after the change do) =="]

    def files(label):
        tag, _, key = label.partition(":")
        return ("new: " if tag == "now" else "") + (" ".join(groups.get(key, [])) or key)

    for f, syms in ship.items():
        out.append(f"{f}:")
        for s in syms:
            if s in w_after:
                out.append(f"  {names[s]}\n      <- {files(w_after[s])}")
    return "\n".join(out) + "\n", unaccounted


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", required=True)
    ap.add_argument("--baseline", required=True)
    ap.add_argument("--traces", action="append", default=[])
    ap.add_argument("--groups")
    ap.add_argument("--reasons")
    ap.add_argument("--header")
    ap.add_argument("-o", "--output")
    a = ap.parse_args(argv)
    ship = shipped(a.asm)
    if not ship:
        sys.exit(f"no .amdhsa_kernel line under {a.asm}: run `make -C attention-models_amd/csrc asm` first")
    after = {}
    for d in a.traces:
        for label, names in launched(d).items():
            after.setdefault(label, {}).update(names)
    header = open(a.header).read() if a.header else ""
    text, unaccounted = report(ship, launched(a.baseline), after, read_groups(a.groups), read_reasons(a.reasons), header)
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    if unaccounted:
        print(f"{unaccounted} instances neither launched nor given a reason", file=sys.stderr)
    return 1 if unaccounted else 0


if __name__ == "__main__":
    sys.exit(main())
