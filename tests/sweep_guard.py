"""The verdict of the memory sweeps' entry-point guard (tests/test_stale_memory_gpu.py, DESIGN.md "Stale memory"): which
launchers of the C ABI the sweep's cases reached, against the table of the ones it leaves out on purpose.

Pure functions on names: no GPU, no library.  tests/test_sweep_guard.py plants inputs on the CPU.
"""
import ctypes


def launchers(signatures):
    """The entry points of amk.lib.SIGNATURES that launch device work: they return a status and end in the stream.  Size
    queries (integer arguments only), amk_version, amk_arch and amk_last_error are not launchers.  tests/test_sweep_guard.py
    holds this rule to include/amk.h: exactly the functions with a `stream` parameter."""
    return sorted(n for n, (res, args) in signatures.items() if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p)


def verdict(reached, signatures, not_swept):
    """Problems, one line each; empty when the sweep is complete:

      * a launcher that no case reached and that NOT_SWEPT does not list -- a new entry point needs a case (or a reason);
      * a name of NOT_SWEPT that a case did reach -- the exemption is stale, remove it;
      * a name of NOT_SWEPT that SIGNATURES does not have, or that is no launcher -- the table rotted;
      * an exemption without a reason.
    """
    all_launchers = set(launchers(signatures))
    reached = set(reached)
    problems = []
    for name in sorted(all_launchers - reached - set(not_swept)):
        problems.append(f"{name}: no case of the sweep calls this launcher and NOT_SWEPT does not list it")
    for name in sorted(not_swept):
        if name not in signatures:
            problems.append(f"{name}: listed in NOT_SWEPT but not in amk.lib.SIGNATURES")
        elif name not in all_launchers:
            problems.append(f"{name}: listed in NOT_SWEPT but takes no stream: not a launcher")
        elif name in reached:
            problems.append(f"{name}: listed in NOT_SWEPT but a case reached it: remove the exemption")
        if not str(not_swept[name] or "").strip():
            problems.append(f"{name}: listed in NOT_SWEPT without a reason")
    for name in sorted(reached - all_launchers):
        problems.append(f"{name}: recorded as reached but no launcher of amk.lib.SIGNATURES")
    return problems
