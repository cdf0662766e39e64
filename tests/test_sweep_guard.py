"""The entry-point guard of the memory sweeps on planted inputs (tests/sweep_guard.py), and its launcher rule against
include/amk.h.  No GPU."""
import ctypes
import re

import sweep_guard

_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
SIG = {
    "amk_version": (_I, []),
    "amk_last_error": (ctypes.c_char_p, []),
    "amk_a_ws_floats": (_L, [_I, _I]),
    "amk_a_num_chunks": (_I, [_I]),
    "amk_a_fwd": (_I, [_P, _P, _I, _P]),
    "amk_a_bwd": (_I, [_P, _P, _I, ctypes.c_float, _P]),
    "amk_c_abi_only": (_I, [_P, _L, _P]),
}


def test_launchers_are_the_entry_points_that_take_a_stream():
    assert sweep_guard.launchers(SIG) == ["amk_a_bwd", "amk_a_fwd", "amk_c_abi_only"]


def test_the_launcher_rule_matches_the_header():
    """Exactly the functions of include/amk.h with a `stream` parameter."""
    from amk import lib

    text = re.sub(r"/\*.*?\*/", "", open(lib.HEADER_PATH).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(amk_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    assert set(decl) == set(lib.SIGNATURES)
    with_stream = sorted(n for n, args in decl.items() if re.search(r"\bstream\b", args))
    assert sweep_guard.launchers(lib.SIGNATURES) == with_stream and len(with_stream) > 90


def test_the_complete_set_passes():
    table = {"amk_c_abi_only": "no Python code of amk calls it (C ABI only)"}
    assert sweep_guard.verdict({"amk_a_fwd", "amk_a_bwd"}, SIG, table) == []
    assert sweep_guard.verdict({"amk_a_fwd", "amk_a_bwd", "amk_c_abi_only"}, SIG, {}) == []


def test_a_missing_launcher_fails_and_is_named():
    table = {"amk_c_abi_only": "C ABI only"}
    problems = sweep_guard.verdict({"amk_a_fwd"}, SIG, table)
    assert len(problems) == 1 and problems[0].startswith("amk_a_bwd: no case"), problems
    # a new entry point in SIGNATURES with no case: the same
    grown = dict(SIG, amk_new_fwd=(_I, [_P, _P]))
    problems = sweep_guard.verdict({"amk_a_fwd", "amk_a_bwd"}, grown, table)
    assert len(problems) == 1 and problems[0].startswith("amk_new_fwd: no case"), problems


def test_a_stale_exemption_fails():
    problems = sweep_guard.verdict({"amk_a_fwd", "amk_a_bwd", "amk_c_abi_only"}, SIG, {"amk_c_abi_only": "C ABI only"})
    assert len(problems) == 1 and "amk_c_abi_only" in problems[0] and "remove the exemption" in problems[0], problems


def test_an_unknown_name_fails():
    reached = {"amk_a_fwd", "amk_a_bwd", "amk_c_abi_only"}
    problems = sweep_guard.verdict(reached, SIG, {"amk_gone_fwd": "C ABI only"})
    assert len(problems) == 1 and "amk_gone_fwd" in problems[0] and "not in amk.lib.SIGNATURES" in problems[0], problems
    problems = sweep_guard.verdict(reached, SIG, {"amk_a_ws_floats": "a size query"})
    assert len(problems) == 1 and "not a launcher" in problems[0], problems
    problems = sweep_guard.verdict(reached | {"amk_typo"}, SIG, {})
    assert len(problems) == 1 and problems[0].startswith("amk_typo: recorded as reached"), problems


def test_an_exemption_needs_a_reason():
    problems = sweep_guard.verdict({"amk_a_fwd", "amk_a_bwd"}, SIG, {"amk_c_abi_only": " "})
    assert len(problems) == 1 and "without a reason" in problems[0], problems
