"""The tuning switches that libamk.so reads once per process, at their non-default values: AMK_ATTN_DECODE_KEYS,
AMK_TN16_TK, AMK_TN16_WGS, AMK_X6_TN_TK, AMK_MOE_SHORT and AMK_MOE_WGRAD_SPLIT (README.md's switch table).  They cannot be
flipped inside pytest's process, so every (switch, value) gets ONE fresh child process with the variable in its environment;
the child (tests/env_switch_children.py) runs the family's existing check against its fp64 reference and bound and exits
non-zero with the message on a violation.  Children run one at a time, so at most one process holds the GPU beside pytest.

The parent asserts returncode == 0.  A child that ends by a signal, an abort or a time limit (124 / 134 / 137 / 139, a
negative status, or the safety-net timeout here) fails its test at once and every later test of this file fails without
starting a child: nothing more is started on a GPU that a child may have faulted."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
SWITCHES = ("AMK_ATTN_DECODE_KEYS", "AMK_TN16_TK", "AMK_TN16_WGS", "AMK_X6_TN_TK", "AMK_MOE_SHORT", "AMK_MOE_WGRAD_SPLIT")
# (switch, value, function of env_switch_children)
CHILDREN = [("AMK_ATTN_DECODE_KEYS", "32", "decode_keys"), ("AMK_ATTN_DECODE_KEYS", "128", "decode_keys"),
            ("AMK_TN16_TK", "256", "tn16_tk"), ("AMK_TN16_TK", "128", "tn16_tk"), ("AMK_TN16_WGS", "4", "tn16_wgs"),
            ("AMK_X6_TN_TK", "128", "x6_tn_tk"), ("AMK_X6_TN_TK", "256", "x6_tn_tk"),
            ("AMK_MOE_SHORT", "0", "moe_short"), ("AMK_MOE_WGRAD_SPLIT", "0", "moe_wgrad_split")]
FATAL = (124, 134, 137, 139)
TIMEOUT = 240          # a safety net, far above a child's few seconds
_stopped = []          # why no further child is started


def _child_code(fn):
    paths = [ROOT, os.path.join(ROOT, "attention-models_amd"), TESTS]       # as tests/conftest.py orders them
    return f"import sys; sys.path[:0] = {paths[::-1]!r}; import env_switch_children as c; c.main({fn!r})"


@pytest.mark.parametrize("switch,value,fn", CHILDREN, ids=[f"{s}={v}" for s, v, _ in CHILDREN])
def test_switch_value_in_a_fresh_process(device, switch, value, fn):
    assert not _stopped, f"not started: {_stopped[0]}"
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}       # one switch per child, the others at their defaults
    env[switch] = value
    try:
        res = subprocess.run([sys.executable, "-c", _child_code(fn)], env=env, timeout=TIMEOUT, cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"the child of {switch}={value} did not end within {TIMEOUT} s")
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"{_stopped[0]}\n{out[-3000:]}")
    print(res.stdout[-3000:])
    if res.returncode in FATAL or res.returncode < 0:
        _stopped.append(f"the child of {switch}={value} ended with status {res.returncode}")
        pytest.fail(f"{_stopped[0]}\n{res.stdout[-3000:]}")
    assert res.returncode == 0, f"{switch}={value}: status {res.returncode}\n{res.stdout[-3000:]}"
    assert f"{fn}: ok" in res.stdout.splitlines(), res.stdout[-3000:]      # (a profiler over the suite logs after it)
