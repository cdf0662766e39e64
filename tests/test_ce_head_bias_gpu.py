"""The loss head with a bias (csrc/ce_head.hip, ops.linear_cross_entropy(..., bias=b)) on the MI355X: loss, dx, dw and db
held element-wise to both tiers of tests/ce_head_bias_ref.py over tile edges, valid-row patterns and counts, slice and
tile boundaries and the input x bias families; a zero bias against the biasless op bit for bit; no valid row;
out-of-range targets; a bias with NaN behind b[V); padded layouts; reproducibility; graph capture; the gradient reducer's
direct writes.  The bodies are tests/ce_head_bias_checks.py."""
import pytest

import ce_head_bias_ref as ref
from ce_head_bias_checks import PATTERNS, VALID_COUNTS, Head

pytestmark = pytest.mark.gpu

H = Head(bf16=False)


@pytest.mark.parametrize("M,V,K,family,bfam", H.sweep_cases())
def test_tile_edges(device, M, V, K, family, bfam):
    H.check_case(device, M, V, K, family, bfam, what="edges")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_valid_patterns(device, pattern):
    H.check_case(device, 300, 1000, H.k_big, "unit", "unit", pattern=pattern, seed=0, what="pattern")


@pytest.mark.parametrize("n", VALID_COUNTS)
def test_valid_counts_around_the_db_and_dw_chains(device, n):
    H.check_valid_count(device, n)


def test_slice_and_tile_boundaries(device):
    H.check_boundaries(device)


@pytest.mark.parametrize("family", ["unit", "large", "climb"])
@pytest.mark.parametrize("bfam", ref.BIAS_FAMILIES)
def test_families(device, bfam, family):
    H.check_case(device, 129, 1000, H.k_big, family, bfam, seed=0, what="family")


def test_zero_bias_equals_the_biasless_op_bitwise(device):
    H.check_zero_bias(device)


def test_no_valid_row(device):
    H.check_no_valid_row(device)


def test_out_of_range_targets(device):
    H.check_out_of_range(device)


@pytest.mark.parametrize("V", [1, 127, 129])
def test_bias_is_not_read_past_V(device, V):
    H.check_bias_tail(device, V)


def test_padded_layouts(device):
    H.check_padded_layouts(device)


def test_run_to_run_bitwise(device):
    H.check_run_to_run(device)


def test_graph_capture_with_changing_valid_counts(device):
    H.check_graph_capture(device)


def test_reducer_receives_both_gradients_in_its_bucket(device):
    H.check_reducer(device)


def test_zz_report_worst_ratios(capsys):
    H.report(capsys, "ce_head_bias")
