"""The loss head with a bias under bf16 autocast (csrc/ce_head_bf16.hip, ops.linear_cross_entropy(..., bias=b) inside
torch.autocast("cuda", bfloat16)) on the MI355X: the checks of tests/test_ce_head_bias_gpu.py on the bf16 head's own K
list, plus the accuracy against the library path.  The bodies are tests/ce_head_bias_checks.py."""
import pytest

import ce_head_bias_ref as ref
from ce_head_bias_checks import PATTERNS, VALID_COUNTS, Head

pytestmark = pytest.mark.gpu

H = Head(bf16=True)


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


@pytest.mark.parametrize("family,bfam", [("unit", "unit"), ("large", "unit"), ("unit", "dominant"), ("peaked", "offset")])
def test_accuracy_against_the_library_path(device, family, bfam):
    H.check_library_path(device, family, bfam)


def test_zz_report_worst_ratios(capsys):
    H.report(capsys, "bf16_ce_head_bias")
