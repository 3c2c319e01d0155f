"""The CPU restatement of the lexical transfer (tests/lexical_ref.py) against what the reference script itself produced
(tests/golden/lexical_*): bit for bit on every row with n <= 16 constituents — which is every row of the committed fixtures."""
import numpy as np
import pytest

from tests import lexical_cases as lc
from tests import lexical_ref


@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("name", lc.CASES)
def test_restatement_matches_reference(name, mode):
    case = lc.load(name)
    got, overlap, id_lists = lexical_ref.transfer(case["model"], case["vocab"], case["tokens"], case["S"], mode, case["unk_token_id"])
    print(f"{name} {mode}: overlap {overlap}, longest decomposition {max(map(len, id_lists))}")
    assert overlap == case["overlap"][mode]
    lc.assert_rows_match(got, lc.expected_cat(name, mode), id_lists, case["S"], f"{name} {mode}")


def test_fixture_rows_are_all_in_the_bit_exact_class():
    for name in lc.CASES:
        case = lc.load(name)
        for mode in ("fvt", "bfvt"):
            id_lists = lexical_ref.plan(lexical_ref.bare_model(case["model"]), case["vocab"], case["tokens"], len(case["S"]), mode)
            assert max(map(len, id_lists)) <= lc.MAX_EXACT_N


def test_row_count_differs_from_tokenizer_length_in_both_directions():
    assert lc.load("unigram")["n_source_rows"] < lc.load("unigram")["tokenizer_length"]
    assert lc.load("bpe")["n_source_rows"] > lc.load("bpe")["tokenizer_length"]


def test_random_fallback_matches_reference():
    case = lc.load("unigram")
    np.random.seed(case["random_seed"])
    got, overlap, id_lists = lexical_ref.transfer(case["model"], case["vocab"], case["tokens"], case["S"], "fvt", case["unk_token_id"], "random")
    assert overlap == case["overlap"]["fvt_random"]
    assert any(len(ids) == 0 for ids in id_lists)
    lc.assert_rows_match(got, lc.expected_cat("unigram", "fvt_random"), id_lists, case["S"], "unigram fvt random")


@pytest.mark.parametrize("block", [1, 3, 7, 128])
@pytest.mark.parametrize("cols", [6, 7])
def test_blocked_draws_equal_the_whole_draw(block, cols):
    """numpy's global generator hands out the same stream whether (rows, D) is drawn at once or in row blocks."""
    rows = 301
    loc, scale = np.linspace(-1, 1, cols), np.linspace(0.5, 2, cols)
    np.random.seed(7)
    whole = np.random.normal(loc=loc, scale=scale, size=(rows, cols))
    np.random.seed(7)
    parts = [np.random.normal(loc=loc, scale=scale, size=(min(rows, r0 + block) - r0, cols)) for r0 in range(0, rows, block)]
    assert np.array_equal(whole, np.concatenate(parts))


def test_mean_is_in_order_sum_then_one_division():
    rng = np.random.default_rng(0)
    S = rng.standard_normal((40, 9)).astype(np.float32)
    ids = [3, 17, 5, 5, 30]
    acc = S[3]
    for i in ids[1:]:
        acc = np.float32(acc + S[i])
    assert np.array_equal(lexical_ref.mean_rows(S, ids), acc / np.float32(5))
    assert np.array_equal(lexical_ref.mean_rows(S, [7]), S[7])
