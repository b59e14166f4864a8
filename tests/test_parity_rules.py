"""The rules of tests/parity_rules.py, tested themselves on a hand-made [3][37] logits block (no GPU): what they accept and, above all, what
they reject.  The expected log-probabilities are worked out here with math.fsum / math.log, not with the module's own arithmetic."""
import math

import numpy as np
import pytest

from parity_rules import assert_bit_equal, assert_within_one_ulp, check_scores, ref_argmax

N, V = 3, 37
TOKS = np.array([4, 11, 30], np.uint32)                  # the targets: token 11 after row 0, token 30 after row 1


def _rows():
    j = np.arange(V)
    rows = np.stack([((j * 7 + r * 13) % V).astype(np.float32) * np.float32(0.37) - np.float32(5 - r) for r in range(N)])
    rows[1, 5] = rows[1, 6] = rows[1].max() + np.float32(1.25)            # an exact tie at the maximum: index 5 wins
    rows[2, 36] = np.float32(40.0)                                        # one logit far above the rest
    return rows


def _exact(rows, toks):
    """the float64 answer: log softmax(row t)[toks[t + 1]] with m = the row's f32 maximum"""
    out = []
    for t in range(len(toks) - 1):
        x = [float(v) for v in rows[t]]
        m = max(x)
        out.append(x[int(toks[t + 1])] - m - math.log(math.fsum(math.exp(v - m) for v in x)))
    return np.array(out, np.float64)


def _good():
    rows = _rows()
    want = _exact(rows, TOKS)
    am = np.array([int(np.argmax(r)) for r in rows], np.uint32)           # numpy's argmax: the first maximum as well
    return rows, want, (want.astype(np.float32), am, float(want.sum()))


def _moved(x, ulps, away_from_zero):
    to = np.float32(-np.inf if (x < 0) == away_from_zero else np.inf)
    for _ in range(ulps):
        x = np.nextafter(np.float32(x), to)
    return x


def test_the_hand_made_block_is_what_the_cases_need():
    rows, want, (lp, am, s) = _good()
    assert rows.shape == (N, V) and rows.dtype == np.float32
    assert am.tolist() == [int(np.flatnonzero(r == r.max())[0]) for r in rows] and am[1] == 5 and rows[1, 5] == rows[1, 6] == rows[1].max()
    assert (want < -1.0).all()                                            # well away from zero: an ulp there is an ulp of the value's own binade
    for v in lp:                                                          # ... and two ulps either way stay inside that binade
        assert math.frexp(float(_moved(v, 2, True)))[1] == math.frexp(float(_moved(v, 2, False)))[1] == math.frexp(float(v))[1]


def test_check_scores_accepts_the_float64_answer_rounded_to_f32():
    rows, want, got = _good()
    check_scores(got, rows, TOKS, "exact")
    assert [ref_argmax(r) for r in rows] == got[1].tolist()


@pytest.mark.parametrize("away", [True, False])
@pytest.mark.parametrize("t", [0, 1])
def test_check_scores_allows_one_ulp_and_rejects_two(t, away):
    rows, want, (lp, am, s) = _good()
    one = lp.copy(); one[t] = _moved(lp[t], 1, away)
    check_scores((one, am, s), rows, TOKS, "one ulp")
    two = lp.copy(); two[t] = _moved(lp[t], 2, away)
    with pytest.raises(AssertionError, match="more than 1 ulp"):
        check_scores((two, am, s), rows, TOKS, "two ulps")


def test_check_scores_rejects_the_second_index_of_a_tie():
    rows, want, (lp, am, s) = _good()
    bad = am.copy(); bad[1] = 6
    with pytest.raises(AssertionError, match="argmax"):
        check_scores((lp, bad, s), rows, TOKS, "tie")


@pytest.mark.parametrize("rel", [1e-6, -1e-6])
def test_check_scores_rejects_a_sum_off_by_a_millionth(rel):
    rows, want, (lp, am, s) = _good()
    check_scores((lp, am, s * (1 + 5e-10)), rows, TOKS, "inside 1e-9")
    with pytest.raises(AssertionError, match="sum"):
        check_scores((lp, am, s * (1 + rel)), rows, TOKS, "sum")


def test_check_scores_rejects_wrong_shapes():
    rows, want, (lp, am, s) = _good()
    for bad in ((np.append(lp, lp[-1]), am, s), (lp, am[:-1], s), (lp[:-1], am, s), (lp.reshape(1, -1), am, s)):
        with pytest.raises(AssertionError):
            check_scores(bad, rows, TOKS, "shape")


def test_check_scores_with_one_token():
    rows = _rows()[:1]
    am = np.array([ref_argmax(rows[0])], np.uint32)
    none = np.zeros(0, np.float32)
    check_scores((none, am, 0.0), rows, TOKS[:1], "n == 1")
    with pytest.raises(AssertionError):
        check_scores((none, am, 1e-300), rows, TOKS[:1], "n == 1: a sum that is not 0.0")
    with pytest.raises(AssertionError, match="argmax"):
        check_scores((none, am + 1, 0.0), rows, TOKS[:1], "n == 1: argmax")
    with pytest.raises(AssertionError):
        check_scores((np.zeros(1, np.float32), am, 0.0), rows, TOKS[:1], "n == 1: a log-probability too many")


def test_one_ulp_rule_takes_any_shape_and_only_f32():
    want = np.array([[-1.5, -2.25, -300.0], [-0.75, -17.0, -1e-3]], np.float64)
    got = want.astype(np.float32)
    assert_within_one_ulp(got, want, "2-d")
    got[1, 2] = _moved(got[1, 2], 2, True)
    with pytest.raises(AssertionError, match="more than 1 ulp"):
        assert_within_one_ulp(got, want, "2-d")
    with pytest.raises(AssertionError):
        assert_within_one_ulp(want, want, "float64 results")
    with pytest.raises(AssertionError):
        assert_within_one_ulp(want.astype(np.float32).ravel(), want, "shape")


def test_assert_bit_equal_tells_signed_zeros_and_nan_payloads_apart():
    z = np.array([0.0, 1.0], np.float32)
    assert_bit_equal(z, z.copy())
    with pytest.raises(AssertionError, match="1/2 elements differ"):
        assert_bit_equal(z, np.array([-0.0, 1.0], np.float32), "-0.0")
    nan = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000], np.uint32).view(np.float32)
    assert_bit_equal(nan, nan.copy(), "the same NaNs")
    for i, j in ((0, 1), (0, 2)):
        with pytest.raises(AssertionError, match="elements differ"):
            assert_bit_equal(nan[[i]], nan[[j]], "NaN payloads")
    with pytest.raises(AssertionError, match="shapes"):
        assert_bit_equal(z, z[:1], "shape")
    with pytest.raises(AssertionError, match="elements differ"):
        assert_bit_equal(np.array([1, 2], np.uint32), np.array([1, 3], np.uint32), "integers")
