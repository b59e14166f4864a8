"""The rules the parity tests judge by, one copy each: bit equality, the reference's argmax, the oracle's SEQUENTIAL forward as the reference of a
token run (one call per token, transformer.rs:316-384), log-probabilities within one f32 ulp of a float64 log-softmax, and the K/V rows and the
forward a call leaves behind.  tests/test_parity_rules.py tests the rules themselves."""
import numpy as np

import oracle_lib as O


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bit_equal(a, b, what=""):
    """equal shapes and, for float32, equal bit patterns (-0.0 is not +0.0, a NaN equals only itself); other types by value"""
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} vs {b.shape}"
    ne = np.flatnonzero(bits(a) != bits(b)) if a.dtype == np.float32 else np.flatnonzero(a != b)
    assert ne.size == 0, f"{what}: {ne.size}/{a.size} elements differ, first at {ne[:5]}: {a.ravel()[ne[:5]]} vs {b.ravel()[ne[:5]]}"


def ref_argmax(row):
    """sample_argmax (sampler.rs:29-41): the first maximum wins"""
    row = np.ascontiguousarray(row)
    return int(O.lib().lmrs_ref_argmax(row.ctypes.data, row.size))


def oracle_rows(orc, toks, start):
    return np.stack([orc.forward(int(t), start + i).copy() for i, t in enumerate(toks)])


def log_softmax64(rows):
    """(x, m, lse) of logits rows [n, V]: x in float64, m = the f32 maximum of a row, lse = log of the sum over every logit of exp(x - m)"""
    x = rows.astype(np.float64)
    m = rows.max(axis=1).astype(np.float64)
    return x, m, np.log(np.exp(x - m[:, None]).sum(axis=1))


def assert_within_one_ulp(got, want64, what):
    """f32 values `got` against float64 `want64` of the same shape (any): at most one f32 ulp from want64 rounded to f32"""
    got = np.asarray(got); want64 = np.asarray(want64, np.float64)
    assert got.dtype == np.float32 and got.shape == want64.shape, f"{what}: {got.dtype} {got.shape} vs {want64.shape}"
    w32 = want64.astype(np.float32)
    assert np.all(np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64)), \
        f"{what}: more than 1 ulp from float64, worst {np.max(np.abs(got - w32))}"


def check_scores(got, rows, toks, what):
    """(logprobs, argmax, sum) of the library against the oracle's logits: the argmax of lmrs_ref_argmax, log-probabilities within one
    f32 ulp of a float64 log-softmax (m = the f32 maximum, the sum over every logit), their double sum to 1e-9 relative."""
    lp, am, s = got
    n = len(toks)
    assert lp.shape == (n - 1,) and am.shape == (n,)
    assert am.tolist() == [ref_argmax(r) for r in rows], f"{what}: argmax"
    x, m, lse = log_softmax64(rows)
    want = x[np.arange(n - 1), np.asarray(toks[1:], np.int64)] - m[:-1] - lse[:-1]
    assert_within_one_ulp(lp, want, f"{what}: log-probabilities")
    if n > 1:
        assert abs(s - want.sum()) <= 1e-9 * abs(want.sum()), f"{what}: sum {s} vs {want.sum()}"
    else:
        assert s == 0.0


def check_kv_rows(m, orc, positions, what):
    """K and V rows of the first and last layer at `positions`, against the oracle's"""
    nl = orc.args.n_layers
    for layer in (0, nl - 1):
        for p in positions:
            for which in (0, 1):
                assert_bit_equal(m.kv_row(which, layer, p), orc.kv_row(which, layer, p), f"{what}: {'kv'[which]} row layer {layer} pos {p}")


def run_positions(start, n):
    """the first, middle and last position of a run of n tokens from `start`"""
    return sorted({start, start + n // 2, start + n - 1})


def check_after(m, orc, n, start, what):
    """K/V rows of the first and last layer at three positions of the run, and one forward at start + n, against the oracle's."""
    check_kv_rows(m, orc, run_positions(start, n), what)
    if start + n < orc.args.seq_len:
        t = 7 % orc.args.vocab_size
        assert_bit_equal(m.forward(t, start + n), orc.forward(t, start + n), f"{what}: forward at {start + n} after the call")
