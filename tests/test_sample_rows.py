"""lmrs_op_sample_rows (the kernels of lmrs_batch_forward_sample: Sampler::sample for up to 16 logit rows at once, everything on the device) against
the oracle's Sampler on the same logits: the probabilities of every row bit for bit, sample_mult's token, and a top-p row's candidates in index order.
No tolerances.  A NaN equals a NaN whatever its sign and payload: 0xFFC00000 is what the host's SSE unit makes of inf - inf, 0x7FC00000 the GPU's."""
import numpy as np
import pytest

import oracle_lib as O
from parity_rules import bits

gpu = pytest.mark.gpu

# the block sizes of launch_sample_rows' kernels (lmrs_kernels.hip / lmrs_kernels.h), both sides of each in the size list:
GROUP = 32        # kRowsUnroll x 4: the terms of one register set of the chain lane (and the cdf's test interval)
BLOCK = 256       # kBlock: the indices one step of a workgroup covers (division, candidate filter)
CHUNK = 2048      # kRowsChunk: the floats of a row staged through one LDS buffer
GRID = 64         # kSampleRowsGrid: workgroups per row; from GRID * BLOCK entries on a workgroup's span of indices is more than one block
SIZES = [1, 2, 63, 64, 65, 1000, 4096, 4102, 40000, 128256,
         GROUP - 1, GROUP, GROUP + 1, BLOCK - 1, BLOCK, BLOCK + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1,
         GRID * BLOCK - 1, GRID * BLOCK, GRID * BLOCK + 1]

# (temperature, top_p) by row: sample_mult (top_p >= 1, <= 0), top-p, one argmax row (never touched)
PARAMS = [(0.8, 1.0), (0.7, 0.9), (1.5, 0.0), (0.05, 0.5), (0.0, 0.9), (3.0, 0.999), (1.0, 0.3), (0.02, 0.9), (0.8, 2.0), (1.3, 0.99),
          (0.5, -1.0), (0.7, 0.9), (2.0, 1.0), (0.3, 0.7), (1.0, 0.95), (0.9, 0.5)]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def assert_same(got, want, what):
    """bit for bit, a NaN matching any NaN"""
    got = np.asarray(got, np.float32); want = np.asarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} vs {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaNs at {np.flatnonzero(gn != wn)[:5]}"
    ne = np.flatnonzero((bits(got) != bits(want)) & ~gn)
    assert ne.size == 0, f"{what}: {ne.size}/{got.size} differ, first at {ne[:5]}: {got.ravel()[ne[:5]]} vs {want.ravel()[ne[:5]]}"


def oracle_row(logits, temperature, top_p, seed):
    """Sampler::sample of the oracle on a copy -> (token or None where the reference panics, what the logits became)"""
    lg = np.ascontiguousarray(logits, np.float32).copy()
    try:
        tok = O.Sampler(lg.size, temperature, top_p, seed).sample(lg)
    except RuntimeError:
        tok = None
    return tok, lg


def is_topp(top_p):
    return not (top_p <= 0.0 or top_p >= 1.0)


def cutoff_of(top_p, n):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.float32(1.0) - np.float32(top_p)) / np.float32(n - 1)          # sampler.rs:71, in f32


def check_rows(L, logits, params, seeds, what):
    """op_sample_rows on logits [R, n] with params[r] and the random number of seeds[r], every row against the oracle's Sampler"""
    R, n = logits.shape
    t, p = [a for a, _ in params], [b for _, b in params]
    rnd = [O.random_f32(s) for s in seeds]
    probs, tok, n0, pairs = L.op_sample_rows(logits, t, p, rnd)
    for r in range(R):
        w = f"{what}: row {r} {params[r]}"
        want_tok, want = oracle_row(logits[r], t[r], p[r], seeds[r])
        assert_same(probs[r], want, w + " probabilities")
        if t[r] == 0.0:
            continue
        if not is_topp(p[r]):
            assert int(tok[r]) == want_tok, w + f": token {tok[r]} vs {want_tok}"
            continue
        keep = np.flatnonzero(want >= cutoff_of(p[r], n))                            # (a NaN is never a candidate)
        assert int(n0[r]) == keep.size, w + f": n0 {n0[r]} vs {keep.size}"
        assert np.array_equal(pairs[r][1], keep.astype(np.uint32)), w + ": candidate indices (ascending)"
        assert_same(pairs[r][0], want[keep], w + ": candidate probabilities")
        if want_tok is None:
            assert keep.size == 0, w
            continue
        # the pairs are what lmrs_sampler_topp_pairs takes: the host half gives the oracle's token
        assert L.Sampler(n, t[r], p[r], seeds[r]).topp_pairs(*pairs[r]) == want_tok, w + ": token through topp_pairs"


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_rows_against_the_oracle_sampler(L, n):
    rng = np.random.default_rng(1000 + n)
    for R in (1, 3, 16):
        logits = (rng.standard_normal((R, n)) * 3.0).astype(np.float32)
        first = {1: 1, 3: 0, 16: 0}[R]                                               # (the one-row case: a top-p row)
        params = [PARAMS[(first + r) % len(PARAMS)] for r in range(R)]
        check_rows(L, logits, params, [500 + 7 * r + n for r in range(R)], f"n {n} rows {R}")


def seq_cdf(p):
    """the running cdf as sample_mult forms it: one f32 chain in index order"""
    out = np.empty(p.size, np.float32)
    acc = np.float32(0.0)
    for i, v in enumerate(p):
        acc = np.float32(acc + v)
        out[i] = acc
    return out


@gpu
def test_sample_mult_around_every_boundary(L):
    """one row, many random numbers: 0, the first three cdf values with the value below and above each, the same around every block boundary of the
    kernels, the last cdf value and the largest random number there is"""
    n, temp = 2 * CHUNK + 100, 0.8
    logits = (np.random.default_rng(7).standard_normal(n) * 0.5).astype(np.float32)
    _, want = oracle_row(logits, temp, 1.0, 1)
    cdf = seq_cdf(want)
    edges = [0, 1, 2] + [b + d for b in (GROUP, 2 * GROUP, BLOCK, CHUNK, CHUNK + GROUP, 2 * CHUNK) for d in (-1, 0)] + [n - 2, n - 1]
    rnds = [np.float32(0.0), np.float32(0.99999994)]
    for i in edges:
        rnds += [np.nextafter(cdf[i], np.float32(0.0)), cdf[i], np.nextafter(cdf[i], np.float32(2.0))]
    rnds = np.array(rnds, np.float32)
    for r0 in range(0, rnds.size, 16):
        rr = rnds[r0: r0 + 16]
        probs, tok, n0 = L.op_sample_rows(np.tile(logits, (rr.size, 1)), [temp] * rr.size, [1.0] * rr.size, rr, pairs=False)
        for k, rnd in enumerate(rr):
            hit = np.flatnonzero(rnd < cdf)
            assert int(tok[k]) == (int(hit[0]) if hit.size else n - 1), f"rnd {rnd!r}: token {tok[k]}"
            assert_same(probs[k], want, f"rnd {rnd!r}: probabilities")


@gpu
def test_top_p_one_candidate_and_all_candidates(L):
    n = CHUNK + 77
    one = np.zeros(n, np.float32); one[1234] = 50.0                                  # everything else is ~2e-22: below the cutoff
    flat = np.full(n, 0.25, np.float32)                                              # p = 1 / n each, above 0.001 / (n - 1)
    logits = np.stack([one, flat, one])
    probs, tok, n0, pairs = L.op_sample_rows(logits, [1.0, 1.0, 1.0], [0.5, 0.999, 0.5], [0.3, 0.3, 0.3])
    assert n0.tolist() == [1, n, 1] and pairs[0][1].tolist() == [1234] and np.array_equal(pairs[1][1], np.arange(n, dtype=np.uint32))
    check_rows(L, logits, [(1.0, 0.5), (1.0, 0.999), (1.0, 0.5)], [3, 4, 5], "one / all candidates")


@gpu
@pytest.mark.parametrize("case", ["nan at 0", "nan elsewhere", "+inf", "equal values", "-inf elsewhere"])
def test_nan_and_infinity(L, case):
    n = CHUNK + 33
    rng = np.random.default_rng(11)
    base = rng.standard_normal(n).astype(np.float32)
    if case == "nan at 0":
        base[0] = np.nan
    elif case == "nan elsewhere":
        base[CHUNK + 5] = np.nan
    elif case == "+inf":
        base[17] = np.inf
    elif case == "-inf elsewhere":
        base[300] = -np.inf
    else:
        base[:] = 1.5
    logits = np.stack([base, base, base, base])
    check_rows(L, logits, [(0.8, 1.0), (0.7, 0.9), (1.5, 0.0), (0.0, 0.9)], [21, 22, 23, 24], case)


@gpu
def test_bad_arguments_are_refused_before_the_device_is_touched(L):
    x = np.zeros((1, 8), np.float32)
    one = [1.0]
    for rows, msg in ((np.zeros((17, 8), np.float32), "n_rows = 17"), (np.zeros((0, 8), np.float32), "n_rows = 0"), (np.zeros((1, 0), np.float32), "1 <= n")):
        r = rows.shape[0]
        with pytest.raises(L.LmrsError, match=msg):
            L.op_sample_rows(rows, one * r, one * r, one * r)
    lib = L.lib()
    tok = np.zeros(1, np.uint32)
    assert lib.lmrs_op_sample_rows(0, None, 1, 8, x.ctypes.data, x.ctypes.data, x.ctypes.data, tok.ctypes.data, tok.ctypes.data, None) != 0
    assert "NULL" in lib.lmrs_last_error().decode()
