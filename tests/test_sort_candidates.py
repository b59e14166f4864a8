"""lmrs_op_sort_candidates (include/lmrs_hip.h): the sort of lmrs_batch_forward_runs_sample's flat top-p rows, every row of a call through one sequence
of launches.  The reference is numpy's STABLE argsort of the negated probabilities over each row's first n0 entries - what the stable sort of
sampler.rs:81 makes of candidates that stand in index order.  Every comparison is bit for bit; nothing outside a row's first n0 entries may move."""
import ctypes

import numpy as np
import pytest

gpu = pytest.mark.gpu

# one LDS block of 8192 keys and both sides of it, the first global step (16384), and two, three and four global levels (32768, 65536, 131072 keys)
LDS = [1, 5, 8191, 8192, 8193, 16384, 16385, 20000, 40000, 70000]
ROWS = [1, 3, 16, 64]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def candidates(L, rng, n_rows, ld, levels=0):
    """n_rows x ld candidates in ascending index order; levels: quantise the probabilities to that many distinct values (ties by the thousand)"""
    x = np.zeros((n_rows, ld), L.PAIR)
    p = rng.random((n_rows, ld), np.float32)
    if levels:
        p = (np.floor(p * levels) / np.float32(levels * 4)).astype(np.float32)
    p[:, ::7] = p[:, :1]                                                               # equal probabilities in every row, whatever the size
    x["prob"] = p
    x["index"] = np.sort(rng.choice(1 << 20, size=ld, replace=False)).astype(np.uint32)[None, :] + np.arange(n_rows, dtype=np.uint32)[:, None]
    return x


def counts(rng, n_rows, ld):
    """0, 1, ld and values in between, cycling, so that the rows of one call differ"""
    base = [ld, 0, 1, ld // 2, ld - 1, ld // 3 + 1]
    return np.array([min(ld, base[r % 6] if r < 6 else int(rng.integers(0, ld + 1))) for r in range(n_rows)], np.uint32)


def reference(x, n0):
    want = x.copy()
    for r in range(x.shape[0]):
        order = np.argsort(-x["prob"][r, : n0[r]], kind="stable")
        want[r, : n0[r]] = x[r, : n0[r]][order]
    return want


def assert_same(got, want, what):
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    assert bad.size == 0, f"{what}: rows {bad.tolist()[:8]} differ from the stable sort"


@gpu
@pytest.mark.parametrize("ld", LDS)
def test_rows_of_one_call_against_the_stable_sort(L, ld):
    rng = np.random.default_rng(9000 + ld)
    pool = candidates(L, rng, 64, ld)
    for n_rows in ROWS:
        x = pool[:n_rows]
        n0 = counts(rng, n_rows, ld)
        assert_same(L.op_sort_candidates(x, n0), reference(x, n0), f"ld {ld} rows {n_rows} n0 {n0.tolist()[:8]}")
    n0 = np.full(64, ld, np.uint32)                                                    # every row full
    assert_same(L.op_sort_candidates(pool, n0), reference(pool, n0), f"ld {ld}, 64 full rows")


@gpu
@pytest.mark.parametrize("ld,levels", [(20000, 5), (70000, 3), (8192, 1)])
def test_ties_by_the_thousand_keep_index_order(L, ld, levels):
    rng = np.random.default_rng(9100 + ld)
    x = candidates(L, rng, 3, ld, levels)
    assert np.unique(x["prob"][1]).size <= levels + 1
    n0 = np.array([ld, ld - 3, ld // 2], np.uint32)
    got = L.op_sort_candidates(x, n0)
    assert_same(got, reference(x, n0), f"ld {ld}, {levels} levels")
    for r in range(3):                                                                 # said directly: inside a run of equal probabilities the indices ascend
        p, i = got["prob"][r, : n0[r]], got["index"][r, : n0[r]].astype(np.int64)
        assert (np.diff(p) <= 0).all() and (np.diff(i)[np.diff(p) == 0] > 0).all()


@gpu
def test_rows_without_candidates_are_left_alone(L):
    rng = np.random.default_rng(9200)
    x = candidates(L, rng, 4, 9000)
    n0 = np.zeros(4, np.uint32)
    assert_same(L.op_sort_candidates(x, n0), x, "no candidates anywhere")
    n0[2] = 9000
    assert_same(L.op_sort_candidates(x, n0), reference(x, n0), "one row of four")


@gpu
def test_refusals_name_the_hook_and_a_valid_call_follows(L):
    lib = L.lib()
    rng = np.random.default_rng(9300)
    x = candidates(L, rng, 2, 100)
    out = x.copy()
    n0 = np.array([100, 7], np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cases = [
        ((0, None, 2, 100, p(n0), p(out)), "NULL argument"), ((0, p(x), 2, 100, None, p(out)), "NULL argument"), ((0, p(x), 2, 100, p(n0), None), "NULL argument"),
        ((0, p(x), 0, 100, p(n0), p(out)), "n_rows = 0 is outside 1 .. 64"), ((0, p(x), 65, 100, p(n0), p(out)), "n_rows = 65 is outside 1 .. 64"),
        ((0, p(x), 2, 0, p(n0), p(out)), "need 1 <= ld <= 2^24"), ((0, p(x), 2, (1 << 24) + 1, p(n0), p(out)), "need 1 <= ld <= 2^24"),
        ((0, p(x), 2, 99, p(n0), p(out)), "row 0: n0 = 100 exceeds ld = 99"),
    ]
    seen = set()
    for args, msg in cases:
        assert lib.lmrs_op_sort_candidates(*args) != 0, msg
        err = lib.lmrs_last_error().decode()
        assert msg in err and err.startswith("lmrs_op_sort_candidates: "), err
        seen.add(err)
        assert_same(L.op_sort_candidates(x, n0), reference(x, n0), f"after {msg!r}")
    assert len(seen) == 5, "a message each"
    with pytest.raises(L.LmrsError, match="one n0 per row"):
        L.op_sort_candidates(x, n0[:1])
