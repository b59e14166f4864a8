"""The filter rule of lmrs_batch_set_filters (include/lmrs_hip.h) in numpy: np.float32 scalars, the candidate order from a stable argsort of the keys the
kernels order by (lmrs_score.hip, topk_key).  The reference of tests/test_batch_filter.py; tests/test_batch_filter_host.py holds it against a naive full
sort."""
import numpy as np

INF = np.float32(np.inf)


def value_words(row):
    """the high word of topk_key for every entry: the value's bits made monotone, -0.0 folded onto +0.0, a NaN 0 (below -inf) - but all ones at index 0"""
    row = np.asarray(row, np.float32)
    b = row.view(np.uint32).copy()
    b[b == 0x80000000] = 0
    neg = (b & 0x80000000) != 0
    hi = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    nan = np.isnan(row)
    hi[nan] = 0
    if row.size and nan[0]:
        hi[0] = 0xFFFFFFFF
    return hi


def order(row):
    """the indices of the row in candidate order: descending value word, equal words by ascending index (the sort is stable)"""
    return np.argsort(-value_words(row).astype(np.int64), kind="stable")


def filtered(row, top_k=0, min_gap=INF):
    """row (float32 [V]) as the sinks see it under top_k (0: off) and min_gap (inf: off): steps 1 - 4 of the header's rule"""
    out = np.asarray(row, np.float32).copy()
    V = out.size
    top_k, min_gap = int(top_k), np.float32(min_gap)
    assert top_k >= 0 and not np.isnan(min_gap) and min_gap >= 0
    cand = order(out)
    m = out[cand[0]]
    if top_k != 0 and top_k < V:
        out[cand[top_k:]] = -INF
    if np.isfinite(min_gap) and not np.isnan(m):
        with np.errstate(all="ignore"):
            thr = np.float32(m - min_gap)
            out[~(out >= thr)] = -INF
    return out
