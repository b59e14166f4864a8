"""sample_topp from its sort on (sampler.rs:81-105) as the device launches of lmrs_batch_generate_topp implement it, written out in numpy: the witness
tests/test_batch_generate_topp_host.py checks against lmrs_sampler_topp_pairs and tests/test_batch_generate_topp.py compares lmrs_op_topp_rows with.

A step takes this call's n0 candidates {prob, index} in ascending index order and the sampler's persistent vector (n pairs, descending prob) and gives
the token and the new vector:
  1. the candidates by (prob descending, index ascending) - the stable sort of the index-ordered candidates;
  2. merged stably with entries [n0, n) of the old vector, equal probabilities from the candidates first, BY RANK: candidate i lands at
     i + #{rest entries > it}, rest entry j at j + #{candidates >= it};
  3. the f32 chain over the new vector's first n0 entries until it exceeds top_p (last_idx; n0 - 1 when it never does), r = rnd * cumulative, the same
     chain again up to last_idx: the first entry with r < cdf, else the entry at last_idx.
n0 == 0: no token (None) and the vector as it was."""
import numpy as np

PAIR = np.dtype([("prob", np.float32), ("index", np.uint32)])


def pairs(prob, index):
    out = np.zeros(len(prob), PAIR)
    out["prob"] = prob; out["index"] = index
    return out


def sort_candidates(cand):
    """index-ordered candidates -> by descending prob, ties by ascending index"""
    assert np.all(np.diff(cand["index"].astype(np.int64)) > 0), "the candidates come in ascending index order"
    return cand[np.argsort(-cand["prob"].astype(np.float64), kind="stable")]


def rank_merge(sorted_cand, rest):
    """both descending by prob -> their stable merge, candidates first on ties, every element placed by its own rank"""
    c, o = -sorted_cand["prob"].astype(np.float64), -rest["prob"].astype(np.float64)
    at_c = np.arange(c.size) + np.searchsorted(o, c, side="left")         # rest entries strictly above the candidate
    at_o = np.arange(o.size) + np.searchsorted(c, o, side="right")        # candidates at or above the rest entry
    out = np.zeros(c.size + o.size, PAIR)
    seen = np.zeros(out.size, np.int64)
    np.add.at(seen, at_c, 1); np.add.at(seen, at_o, 1)
    assert np.all(seen == 1), "the ranks are not a permutation: a vector was not ordered"
    out[at_c] = sorted_cand; out[at_o] = rest
    return out


def chain(prob):
    """the running f32 sum, term by term in order"""
    return np.add.accumulate(np.asarray(prob, np.float32), dtype=np.float32)


def cut_and_draw(vec, n0, top_p, rnd):
    cum = chain(vec["prob"][:n0])
    over = np.nonzero(cum > np.float32(top_p))[0]
    last = int(over[0]) if over.size else n0 - 1
    r = np.float32(rnd) * cum[last]
    hit = np.nonzero(r < cum[:last + 1])[0]
    return int(vec["index"][int(hit[0]) if hit.size else last])


def step(cand, n0, state, top_p, rnd):
    """-> (token or None, the new vector)"""
    state = np.asarray(state, PAIR)
    if n0 == 0:
        return None, state.copy()
    new = rank_merge(sort_candidates(np.asarray(cand, PAIR)[:n0]), state[n0:])
    return cut_and_draw(new, n0, top_p, rnd), new


def host_step(L, sampler, cand, n0):
    """the same step through lmrs_sampler_topp_pairs on a host sampler that holds the vector -> (token or None, the new vector)"""
    c = np.asarray(cand, PAIR)[:n0]
    try:
        tok = sampler.topp_pairs(c["prob"].copy(), c["index"].copy())
    except L.LmrsError as e:
        assert n0 == 0 and "no candidate" in str(e), str(e)
        tok = None
    return tok, sampler.candidates()[0]
