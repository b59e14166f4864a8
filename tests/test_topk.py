"""lmrs_score_tokens_topk / lmrs_forward_topk / lmrs_op_topk (include/lmrs_hip.h): the k first next-token candidates of a position, selected on
the device.  The reference is the CPU oracle's SEQUENTIAL forward (one call per token), its rows ranked on the host by rank_row below - a stable
sort on (-value, index) with the NaN rules of the header - never a second call into the library.  Indices must be equal; log-probabilities
follow tests/parity_rules.py's rule (one f32 ulp of a float64 log-softmax of the oracle's logits: check_scores itself on the results
lmrs_score_tokens also has, topk_rule - the same arithmetic over k columns instead of one target - on the rest)."""
import ctypes
import dataclasses
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, assert_within_one_ulp, check_scores, log_softmax64, oracle_rows, ref_argmax
from tools import synth_lmrs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
NEW = ("lmrs_score_tokens_topk", "lmrs_forward_topk", "lmrs_op_topk")


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


# ------------------------------------------------------------------ the host reference
def rank_row(row):
    """Every index of `row` in candidate order: the larger value first (-0.0 == +0.0), equal values by ascending index, NaNs after every
    number in index order - and a NaN at index 0 in front of everything (sampler.rs:29-41 starts at index 0 and moves on a strict `>`)."""
    row = np.asarray(row, np.float32)
    nan = np.isnan(row)
    neg = -np.where(nan, np.float32(0), row).astype(np.float64)
    order = np.lexsort((np.arange(row.size), neg, nan))          # stable; keys from the last: NaN flag, -value, index
    if nan[0]:
        order = np.concatenate(([0], order[order != 0]))
    return order


def topk_rule(tl, ti, rows, what):
    """check_scores' rule for log-probabilities, over the k indices ti[t] of every row instead of one target"""
    x, m, lse = log_softmax64(rows)
    assert_within_one_ulp(tl, np.take_along_axis(x, ti.astype(np.int64), axis=1) - m[:, None] - lse[:, None], f"{what}: top-k log-probabilities")


def guided_tokens(orc, cfg, n, start, seed, picks=(0, 2, None, 7, 300, 1, None, 40)):
    """n tokens and the oracle's rows for them: a random first token, then by turns the oracle's rank-p candidate (p from `picks`) or a
    random token (None) - so that targets fall inside and outside the top k at known ranks"""
    rand = S.prompt_tokens(cfg, n, seed)
    toks, rows = [int(rand[0])], []
    for t in range(n):
        rows.append(orc.forward(toks[t], start + t).copy())
        p = picks[t % len(picks)]
        toks.append(int(rand[t]) if p is None else int(rank_row(rows[t])[p]))
    return np.array(toks[:n], np.uint32), np.stack(rows)


def check_topk(L, img, got, rows, toks, start, k, what, inside_min=0):
    """score_topk's six results against the oracle's rows, and the first three against Transformer.score on a fresh context"""
    lp, am, s, ti, tl, rk = got
    n = len(toks)
    assert ti.shape == (n, k) and tl.shape == (n, k) and rk.shape == (n - 1,)
    check_scores((lp, am, s), rows, toks, what)
    plain = L.Transformer(img).score(toks, start)
    assert_bit_equal(lp, plain[0], f"{what}: logprobs against score()")
    assert am.tolist() == plain[1].tolist() and s == plain[2], f"{what}: argmax / sum against score()"
    orders = [rank_row(r) for r in rows]
    want = np.stack([o[:k] for o in orders])
    bad = np.flatnonzero((ti != want).any(axis=1))
    assert bad.size == 0, f"{what}: top-{k} indices differ at positions {bad[:5]}: {ti[bad[0]][:12]} vs {want[bad[0]][:12]}"
    assert ti[:, 0].tolist() == am.tolist(), f"{what}: rank 0 is not the argmax"
    topk_rule(tl, ti, rows, what)
    want_rk = np.array([int(np.flatnonzero(orders[t] == toks[t + 1])[0]) for t in range(n - 1)], np.uint32)
    assert rk.tolist() == want_rk.tolist(), f"{what}: target_rank"
    inside = np.flatnonzero(rk < k)
    assert inside.size >= inside_min, f"{what}: {inside.size} targets inside the top {k}"
    assert_bit_equal(tl[inside, rk[inside]], lp[inside], f"{what}: the target's entry against logprobs")
    return orders


# ------------------------------------------------------------------ CPU
def test_new_symbols_are_declared_exported_and_mirrored():
    import lmrs_amd
    import test_rust_crate as R
    lmrs_amd.build()
    lib = ctypes.CDLL(lmrs_amd.LIB_PATH)
    c, r = R.c_prototypes(), R.rust_externs()
    for name in NEW:
        assert name in c, f"{name} is not in include/lmrs_hip.h"
        assert name in lmrs_amd.EXPORTS and hasattr(lib, name), name
        assert name in r, f"{name} is not declared in rust/lmrs-hip/src/ffi.rs"
        (cret, cargs), (rret, rargs) = c[name], r[name]
        assert R.CMAP[cret] == rret and [R.CMAP[a] for a in cargs] == rargs, (name, cargs, rargs)
    assert hasattr(lmrs_amd.Transformer, "score_topk") and hasattr(lmrs_amd.Transformer, "forward_topk") and hasattr(lmrs_amd, "topk")
    t = re.sub(r"\s+", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "transformer.rs")).read())
    assert "pub fn score_topk(&mut self, tokens: &[u32], k: u32, start_pos: u32) -> ScoreTopk" in t
    assert "pub fn forward_topk(&mut self, token: u32, pos: u32, k: u32) -> (Vec<u32>, Vec<f32>)" in t
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    assert "lmrs_score_tokens_topk" in hpp and "lmrs_forward_topk" in hpp
    for f in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        txt = open(os.path.join(ROOT, f)).read()
        assert "lmrs_score_tokens_topk" in txt and "lmrs_forward_topk" in txt, f


def test_k_is_checked_before_any_device_work(L):
    """k = 0, k = 257 and k > vocab, through the paths that need no device: the k range comes before the context is looked at, and
    lmrs_op_topk checks all of its arguments before it opens the device"""
    lib = L.lib()
    row = np.arange(40, dtype=np.float32); idx = np.zeros(300, np.uint32); val = np.zeros(300, np.float32)
    toks = np.zeros(4, np.uint32)
    err = lambda: lib.lmrs_last_error().decode()
    for k, msg in ((0, "k = 0 is outside 1 .. 256"), (257, "k = 257 is outside 1 .. 256")):
        assert lib.lmrs_op_topk(0, row.ctypes.data, row.size, row.size, k, idx.ctypes.data, val.ctypes.data) != 0 and msg in err()
        assert lib.lmrs_forward_topk(None, 0, 0, k, idx.ctypes.data, val.ctypes.data) != 0 and msg in err()
        assert lib.lmrs_score_tokens_topk(None, toks.ctypes.data, 4, 0, k, None, None, None, idx.ctypes.data, val.ctypes.data, None) != 0 and msg in err()
    assert lib.lmrs_op_topk(0, row.ctypes.data, row.size, row.size, 41, idx.ctypes.data, val.ctypes.data) != 0
    assert "k = 41 exceeds vocab_size = 40" in err()
    assert lib.lmrs_op_topk(0, row.ctypes.data, row.size, row.size + 1, 4, idx.ctypes.data, val.ctypes.data) != 0 and "written" in err()
    assert lib.lmrs_score_tokens_topk(None, toks.ctypes.data, 4, 0, 5, None, None, None, None, val.ctypes.data, None) != 0 and "NULL" in err()
    assert lib.lmrs_forward_topk(None, 0, 0, 5, idx.ctypes.data, val.ctypes.data) != 0 and "NULL" in err()
    with pytest.raises(L.LmrsError, match="outside 1 .. 256"):
        L.topk(row, 0)


def test_rank_row_agrees_with_the_reference_argmax_at_rank_0():
    rng = np.random.default_rng(7)
    rows = [rng.standard_normal(500).astype(np.float32) for _ in range(4)]
    rows[1][[3, 77]] = rows[1].max() + 1                                        # a tied maximum: the first index
    rows[2][0] = np.nan                                                         # a NaN at index 0 is never displaced
    rows[3][[5, 9]] = np.nan; rows[3][200] = np.inf                             # NaNs elsewhere never win
    rows.append(np.array([-0.0, 0.0, -1.0, 0.0], np.float32))                   # -0.0 == +0.0: index 0
    rows.append(np.full(6, np.nan, np.float32))
    for r in rows:
        o = rank_row(r)
        assert sorted(o.tolist()) == list(range(r.size))
        assert int(o[0]) == ref_argmax(r)
    o = rank_row(rows[3])
    assert o[0] == 200 and o[-2:].tolist() == [5, 9]
    assert rank_row(rows[2])[0] == 0 and rank_row(rows[4]).tolist() == [0, 1, 3, 2]


def test_topk_kernels_have_no_scratch_and_no_spills():
    import lmrs_amd
    from tools import kernel_resources as KR
    lmrs_amd.build()
    ks = [(n, k) for n, k in KR._kernels_of(os.path.join(KR.CSRC, "lmrs_score.o")) if "topk_" in n]
    names = " ".join(n for n, _ in ks)
    assert "topk_chunk_kernel" in names and "topk_merge_kernel" in names, names
    for n, k in ks:
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (n, k)


def test_perplexity_program_and_host_mirror_compile_with_topk(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "lm.rs_amd/hostcpp/transformer.hpp"\n'
                   'int main(int argc, char**) {\n'
                   '    if (argc > 99) {\n'
                   '        auto [m, used] = lmrs_host::Transformer::create(nullptr, 0); (void)used;\n'
                   '        auto s = m.score_topk({1, 2, 3}, 5, 0); auto [i, v] = m.forward_topk(0, 0, 5);\n'
                   '        return (int)(s.topk_idx.size() + s.topk_logprob.size() + s.target_rank.size() + s.logprobs.size() + i.size() + v.size());\n'
                   '    }\n'
                   '    return 0;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", ROOT, str(src)], check=True, capture_output=True)
    ppl = os.path.join(ROOT, "lm.rs_amd", "hostcpp", "perplexity.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", ppl], check=True, capture_output=True)
    assert "--topk" in open(ppl).read() and "--topk" in open(os.path.join(ROOT, "tools", "score_rate.py")).read()


# ------------------------------------------------------------------ GPU: scoring
@functools.lru_cache(maxsize=None)
def _llama_run():
    """the reference of the four k of the batched case, computed once"""
    img = S.build_image("mini-llama", S.Q8_0, seed=37)
    return guided_tokens(O.Oracle(img), "mini-llama", 40, 2, 37)


@gpu
@pytest.mark.parametrize("k", [1, 5, 64, 256])
def test_batched_pass_one_chunk_pair(L, k):
    """mini-llama Q8_0, 40 tokens from position 2: the batched pass, 4096 logits = two chunks a row"""
    img = S.build_image("mini-llama", S.Q8_0, seed=37)
    toks, rows = _llama_run()
    m = L.Transformer(img)
    assert m.tokens_path(40)
    # the 39 targets by construction: five each at ranks 0, 1, 2, 7 and 300, four at 40, ten random ones
    check_topk(L, img, m.score_topk(toks, k, 2), rows, toks, 2, k, f"mini-llama k={k}", inside_min={1: 5, 5: 15, 64: 24, 256: 24}[k])


@gpu
def test_many_chunks_and_a_ragged_last_chunk(L):
    """a vocabulary of 40000: 20 chunks a row, the last of 1088 logits"""
    cfg = "mini-llama-v40k"
    img = S.build_image(cfg, S.Q8_0, seed=39)
    toks, rows = guided_tokens(O.Oracle(img), cfg, 24, 0, 39)
    check_topk(L, img, L.Transformer(img).score_topk(toks, 64, 0), rows, toks, 0, 64, cfg, inside_min=14)


def _sunk_logits(name, layer, row0, w):
    """Channel 0 of every embedding row a constant and the final norm's weight for it large and negative: the classifier's (tied) column 0
    then shifts every written logit of a position by the same amount, far below zero at about half the positions"""
    if name == "embed_tokens":
        w = w.copy(); w[:, 0] = np.float32(0.1)
    elif name == "norm":
        w = w.copy(); w[0, 0] = np.float32(-100.0)
    return w


@gpu
def test_zero_tail_on_the_token_path(L):
    """A vocabulary of 4102: the classifier writes 4100 logits, entries 4100 and 4101 count as 0.0 and are never read; rows go through the
    decode step one by one.  Witness on the oracle's rows: at some positions the 16th value is <= 0, so the tail must be among the 16."""
    cfg, k = "mini-llama-v4102", 16
    img = S.build_image(cfg, S.Q8_0, seed=61, transform=_sunk_logits)
    toks = S.prompt_tokens(cfg, 20, 61)
    m = L.Transformer(img)
    rows = oracle_rows(O.Oracle(img), toks, 0)
    assert np.isfinite(rows).all() and not rows[:, 4100:].any()
    kth = -np.sort(-rows, axis=1)[:, k - 1]
    sunk = np.flatnonzero(kth <= 0)
    assert 3 <= sunk.size <= 17, f"the recipe must sink some rows and leave others: {kth}"
    orders = check_topk(L, img, m.score_topk(toks, k, 0), rows, toks, 0, k, cfg)
    for t in sunk:
        assert {4100, 4101} <= set(orders[t][:k].tolist()), t


@gpu
def test_exact_ties_come_out_in_index_order(L):
    """tied_classifier on mini-phi: every logit has a bit-identical twin V/2 rows away - in the row's other chunk"""
    import test_stress_regimes as SR
    cfg, k = "mini-phi", 64
    n = SR.N_DECODE[cfg]
    img, c, toks, rows, kv, st = SR.oracle_decode(cfg, S.Q8_0, "tied_classifier", n)
    SR.check_witness("tied_classifier", c, S.Q8_0, st, rows, n)
    got = L.Transformer(img).score_topk(toks, k, 0)
    orders = check_topk(L, img, got, rows, toks, 0, k, "mini-phi tied_classifier")
    def ties_in_index_order(ti, rows_):
        count = 0
        for t in range(len(ti)):
            v = rows_[t][ti[t]]
            eq = v[1:] == v[:-1]
            assert (ti[t][1:][eq] > ti[t][:-1][eq]).all(), f"position {t}: equal values out of index order"
            count += int(eq.sum())
        return count
    assert ties_in_index_order(got[3], rows) >= n * k // 4, "ties among the top k"
    # an odd k cuts a pair of twins in two: the boundary itself falls inside a tie, and the lower twin is the one that stays
    k = 33
    cut = [t for t in range(30) if rows[t][orders[t][k - 1]] == rows[t][orders[t][k]]]
    assert len(cut) >= 15, f"positions whose tie spans the top-{k} boundary: {cut}"
    got = L.Transformer(img).score_topk(toks[:30], k, 0)
    ties_in_index_order(got[3], rows)
    for t in cut:
        assert (got[3][t] == orders[t][:k]).all() and orders[t][k - 1] < orders[t][k], t


@gpu
def test_gemma_soft_cap(L):
    """softcap on mini-gemma Q4_0: the batched pass caps the first `dim` logits in a launch of its own before the selection; saturated logits
    are +-30 exactly, in long runs of equal values"""
    import test_stress_regimes as SR
    cfg, k, n = "mini-gemma", 32, 30
    img, c, toks, rows, kv, st = SR.oracle_decode(cfg, S.Q4_0, "softcap", n)
    SR.check_witness("softcap", c, S.Q4_0, st, rows, n)
    assert ((rows == 30.0).sum(axis=1) >= 2).any(), "no position with several logits saturated at the cap"
    check_topk(L, img, L.Transformer(img).score_topk(toks, k, 0), rows, toks, 0, k, "mini-gemma softcap")


@gpu
def test_a_row_does_not_depend_on_the_call_around_it(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=43)
    toks = S.prompt_tokens("mini-llama", 40, 43)
    one = L.Transformer(img).score_topk(toks, 20, 0)
    m = L.Transformer(img)
    a, b = m.score_topk(toks[:25], 20, 0), m.score_topk(toks[25:], 20, 25)
    assert (np.concatenate([a[3], b[3]]) == one[3]).all()
    assert_bit_equal(np.concatenate([a[4], b[4]]), one[4], "top-k log-probabilities, one call against 25 + 15")
    assert np.concatenate([a[5], b[5]]).tolist() == np.delete(one[5], 24).tolist()
    rows = oracle_rows(O.Oracle(img), toks, 0)
    assert (one[3] == np.stack([rank_row(r)[:20] for r in rows])).all()


@gpu
def test_score_topk_errors_leave_the_context_usable(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=47)
    m = L.Transformer(img)
    toks = S.prompt_tokens("mini-llama", 24, 47)
    small = dataclasses.replace(S.CONFIGS["tiny-llama"], name="tiny-llama-v128", vocab_size=128)
    simg = S.build_image(small, S.Q8_0, seed=3)
    ms = L.Transformer(simg)
    with pytest.raises(L.LmrsError, match="k = 129 exceeds vocab_size = 128"):
        ms.score_topk([1, 2, 3], 129)
    with pytest.raises(L.LmrsError, match="k = 200 exceeds vocab_size = 128"):
        ms.forward_topk(1, 0, 200)
    stoks = S.prompt_tokens(small, 9, 3)
    check_topk(L, simg, ms.score_topk(stoks, 128, 0), oracle_rows(O.Oracle(simg), stoks, 0), stoks, 0, 128, "k = vocab_size = 128")
    with pytest.raises(L.LmrsError, match="outside 1 .. 256"):
        m.score_topk(toks, 0)
    bad = toks.copy(); bad[5] = m.args.vocab_size
    with pytest.raises(L.LmrsError, match="out of range"):
        m.score_topk(bad, 4)
    grp = L.ShardGroup(img, 2)
    ti = np.zeros((24, 4), np.uint32); tl = np.zeros((24, 4), np.float32)
    rc = L.lib().lmrs_score_tokens_topk(grp._arr[0], toks.ctypes.data, toks.size, 0, 4, None, None, None, ti.ctypes.data, tl.ctypes.data, None)
    assert rc != 0 and "single-GPU" in L.lib().lmrs_last_error().decode()
    grp.close()
    rows = oracle_rows(O.Oracle(img), toks, 0)
    check_topk(L, img, m.score_topk(toks, 4, 0), rows, toks, 0, 4, "after the errors")
    check_topk(L, img, m.score_topk(toks, 100, 0), rows, toks, 0, 100, "a larger k on the same context")


# ------------------------------------------------------------------ GPU: the decode step
@gpu
@pytest.mark.parametrize("q", [S.Q8_0, S.Q_NONE])
def test_forward_topk_matches_the_ranked_oracle_logits(L, q):
    img = S.build_image("mini-llama", q, seed=53)
    m = L.Transformer(img); orc = O.Oracle(img)
    toks = S.prompt_tokens("mini-llama", 13, 53)
    for pos in range(12):
        k = (1, 40, 256)[pos % 3]
        idx, val = m.forward_topk(int(toks[pos]), pos, k)
        row = orc.forward(int(toks[pos]), pos).copy()
        want = rank_row(row)[:k]
        assert (idx == want).all(), f"step {pos}: {idx[:8]} vs {want[:8]}"
        assert_bit_equal(val, row[want], f"step {pos}: raw logits of the top {k}")
    assert_bit_equal(m.forward(int(toks[12]), 12), orc.forward(int(toks[12]), 12), "forward after 12 forward_topk steps")


@gpu
def test_forward_topk_refuses_a_shard(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=53)
    grp = L.ShardGroup(img, 2)
    idx = np.zeros(8, np.uint32); val = np.zeros(8, np.float32)
    rc = L.lib().lmrs_forward_topk(grp._arr[0], 1, 0, 8, idx.ctypes.data, val.ctypes.data)
    assert rc != 0 and "single-GPU" in L.lib().lmrs_last_error().decode()
    grp.close()
    m = L.Transformer(img)
    with pytest.raises(L.LmrsError, match="out of range"):
        m.forward_topk(m.args.vocab_size, 0, 8)


# ------------------------------------------------------------------ GPU: the ordering rule on hand-made rows
def _hand_rows():
    rng = np.random.default_rng(11)
    nan0 = rng.standard_normal(3000).astype(np.float32); nan0[0] = np.nan; nan0[[17, 2500]] = np.nan
    nans = rng.standard_normal(200).astype(np.float32); nans[[3, 60, 199]] = np.nan; nans[100] = -np.inf; nans[101] = np.inf
    zeros = np.where(rng.integers(0, 2, 5000) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    few = rng.integers(-3, 4, 10000).astype(np.float32)                          # seven values: ties across lanes, waves and chunks
    neg = -np.abs(rng.standard_normal(4102)).astype(np.float32) - 1
    return [("a NaN at 0, NaNs elsewhere", nan0, 3000, 256), ("k = vocab with NaNs and infinities", nans, 200, 200),
            ("signed zeros", zeros, 5000, 256), ("all equal", np.full(5000, 2.5, np.float32), 5000, 256), ("all NaN", np.full(2100, np.nan, np.float32), 2100, 7),
            ("seven values", few, 10000, 256), ("seven values, k = 1", few, 10000, 1), ("negative with a zero tail", neg, 4100, 16),
            ("nothing written", neg, 0, 5), ("one chunk, ragged", rng.standard_normal(300).astype(np.float32), 300, 256),
            ("one entry", np.array([np.nan], np.float32), 1, 1)]


@gpu
@pytest.mark.parametrize("what,row,written,k", _hand_rows(), ids=[h[0] for h in _hand_rows()])
def test_ordering_rule_on_hand_made_rows(L, what, row, written, k):
    full = row.copy(); full[written:] = 0.0                                      # what the row counts as
    idx, val = L.topk(row, k, written)
    want = rank_row(full)[:k]
    assert (idx == want).all(), f"{what}: {idx[:10]} vs {want[:10]}"
    assert_bit_equal(val, full[want], what)
    assert int(idx[0]) == ref_argmax(full), what
