"""Candidate filters on batch slots (lmrs_batch_set_filters / _clear_filters / _filter_info, lmrs_op_filter_rows; include/lmrs_hip.h): top_k and min_gap on
the device, behind the penalties and the masks and in front of every sink.  The reference is one CPU oracle PER SEQUENCE whose logits row goes through
filter_rules.filtered - the header's rule in numpy - before Sampler::sample (the oracle's), sample_argmax (lmrs_ref_argmax) or the top-k definition
(tests/test_topk.py).  Every comparison is exact: logits bit for bit, tokens and indices by value.  In every sampled case the filtered oracle's tokens
differ from the unfiltered oracle's somewhere (asserted on the CPU side): no test passes with the filter ignored."""
import ctypes
import dataclasses

import numpy as np
import pytest

import oracle_lib as O
from filter_rules import INF, filtered
from parity_rules import assert_bit_equal, assert_within_one_ulp, ref_argmax
from penalty_rules import params
from test_batch import Seq as TokenSeq, check_slot_rows
from test_batch_generate import BUDGET, STOP, Row, expect, rounds, want_logprobs
from test_batch_mask import ban, masked
from test_batch_penalty import Seq as RecordSeq, alphabet, from_alphabet
from test_topk import rank_row, topk_rule
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
V = 4096


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


# ---------------------------------------------------------------------------------------------- 1. the kernel alone

def check_rows(L, rows, top_k, min_gap, what, n=None):
    """lmrs_op_filter_rows over `rows` against filtered() row by row, bit for bit; columns from n on must come back untouched"""
    rows = np.ascontiguousarray(rows, np.float32)
    R, ld = rows.shape
    n = ld if n is None else n
    k = np.broadcast_to(np.asarray(top_k, np.uint32), (R,))
    g = np.broadcast_to(np.asarray(min_gap, np.float32), (R,))
    got = L.filter_rows(rows, k, g, n=n)
    for r in range(R):
        want = filtered(rows[r, :n], k[r], g[r])
        assert_bit_equal(got[r, :n], want, f"{what}: row {r} (top_k {k[r]}, min_gap {g[r]})")
        assert_bit_equal(got[r, n:], rows[r, n:], f"{what}: row {r}: the floats behind the row")
    return got


WIDTHS = [33, 2052, 4096, 131072]


@gpu
@pytest.mark.parametrize("n", WIDTHS)
def test_the_kernel_alone_on_random_rows(L, n):
    rng = np.random.default_rng(n)
    rows = (rng.standard_normal((6, n)) * 6).astype(np.float32)
    rows[1, rng.integers(0, n, n // 8)] = 0.0; rows[1, 3] = -0.0              # ties at a common value, both zeros
    rows[2] = np.round(rows[2])                                             # many ties at every value
    rows[3, 5] = np.float32(3e38); rows[3, 7] = np.float32(-1e-40); rows[3, 9] = -INF; rows[3, 11] = np.nan
    rows[5, 0] = np.nan                                                      # a NaN at index 0: the first candidate, and no gap step
    for top_k, gap in ((1, INF), (2, INF), (5, INF), (40, INF), (n - 1, INF), (n, INF), (n + 7, INF), (n // 2, INF), (0, 0.0), (0, 1e-30), (0, 2.5), (0, 40.0),
                       (5, 0.5), (40, 3.0), (n // 2, 4.0), (0, INF)):
        got = check_rows(L, rows, top_k, gap, f"n = {n}")
        if 0 < top_k < n and gap == INF:
            assert ((~np.isneginf(got[:3])).sum(axis=1) == top_k).all(), f"n = {n}, top_k = {top_k}: exactly top_k entries stay"
    # every row its own parameters in one launch, unfiltered rows (handed over as slot -1) among them
    check_rows(L, rows, [5, 0, n - 1, 0, 3, 0], [INF, INF, 1.0, 2.0, 0.0, INF], f"n = {n}: mixed rows")


@gpu
@pytest.mark.parametrize("n", WIDTHS)
def test_the_kernel_alone_on_ties(L, n):
    """rows of equal values (the index tie-break, through every round of the select, with more ties than any LDS buffer holds), a two-valued row whose
    threshold falls inside the larger class, and a row that is half -inf under a top_k beyond the finite count"""
    rng = np.random.default_rng(7 * n)
    flat = np.full((1, n), np.float32(1.25))
    for top_k in [k for k in (1, 5, 255, 256, 257, 70000) if k < n]:
        got = check_rows(L, flat, top_k, INF, f"n = {n}: all equal")
        assert np.array_equal(np.flatnonzero(~np.isneginf(got[0])), np.arange(top_k)), f"n = {n}, top_k = {top_k}: the first top_k indices stay"
    check_rows(L, flat, 0, 0.0, f"n = {n}: all equal, gap 0")                  # every value tied at thr stays
    two = np.where(rng.random((1, n)) < 0.25, np.float32(2.0), np.float32(-1.0)).astype(np.float32)
    hi = int((two > 0).sum())
    for top_k in [k for k in (hi - 1, hi, hi + 1, hi + (n - hi) // 2, n - 1) if 0 < k < n]:
        check_rows(L, two, top_k, INF, f"n = {n}: two values, {hi} of the larger")
    check_rows(L, two, hi + 3, 3.0, f"n = {n}: two values, the gap keeps both")
    check_rows(L, two, hi + 3, 2.0, f"n = {n}: two values, the gap cuts the smaller")
    half = (rng.standard_normal((2, n)) * 3).astype(np.float32)
    half[:, rng.permutation(n)[: n // 2]] = -INF
    fin = int((~np.isneginf(half[0])).sum())
    for top_k in (fin - 1, fin, fin + 1, min(n - 1, fin + 5)):
        got = check_rows(L, half, top_k, INF, f"n = {n}: half -inf")
        assert_bit_equal(got[0][np.isneginf(half[0])], half[0][np.isneginf(half[0])], "entries that were -inf stay")


@gpu
def test_the_kernel_alone_with_a_stride_and_an_odd_start(L):
    """ld > n: rows of 2050 logits at stride 2053 - every row but the first starts off a 16-byte boundary (the scalar path) - and at stride 2056 (float4 path
    with a tail of two); the floats between the rows come back as they went"""
    rng = np.random.default_rng(99)
    for ld in (2053, 2056):
        rows = (rng.standard_normal((5, ld)) * 5).astype(np.float32)
        rows[2, :2050] = np.round(rows[2, :2050])
        check_rows(L, rows, [40, 0, 7, 2049, 0], [INF, 1.5, 2.0, INF, INF], f"ld = {ld}", n=2050)


# ---------------------------------------------------------------------------------------------- 2. the per-call passes

# (top_k, min_gap) per row in turn; None: the row has no filter.  The synthetic rows are flat (logits within a few units of each other), so top_k = 5 at
# temperature about 1 moves nearly every draw
FILTERS = [(5, INF), None, (0, 0.5), (40, 1.0), None, (3, INF), (1, INF), (0, 0.0)]


class FRow(Row):
    """test_batch_generate.Row - oracle, record, penalties, mask, samplers - with the slot's filter behind them: feed() gives the row the sinks see; .plain the
    row in front of the filter, and .twin (a second reference sampler of the same kind and seed) what the sampler would have drawn from THAT row"""

    def __init__(self, L, img, slot, kind=None, flt=None, **kw):
        super().__init__(L, img, slot, kind=kind, **kw)
        self.flt, self.plain, self.moved = flt, None, 0
        self.twin = O.Sampler(V, kind[0], kind[1], kind[2]) if kind is not None else None

    def feed(self, tok):
        self.plain = super().feed(tok)
        return filtered(self.plain, *self.flt) if self.flt else self.plain

    def choose(self, row):
        t = super().choose(row)
        if self.twin is not None and self.twin.sample(self.plain.copy()) != t:
            self.moved += 1
        return t


def set_filters(b, rows):
    """every row's .flt (None: cleared) in one set_filters call and one clear_filters call; filter_info says the same"""
    on = [r for r in rows if r.flt is not None]
    if on:
        b.set_filters([r.slot for r in on], [r.flt[0] for r in on], [r.flt[1] for r in on])
    b.clear_filters([r.slot for r in rows if r.flt is None])
    for r in rows:
        info = b.filter_info(r.slot)
        if r.flt is None:
            assert info == dict(top_k=0, min_gap=float("inf"), active=False), (r.slot, info)
        else:
            active = 0 < r.flt[0] < V or np.isfinite(r.flt[1])
            assert info == dict(top_k=r.flt[0], min_gap=float(np.float32(r.flt[1])), active=bool(active)), (r.slot, info)


def batch_of(L, m, form, n):
    if form == "paged":
        return L.Batch(m, n, page_len=64, n_pages=4 * n + 4)
    return L.Batch(m, n, wide=form == "wide")


FORMS = [("mini-llama", S.Q8_0, "rows"), ("mini-llama", S.Q8_0, "wide"), ("mini-llama", S.Q8_0, "paged"), ("mini-phi", S.Q8_0, "rows"),
         ("mini-gemma", S.Q4_0, "rows"), ("mini-gemma", S.Q4_0, "wide")]
PASS_DEPTHS = [0, 1, 7, 63, 64, 65, 2, 33]


@gpu
@pytest.mark.parametrize("cfg,q,form", FORMS)
def test_forward_and_forward_runs_under_filters(L, cfg, q, form):
    """filtered and unfiltered slots in one pass: forward with logits, then forward_runs with runs of three tokens, two outputs each, logits and the eight
    first candidates (top_k = 5, 3 and 1 rows: the candidates beyond the kept set are -inf entries in index order)"""
    img = S.build_image(cfg, q, seed=701)
    m = L.Transformer(img)
    n = 20 if form == "wide" else 6
    b = batch_of(L, m, form, n)
    rows = [FRow(L, img, i, flt=FILTERS[i % 8]) for i in range(n)]
    set_filters(b, rows)
    for i, r in enumerate(rows):
        r.prefill(b, S.prompt_tokens(cfg, PASS_DEPTHS[i % 8], 702 + i))
    toks = [(37 * i + 11) % V for i in range(n)]
    pos = [r.n for r in rows]
    am, lg = b.forward([r.slot for r in rows], toks, pos, logits=True)
    for i, r in enumerate(rows):
        what = f"{cfg} q{q} {form}: forward row {i} (filter {r.flt})"
        want = r.feed(toks[i])
        assert_bit_equal(lg[i], want, f"{what}: logits")
        assert int(am[i]) == ref_argmax(want) == ref_argmax(r.plain), f"{what}: the argmax is the unfiltered row's"
        if r.flt is None:
            assert_bit_equal(lg[i], r.plain, f"{what}: an unfiltered row beside filtered ones")
        elif 0 < r.flt[0] < V:
            assert (~np.isneginf(lg[i])).sum() <= r.flt[0], what
    cut = sum(int((np.isneginf(lg[i]) & ~np.isneginf(r.plain)).sum()) for i, r in enumerate(rows))
    assert cut > 3000 * sum(1 for r in rows if r.flt and r.flt[1] == INF), "the top_k rows cut nearly their whole vocabulary"
    runs = [[int(am[i]), (5 * i + 3) % V, (91 * i + 7) % V] for i in range(n)]
    start = [r.n for r in rows]
    am2, lg2, ti, tl = b.forward_runs([(r.slot, start[i], runs[i], 2) for i, r in enumerate(rows)], k=8, logits=True)
    o = 0
    for i, r in enumerate(rows):
        for j, t in enumerate(runs[i]):
            want = r.feed(t)
            if j == 0:
                continue
            what = f"{cfg} q{q} {form}: forward_runs slot {i} row {j} (output {o}, filter {r.flt})"
            assert_bit_equal(lg2[o], want, f"{what}: logits")
            assert int(am2[o]) == ref_argmax(want), what
            assert ti[o].tolist() == rank_row(want)[:8].tolist(), f"{what}: top-8 indices"
            # test_topk's rule over the candidates of the kept set (its ulp comparison has no meaning at -inf), and -inf exactly beyond it
            c = min(8, int((~np.isneginf(want)).sum()))
            assert c >= 1 and (c == min(8, r.flt[0]) if r.flt and r.flt[0] and r.flt[1] == INF else True), what      # (top_k alone: exactly top_k stay)
            with np.errstate(all="ignore"):
                topk_rule(tl[o:o + 1, :c], ti[o:o + 1, :c], want[None, :], what)
            assert np.isfinite(tl[o, :c]).all() and np.isneginf(tl[o, c:]).all(), f"{what}: log-probabilities beyond the kept set are -inf"
            o += 1
    assert o == 2 * n
    b.close()


# (temperature, top_p, seed): argmax, two sample_mult, the default flags' top-p, a peaked and a flat top-p.  mini-gemma's rows are peaked by themselves (a row's
# own input token leads by about 13), so its samplers run ten times hotter: the draws then reach beyond the first candidates, as mini-llama's do
SAMPLED_KINDS = {"mini-llama": [(0.0, 0.9, 1), (0.8, 1.0, 2), (1.5, 0.0, 3), (0.7, 0.9, 4), (0.25, 0.5, 7), (3.0, 0.999, 6)],
                 "mini-gemma": [(0.0, 0.9, 1), (8.0, 1.0, 2), (15.0, 0.0, 3), (7.0, 0.9, 4), (2.5, 0.5, 7), (30.0, 0.999, 6)]}
SAMPLED_FILTERS = [(5, INF), (5, INF), (0, 0.4), (5, INF), (2, 0.3), (5, INF), None, (40, 0.8)]
PEAKED_FILTER = (1, INF)            # a peaked sampler draws among the first few candidates: only top_k = 1 moves its tokens
SAMPLED_FORMS = [("mini-llama", S.Q8_0, "rows"), ("mini-llama", S.Q8_0, "wide"), ("mini-llama", S.Q8_0, "paged"), ("mini-gemma", S.Q4_0, "rows")]
SAMPLED_CALLS = 4


def sampled_scene(L, cfg, q, form):
    """the CPU side of test_sampled_passes_under_filters: the rows (oracles, samplers of both sides, filters), their prompts, and per call the row order, the
    tokens fed and the tokens the oracles' samplers draw from the filtered rows; every row counts the draws its filter moved (FRow.moved)"""
    img = S.build_image(cfg, q, seed=711)
    n = 20 if form == "wide" else 8
    rows = []
    for i in range(n):
        kind = SAMPLED_KINDS[cfg][i % 6]
        flt = SAMPLED_FILTERS[i % 8]
        rows.append(FRow(L, img, i, kind=kind, flt=PEAKED_FILTER if i % 6 == 4 and flt is not None else flt))
    prompts = [S.prompt_tokens(cfg, PASS_DEPTHS[i % 8], 712 + i) for i in range(n)]
    for r, p in zip(rows, prompts):
        for t in p:
            r.feed(t)
    last = [(53 * i + 29) % V for i in range(n)]
    calls = []
    for k in range(SAMPLED_CALLS):
        order = rows if k % 2 == 0 else rows[::-1]
        fed = [last[r.slot] for r in order]
        pos = [r.n for r in order]
        want = [r.choose(r.feed(last[r.slot])) for r in order]
        calls.append((order, fed, pos, want))
        for r, t in zip(order, want):
            last[r.slot] = t
    return img, rows, prompts, calls


@pytest.mark.parametrize("cfg,q,form", SAMPLED_FORMS)
def test_the_sampled_cases_are_not_vacuous(cfg, q, form):
    """on the CPU, before any device run: EVERY filtered row with a sampler other than argmax - sample_mult, the default, the peaked and the flat top-p
    alike - draws at least one token under its filter that the same sampler does not draw from the unfiltered row; unfiltered and argmax rows none"""
    import lmrs_amd
    img, rows, prompts, calls = sampled_scene(lmrs_amd, cfg, q, form)
    for r in rows:
        if r.flt is not None and r.kind[0] != 0.0:
            assert r.moved >= 1, f"{cfg} {form}: slot {r.slot} ({r.kind}, filter {r.flt}): the unfiltered oracle draws the same {SAMPLED_CALLS} tokens"
        else:
            assert r.moved == 0, (r.slot, r.kind, r.flt)
    assert {i % 6 for i, r in enumerate(rows) if r.flt is not None and r.moved} == {1, 2, 3, 4, 5}, "a sampler kind has no filtered row"


@gpu
@pytest.mark.parametrize("cfg,q,form", SAMPLED_FORMS)
def test_sampled_passes_under_filters(L, cfg, q, form):
    """forward_sample (up to 16 rows) and forward_runs_sample, every sampler kind over filtered and unfiltered slots, on mini-llama (contiguous, wide, paged)
    and on mini-gemma Q4_0 (the soft-cap, then the filter, then a sampler): each token is what the oracle's sampler draws from the filtered row - which
    test_the_sampled_cases_are_not_vacuous shows is not what it draws from the unfiltered one"""
    img, rows, prompts, calls = sampled_scene(L, cfg, q, form)
    m = L.Transformer(img)
    b = batch_of(L, m, form, len(rows))
    set_filters(b, rows)
    for r, p in zip(rows, prompts):
        if len(p):
            b.prefill(r.slot, p, 0)
    for k, (order, fed, pos, want) in enumerate(calls):
        if form == "wide" or k >= 2:
            got = b.forward_runs_sample([(r.slot, pos[i], [fed[i]], r.dev) for i, r in enumerate(order)])
        else:
            got = b.forward_sample([r.slot for r in order], fed, pos, [r.dev for r in order])
        assert got.tolist() == want, f"{cfg} {form} call {k}: tokens {got.tolist()} vs the oracle's {want}"
    b.close()


# a slab boundary inside the pass: the classifier runs a pass's output rows through the logits block sc_rows = min(512, 512 MiB / (4 * vocab_size)) rows at a
# time, and the filter's launch takes its column from the slab's first row on.  At the other tests' vocabulary (4096) one slab holds the 512 rows that are
# the most a pass takes; a vocabulary of 524 288 makes a slab 256 rows
SLAB_V, SLAB_ROWS, SLAB_RUNS, SLAB_LEN = 524288, 256, 45, 6


def first_candidates(row, k):
    """rank_row(row)[:k] without sorting half a million entries: the candidates at or above the k-th value in rank_row's order, then - where fewer than k
    entries are above -inf - the -inf entries by ascending index"""
    row = np.asarray(row, np.float32)
    top = np.flatnonzero(row >= np.partition(row, -k)[-k])                          # (every tie at the k-th value is in)
    if np.isneginf(row[top]).any():
        top = np.flatnonzero(~np.isneginf(row))
        top = np.concatenate((top, np.flatnonzero(np.isneginf(row))[:k]))
    return top[rank_row(row[top])][:k]


@gpu
def test_a_slab_boundary_inside_the_pass(L):
    """45 runs of 6 tokens, every row an output: 270 output rows, the boundary at output 256 inside slot 42's run.  Three calls: filtered slots on both sides
    of the boundary; a first slab without any filtered row; a second slab without one.  EVERY output row is judged by how many of its 8 candidates have a
    finite log-probability (top_k of them on a filtered slot, all 8 otherwise: a column read at the wrong offset, or a slab whose launch was skipped,
    shows), and the rows of four slots - the first, the one the boundary cuts, an unfiltered one and the last - against the oracle"""
    assert SLAB_RUNS * SLAB_LEN > SLAB_ROWS and (SLAB_ROWS // SLAB_LEN) * SLAB_LEN != SLAB_ROWS, "the boundary must fall inside a run"
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-v512k", vocab_size=SLAB_V)
    img = S.build_image(cfg, S.Q8_0, seed=761)
    m = L.Transformer(img); b = L.Batch(m, SLAB_RUNS, wide=True)
    rng = np.random.default_rng(762)
    toks = rng.integers(0, SLAB_V, (SLAB_RUNS, SLAB_LEN)).astype(np.uint32)
    cut = SLAB_ROWS // SLAB_LEN                                                      # slot 42: outputs 252 .. 257
    checked = [0, cut, cut + 1, SLAB_RUNS - 1]
    orc = O.Oracle(img)                                                              # one oracle, a sequence after the other from position 0
    plain = {s: [orc.forward(int(t), j).copy() for j, t in enumerate(toks[s])] for s in checked}
    runs = [(s, 0, toks[s].tolist(), SLAB_LEN) for s in range(SLAB_RUNS)]
    cases = [("filtered slots on both sides", {s: 3 for s in range(0, SLAB_RUNS, 2)}),
             ("no filtered row in the first slab", {cut + 1: 2, cut + 2: 5}),
             ("no filtered row in the second slab", {s: 2 for s in range(cut)})]
    for what, top_k in cases:
        b.clear_filters()
        b.set_filters(sorted(top_k), [top_k[s] for s in sorted(top_k)])
        first = {(s * SLAB_LEN + j) // SLAB_ROWS for s in top_k for j in range(SLAB_LEN)}
        assert first == {"filtered slots on both sides": {0, 1}, "no filtered row in the first slab": {1}, "no filtered row in the second slab": {0}}[what]
        am, ti, tl = b.forward_runs(runs, k=8)
        assert am.shape == (SLAB_RUNS * SLAB_LEN,)
        for s in range(SLAB_RUNS):
            for j in range(SLAB_LEN):
                o = s * SLAB_LEN + j
                assert int(np.isfinite(tl[o]).sum()) == top_k.get(s, 8) and np.isneginf(tl[o, top_k.get(s, 8):]).all(), \
                    f"{what}: output {o} (slot {s} row {j}, slab {o // SLAB_ROWS}, top_k {top_k.get(s)}): log-probabilities {tl[o]}"
        for s in checked:
            for j in range(SLAB_LEN):
                o = s * SLAB_LEN + j
                want = filtered(plain[s][j], top_k.get(s, 0))
                where = f"{what}: output {o} (slot {s} row {j}, slab {o // SLAB_ROWS}, top_k {top_k.get(s)})"
                c = top_k.get(s, 8)
                assert ti[o].tolist() == first_candidates(want, 8).tolist() and int(am[o]) == int(ti[o, 0]) == ref_argmax(plain[s][j]), where
                with np.errstate(all="ignore"):
                    topk_rule(tl[o:o + 1, :c], ti[o:o + 1, :c], want[None, :], where)
    b.close()


# ---------------------------------------------------------------------------------------------- 3. the order of the stages

@gpu
def test_penalties_then_the_mask_then_the_filter(L):
    cfg = "mini-gemma"
    img = S.build_image(cfg, S.Q4_0, seed=721)
    m = L.Transformer(img); b = L.Batch(m, 2)
    alpha = alphabet(722)
    seqs = [RecordSeq(img, 0), RecordSeq(img, 1)]
    seqs[0].par = params("all"); seqs[1].par = params("boost")
    for s in seqs:
        b.set_penalties([s.slot], **s.par)
    for s, d in zip(seqs, (9, 70)):
        p = from_alphabet(alpha, d, 723 + s.slot)
        b.prefill(s.slot, p, 0); s.feed(p)
    pos = [s.n for s in seqs]
    want = [s.want(int(alpha[3])) for s in seqs]
    # the ban-list holds the five first candidates of the PENALISED row: top_k = 5 behind the mask keeps the NEXT five, in front of it it would keep nothing
    masks = [ban(V, rank_row(pen)[:5].tolist() + [17]) for row, pen in want]
    b.set_masks([0, 1], np.stack(masks))
    b.set_filters([0, 1], [5, 0], [INF, 0.25])
    am, lg = b.forward([0, 1], [int(alpha[3])] * 2, pos, logits=True)
    for i, (row, pen) in enumerate(want):
        exp = filtered(masked(pen, masks[i]), *((5, INF), (0, 0.25))[i])
        assert_bit_equal(lg[i], exp, f"slot {i}: penalised -> masked -> filtered")
        assert int(am[i]) == ref_argmax(exp) == ref_argmax(masked(pen, masks[i])) != ref_argmax(pen)
        other = filtered(pen, *((5, INF), (0, 0.25))[i])
        assert not np.array_equal(np.isneginf(exp), np.isneginf(masked(other, masks[i]))), f"slot {i}: the case does not tell the orders apart"
    banned = set(rank_row(want[0][1])[:5].tolist()) | {17}
    assert np.flatnonzero(~np.isneginf(lg[0])).tolist() == sorted([t for t in rank_row(want[0][1]).tolist() if t not in banned][:5])
    b.close()


# ---------------------------------------------------------------------------------------------- 4. the device loops

LOOP_DEPTHS = [65, 0, 128, 63, 200]
LOOP_BUDGETS = [1, 2, 7, 12, 12]
LOOP_FIRSTS = [3, 400, 77, 1000, 21]
LOOP_FILTERS = [(5, INF), None, (5, INF), (0, 0.5), (4, 1.0)]
# generate: argmax and sample_mult rows; generate_topp: a flat and a default-flags top-p row among them
LOOP_KINDS = {"generate": [(0.9, 1.0, 31), None, (1.0, 1.0, 32), (0.0, 0.9, 33), (1.2, 0.0, 34)],
              "generate_topp": [(0.9, 1.0, 31), None, (1.0, 0.9, 32), (0.7, 0.9, 33), (1.2, 0.0, 34)]}


def loop_scene(L, call, img):
    """five fresh rows (oracles, samplers on both sides) with their continuations under the filters, stop sets from their own sequences"""
    cfg = "mini-llama"
    rows = [FRow(L, img, i, kind=LOOP_KINDS[call][i], flt=LOOP_FILTERS[i]) for i in range(5)]
    prompts = [S.prompt_tokens(cfg, LOOP_DEPTHS[i], 732 + i) for i in range(5)]
    for r, p in zip(rows, prompts):
        for t in p:
            r.feed(t)
    conts = [r.continuation(LOOP_FIRSTS[i], 12) for i, r in enumerate(rows)]
    outs = [c[0] for c in conts]
    stops = [[outs[0][0]], [], [outs[2][4]], [outs[3][9]], []]
    want = expect(rows, LOOP_FIRSTS, outs, LOOP_BUDGETS, stops)
    return rows, prompts, conts, stops, want


@pytest.mark.parametrize("call", ["generate", "generate_topp"])
def test_the_loop_cases_are_not_vacuous(call):
    """on the CPU, before any device run: rows end at different passes, both finish codes occur, and the sampled rows' tokens under their filters differ from
    what the same samplers draw from the unfiltered rows"""
    import lmrs_amd
    rows, prompts, conts, stops, want = loop_scene(lmrs_amd, call, S.build_image("mini-llama", S.Q8_0, seed=731))
    assert len({len(w[0]) for w in want}) >= 3 and {w[1] for w in want} == {BUDGET, STOP}, [(len(w[0]), w[1]) for w in want]
    assert any(rounds(len(w[0]), 3) - len(w[0]) >= 2 for w in want)
    for i in (0, 2, 4):
        assert rows[i].moved >= 1, f"row {i} ({rows[i].kind}, filter {rows[i].flt}): the filter moves no token"
    assert rows[1].moved == 0


@gpu
@pytest.mark.parametrize("call", ["generate", "generate_topp"])
def test_the_device_loops_under_filters(L, call):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=731)
    m = L.Transformer(img); b = L.Batch(m, 5)
    for ce in (1, 3, 64):
        what = f"{call} check_every {ce}"
        rows, prompts, conts, stops, want = loop_scene(L, call, img)
        set_filters(b, rows)
        for r, p in zip(rows, prompts):
            if len(p):
                b.prefill(r.slot, p, 0)
        got = getattr(b, call)([r.slot for r in rows], LOOP_FIRSTS, LOOP_DEPTHS, LOOP_BUDGETS, stop=stops, samplers=[r.dev for r in rows], check_every=ce,
                               logprobs=True)
        toks, fin, lps, stats = got
        n_out = [len(w[0]) for w in want]
        for i, (w, f) in enumerate(want):
            assert toks[i].tolist() == w, f"{what}: row {i} ({rows[i].kind}, filter {rows[i].flt}): tokens {toks[i].tolist()} vs {w}"
            assert int(fin[i]) == f, f"{what}: row {i}: finish {fin[i]} vs {f}"
            assert_within_one_ulp(lps[i], want_logprobs(conts[i][1][:n_out[i]], w), f"{what}: row {i}: log-probabilities over the kept set")
            rows[i].rewind(LOOP_DEPTHS[i] + n_out[i])
            check_slot_rows(b, rows[i], sorted({LOOP_DEPTHS[i], LOOP_DEPTHS[i] + n_out[i] - 1}), what)
        assert stats == dict(passes=max(rounds(k, ce) for k in n_out), row_passes=sum(rounds(k, ce) for k in n_out)), f"{what}: {stats}"
        # the top-p samplers' vectors: what a host sampler holds after the same filtered rows
        for i, r in enumerate(rows):
            if r.kind is not None and r.kind[0] != 0.0 and 0.0 < r.kind[1] < 1.0:
                host = L.Sampler(V, *r.kind)
                for row in conts[i][1][:n_out[i]]:
                    host.sample(row.copy())
                vec, ordered = r.dev.candidates()
                assert ordered and vec.tobytes() == host.candidates()[0].tobytes(), f"{what}: row {i}: the sampler's vector after the call"
    # generate_greedy skips the launch: the unfiltered tokens, which are the filtered rows' argmax as well
    rows, prompts, conts, stops, want = loop_scene(L, "generate", img)
    out = b.generate_greedy([r.slot for r in rows], LOOP_FIRSTS, LOOP_DEPTHS, 6)
    for i, r in enumerate(rows):
        r.rewind(LOOP_DEPTHS[i]); r.ref = None
        t, exp = LOOP_FIRSTS[i], []
        for _ in range(6):
            row = r.feed(t)
            assert ref_argmax(row) == ref_argmax(r.plain)
            t = ref_argmax(r.plain); exp.append(t)
        assert out[i].tolist() == exp, f"generate_greedy row {i}: {out[i].tolist()} vs {exp}"
    b.close()


# ---------------------------------------------------------------------------------------------- 5. state

@gpu
def test_filter_state(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=741)
    m = L.Transformer(img)
    b, fresh = L.Batch(m, 4, page_len=64, n_pages=12), L.Batch(m, 4)           # (paged: release is a paged batch's call)
    rows = [FRow(L, img, i) for i in range(3)]
    for r, d in zip(rows, (6, 3, 0)):
        p = S.prompt_tokens(cfg, d, 742 + r.slot)
        r.prefill(b, p)
        if d:
            fresh.prefill(r.slot, p, 0)

    def step(what, bits_of_fresh=False):
        pos = [r.n for r in rows]
        toks = [(11 * r.slot + 5 * pos[r.slot] + 1) % V for r in rows]
        am, lg = b.forward([0, 1, 2], toks, pos, logits=True)
        am0, lg0 = fresh.forward([0, 1, 2], toks, pos, logits=True)
        for i, r in enumerate(rows):
            want = r.feed(toks[i])
            assert_bit_equal(lg[i], want, f"{what}: slot {i} (filter {r.flt})")
            assert_bit_equal(lg0[i], r.plain, f"{what}: slot {i} of the batch that never had a filter")
            assert int(am[i]) == int(am0[i]) == ref_argmax(want)
            if bits_of_fresh:
                assert_bit_equal(lg[i], lg0[i], f"{what}: slot {i}: the bits of a fresh batch")

    assert b.filter_info(0) == dict(top_k=0, min_gap=float("inf"), active=False)
    step("no filter was ever set", bits_of_fresh=True)
    rows[0].flt, rows[1].flt = (5, INF), (0, 0.5)
    set_filters(b, rows)
    step("two slots filtered")
    rows[0].flt, rows[1].flt, rows[2].flt = (7, 0.75), None, (V, INF)                  # a replacement; (0, +inf) = clearing; top_k >= vocab: legal, inactive
    b.set_filters([0, 1, 2], [7, 0, V], [0.75, INF, INF])
    assert b.filter_info(0) == dict(top_k=7, min_gap=0.75, active=True)
    assert b.filter_info(1) == dict(top_k=0, min_gap=float("inf"), active=False)
    assert b.filter_info(2) == dict(top_k=V, min_gap=float("inf"), active=False)
    step("slot 0 replaced, slot 1 at (0, inf), slot 2 at top_k = vocab")
    # fork and release neither copy nor clear: slot 3 takes slot 0's rows and no filter; slot 0 released and prefilled again keeps its filter
    b.fork(0, 3, rows[0].n); fresh.fork(0, 3, rows[0].n)
    assert b.filter_info(3) == dict(top_k=0, min_gap=float("inf"), active=False) and b.filter_info(0)["active"]
    am, lg = b.forward([3], [9], [rows[0].n], logits=True)
    unf = rows[0].orc.forward(9, rows[0].n).copy()
    assert_bit_equal(lg[0], unf, "the fork's target has no filter")
    b.set_filters([3], 2); b.fork(0, 3, rows[0].n)
    assert b.filter_info(3) == dict(top_k=2, min_gap=float("inf"), active=True), "a fork into a filtered slot leaves its filter"
    am, lg = b.forward([3], [9], [rows[0].n], logits=True)
    assert_bit_equal(lg[0], filtered(unf, 2), "the fork's target keeps its own filter")
    b.release(0, rows[0].n)
    assert b.filter_info(0) == dict(top_k=7, min_gap=0.75, active=True), "release leaves the filter"
    step("after fork and release")
    b.clear_filters([0])
    rows[0].flt = None
    assert not b.filter_info(0)["active"] and b.filter_info(3)["active"]
    b.clear_filters()
    rows[2].flt = None
    assert not any(b.filter_info(i)["active"] for i in range(4))
    step("set and cleared all", bits_of_fresh=True)
    b.close(); fresh.close()


# ---------------------------------------------------------------------------------------------- 6. refusals

@gpu
def test_refusals_come_before_any_change_and_leave_everything_usable(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=751)
    m = L.Transformer(img); b = L.Batch(m, 3)
    lib = L.lib()
    rows = [FRow(L, img, i) for i in range(3)]
    rows[1].flt = (5, 1.5)
    set_filters(b, rows)
    info1 = b.filter_info(1)

    def valid(what):
        pos = [r.n for r in rows]
        toks = [(7 * pos[i] + i + 2) % V for i in range(3)]
        am, lg = b.forward([0, 1, 2], toks, pos, logits=True)
        for i, r in enumerate(rows):
            assert_bit_equal(lg[i], r.feed(toks[i]), f"{what}: slot {i}")
        assert b.filter_info(1) == info1 and not b.filter_info(0)["active"] and not b.filter_info(2)["active"], what

    u32 = lambda *v: np.array(v, np.uint32)
    f32 = lambda *v: np.array(v, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    k17, g17, s17 = np.full(17, 3, np.uint32), np.full(17, 1.0, np.float32), np.arange(17, dtype=np.uint32)
    sf = lambda n, slot, k=k17, g=g17: lib.lmrs_batch_set_filters(b._h, n, p(slot), p(k), p(g))
    ui, fl, ii = ctypes.c_uint32(), ctypes.c_float(), ctypes.c_int()
    R = ctypes.byref
    valid("first")
    cases = [
        (lambda: lib.lmrs_batch_set_filters(None, 1, p(u32(0)), p(k17), p(g17)), "lmrs_batch_set_filters: NULL argument"),
        (lambda: sf(1, None), "lmrs_batch_set_filters: NULL array"),
        (lambda: sf(1, u32(0), k=None), "lmrs_batch_set_filters: NULL array"),
        (lambda: sf(1, u32(0), g=None), "lmrs_batch_set_filters: NULL array"),
        (lambda: sf(17, s17), "lmrs_batch_set_filters: n = 17 exceeds the batch's width of 16"),
        (lambda: sf(2, u32(0, 3)), "lmrs_batch_set_filters: filter 1: slot 3 of 3"),
        (lambda: sf(2, u32(2, 2)), "lmrs_batch_set_filters: slot 2 appears twice"),
        (lambda: sf(2, u32(0, 2), g=f32(1.0, np.nan)), "lmrs_batch_set_filters: filter 1: slot 2: min_gap is NaN"),
        (lambda: sf(2, u32(0, 2), g=f32(-0.5, 1.0)), "lmrs_batch_set_filters: filter 0: slot 0: min_gap = -0.500000 is negative"),
        (lambda: sf(2, u32(0, 2), g=f32(1.0, -np.inf)), "lmrs_batch_set_filters: filter 1: slot 2: min_gap = -inf is negative"),
        (lambda: lib.lmrs_batch_clear_filters(None, 0, None), "lmrs_batch_clear_filters: NULL argument"),
        (lambda: lib.lmrs_batch_clear_filters(b._h, 1, None), "lmrs_batch_clear_filters: NULL array"),
        (lambda: lib.lmrs_batch_clear_filters(b._h, 17, p(s17)), "lmrs_batch_clear_filters: n = 17 exceeds the batch's width of 16"),
        (lambda: lib.lmrs_batch_clear_filters(b._h, 1, p(u32(3))), "lmrs_batch_clear_filters: filter 0: slot 3 of 3"),
        (lambda: lib.lmrs_batch_clear_filters(b._h, 2, p(u32(1, 1))), "lmrs_batch_clear_filters: slot 1 appears twice"),
        (lambda: lib.lmrs_batch_filter_info(None, 0, R(ui), R(fl), R(ii)), "lmrs_batch_filter_info: NULL argument"),
        (lambda: lib.lmrs_batch_filter_info(b._h, 0, R(ui), R(fl), None), "lmrs_batch_filter_info: NULL argument"),
        (lambda: lib.lmrs_batch_filter_info(b._h, 3, R(ui), R(fl), R(ii)), "lmrs_batch_filter_info: slot 3 of 3"),
    ]
    for fn, msg in cases:
        assert fn() != 0, msg
        assert lib.lmrs_last_error().decode().startswith(msg), (msg, lib.lmrs_last_error().decode())
        valid(f"after {msg!r}")
    with pytest.raises(L.LmrsError, match="top_k must be a scalar or hold one value per slot"):
        b.set_filters([0, 1], top_k=[1, 2, 3])
    valid("last")
    b.close()


@gpu
def test_a_vocabulary_with_an_unwritten_tail_has_no_filters(L):
    """vocabulary 4098 (Q8_0): the classifier writes 4096 of the 4098 logits - set_masks and set_penalties refuse such a batch and so does set_filters"""
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-v4098", vocab_size=4098)
    img = S.build_image(cfg, S.Q8_0, seed=755)
    m = L.Transformer(img); b = L.Batch(m, 2)
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_set_filters: the classifier leaves the last vocab_size % 4 logits unwritten"):
        b.set_filters([0], top_k=5)
    assert not b.filter_info(0)["active"]
    s = TokenSeq(img, 0)
    am, lg = b.forward([0], [5], [0], logits=True)
    assert_bit_equal(lg[0], s.feed([5]), "slot 0 after the refusal")
    b.close()
