"""Q8 and Q4 page pools (lmrs_batch_create_paged_q8 / _q4, lm.rs_amd/csrc/lmrs_kvq.inc, lmrs_kv4.inc) where the four standing modules - page_len 64,
at most 400 positions, forward and prefill only - do not reach: pages of 256 and 1024 positions, where a 64-key chunk is no longer a page and every
`& (PL - 1)` and every stride by PL counts; rows beyond 256 keys for every head size; prefills of more than one 512-row chunk; block attention that
starts inside a page; ragged passes (forward_runs), whose later rows read the earlier rows of the same launch back quantised; more than 16 rows a pass;
copy on write into a shared page, release and rewrite, the context's import across long pages; the device loop across deep page edges; the stress
recipes; Gemma-2's 4096-key window; pages above 2^32 bytes of a pool.  It is what tests/test_batch_paged_deep.py and tests/test_batch_stress.py ask of
the f32 pool.

The reference is the round-trip witness of tests/kvpool_rules.py.  Every comparison - logits, argmax, K/V rows - is bit for bit; a position nobody
wrote or that was released is compared numerically with zero (an all-zero Q4 page reads back as -0.0).  No tolerances.  The route of every prefill is
asserted through prefill_form against the documented floors, 256 rows (Q8) and 320 rows (Q4)."""
import dataclasses
import functools

import numpy as np
import pytest

import deep_rules
import oracle_lib as O
import stress_models as SM
from kvpool_rules import (BRANCH_EDGE, BRANCH_FROM, DEEP, FLOOR, FORMATS, QSEQ, ROUND_TRIP, Ref, WSeq, assert_reads_zero, expected_form, kv_rows,
                          pages_of, prefill, qbatch, stats_run, witness)
from parity_rules import assert_bit_equal, ref_argmax, run_positions
from test_batch import check_slot_rows, snapshot, step
from test_batch_embed import random_rows
from test_batch_kvq import CLASSES as SHORT
from test_batch_paged_deep import D, N, N_NEW, SEED, STEPS, check_ref_rows, reference, ref_steps
from test_batch_runs import FORMS as RUN_FORMS, run_pass
from test_batch_stress import BLOCK_ROWS, D16, STEPS as STRESS_STEPS, step_positions, summed
from test_stress_regimes import SEED as STRESS_SEED, check_witness
from tools import synth_lmrs as S

pytestmark = pytest.mark.gpu

PAGE_LENS = [64, 256, 1024]                                 # 64: the control, where the standing behaviour must hold on the same inputs
ident = lambda v: {S.Q8_0: "w8", S.Q4_0: "w4"}.get(v) if isinstance(v, int) and not isinstance(v, bool) and v in (S.Q8_0, S.Q4_0) else None


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


# ---------------------------------------------------------------------------------------------- A. page lengths, rows at every pass edge

def prefilled(L, ref, fmt, page_len, n_slots):
    """slot i holds toks[:D[i]], one prefill call each: above 512 rows two chunks, the second a block chunk where it reaches the floor"""
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, n_slots)
    for i, d in enumerate(D):
        if d:
            prefill(b, fmt, i, ref.toks[:d])
    return m, b


@pytest.mark.parametrize("page_len", PAGE_LENS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q", DEEP, ids=ident)
def test_prefilled_rows_at_every_pass_edge(L, cfg, q, fmt, page_len):
    """16 slots at the depths of test_batch_paged_deep.D - the 256 / 512 / 768 score-pass edges, the 319 / 320 V-chunk edge, three steps that end at
    the last position -: page accounting, K/V rows, three decode passes of all 16 rows"""
    ref = witness(cfg, q, fmt)
    what = f"{cfg} q{q} {fmt} pages of {page_len}"
    # two chunks above 512 rows; the second one is a block chunk from 768 (Q8) / 832 (Q4) rows on, a table chunk that reads the first one's pages below
    assert expected_form(fmt, 1021) == (2, 2) and expected_form(fmt, 767) == (2, 1) and expected_form(fmt, 769) == (2, 2 if fmt == "q8" else 1)
    m, b = prefilled(L, ref, fmt, page_len, 16)
    for i, d in enumerate(D):
        assert b.slot_pages(i) == (pages_of(d, page_len), 0), f"{what}: slot {i} after a prefill of {d}"
    n_pages = b.pages()[1]
    assert b.pages() == (page_len, n_pages, n_pages - sum(pages_of(d, page_len) for d in D))
    for i, d in enumerate(D):
        at = {0, d // 2, d - 1} | ({511, 512} if d > 512 else set()) if d else set()
        check_ref_rows(b, ref, i, sorted(at), f"{what}: prefill of {d}")
    assert_reads_zero(b, D.index(3), ref.cfg.n_layers, [3, page_len - 1], f"{what}: behind a prefill of 3")
    ref_steps(b, ref, list(range(16)), D, f"{what}: the 16-row table")
    assert b.pages()[2] == n_pages - sum(pages_of(min(d + STEPS, N), page_len) for d in D)


@pytest.mark.parametrize("page_len", PAGE_LENS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q", DEEP, ids=ident)
def test_prefilled_rows_in_a_20_row_pass(L, cfg, q, fmt, page_len):
    """the same rows through the long table: four more slots are forks of the slots at 257, 513, 769 and 1000"""
    ref = witness(cfg, q, fmt)
    what = f"{cfg} q{q} {fmt} pages of {page_len}"
    m, b = prefilled(L, ref, fmt, page_len, 20)
    extra = [257, 513, 769, 1000]
    for j, d in enumerate(extra):
        b.fork(D.index(d), 16 + j, d)
        for s in (D.index(d), 16 + j):
            assert b.slot_pages(s) == (pages_of(d, page_len), d // page_len), f"{what}: slot {s} after the fork at {d}"
        check_ref_rows(b, ref, 16 + j, [0, d // 2, d - 1], f"{what}: the fork at {d}")
    ref_steps(b, ref, list(range(20)), D + extra, f"{what}: the long table")


# ---------------------------------------------------------------------------------------------- B. block attention off the page grid

def plans(fmt):
    """tests/test_batch_kv4_block.py's plans at the format's floor f: f / 64 whole blocks | one more block of one row | a start inside a page and a key
    chunk behind a table-pass call | a start on a 64-key edge, the end one past a chunk edge.  Then a table chunk, a full 512-row block chunk that starts
    inside a page of every length, and a short table chunk behind it that reads both: [f - 20, 512, 200] - at Q4 the [300, 512, 200] of 1012 rows; at
    Q8, whose floor 300 rows exceed, the first chunk is 236 rows so that it stays the table chunk it is there to be."""
    f = FLOOR[fmt]
    return {"at the floor": [[f], [f + 1], [70, f], [64, f + 1]], "three chunks": [[f - 20, 512, 200]]}


def plan_rows(plan):
    """The rows of a plan that are read back.  A row of layer 1 witnesses its own query's attention in layer 0, so the rows are spread over every
    query block: both rows at each end of every chunk, the first and last row of every 64-position stretch (the edges of key chunks, of query blocks
    that start on the grid, and of pages), and every 7th row between - 7 and 64 are coprime, so over the blocks of a plan every lane of a block is read.
    (Every row of every plan was read at first: a K row costs a strided copy of kv_dim / 16 pieces, and the 32 cases took 65 s of the module's 133
    against the f32 twin's 49; a fifth of the rows keeps the module under twice its twin.  The stride mutations the module was proven on change
    nearly every row behind the first key group, and fail this list as they failed every row.)"""
    rows, at = set(), 0
    for n in plan:
        rows |= {at, at + 1, at + n - 2, at + n - 1}
        at += n
    return sorted(rows | {p for p in range(at) if p % 64 in (0, 63) or p % 7 == 0})


@pytest.mark.parametrize("which", ["at the floor", "three chunks"])
@pytest.mark.parametrize("page_len", [256, 1024])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q", DEEP, ids=ident)
def test_block_attention_off_the_page_grid(L, cfg, q, fmt, page_len, which):
    """every plan in a slot of its own: the slot's K/V rows (plan_rows) against the witness, then one decode pass over the slots, which reads them all"""
    ref = witness(cfg, q, fmt)
    what = f"{cfg} q{q} {fmt} pages of {page_len}"
    f = FLOOR[fmt]
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, len(plans(fmt)[which]))
    seqs = []
    for slot, plan in enumerate(plans(fmt)[which]):
        at = 0
        for n in plan:
            assert expected_form(fmt, n) == (1, 1 if n >= f else 0) and at + n <= 1012
            prefill(b, fmt, slot, ref.toks[at:at + n], at)
            at += n
        assert b.slot_pages(slot) == (pages_of(at, page_len), 0)
        seqs.append(WSeq(ref, slot, at))
        check_slot_rows(b, seqs[-1], plan_rows(plan), f"{what}: {plan}")
    step(b, seqs, [s.next()[0] for s in seqs], f"{what}: the decode pass behind the prefills")


# (class, format, embedding rows): one class per format on token rows, and one prefill_embeddings case
ROUTES = [("mini-llama3b-1k", S.Q8_0, "q8", False), ("mini-gemma-1k", S.Q4_0, "q4", False), ("mini-phi-long", S.Q8_0, "q4", True)]


@pytest.mark.parametrize("cfg,q,fmt,embed", ROUTES, ids=ident)
def test_block_route_equals_the_table_pass_on_256_position_pages(L, cfg, q, fmt, embed):
    """slot 0 by the library's rule, slot 1 forced to the table pass, the same 70 + (floor + 10) rows: the block chunk starts inside page 0 and ends
    inside page 1.  Every K/V row and one decode step's logits are equal; token rows are the witness's too"""
    ref = witness(cfg, q, fmt)
    f, page_len = FLOOR[fmt], 256
    n = 70 + f + 10
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, 2)
    rows = random_rows(n, m.args.dim, SEED + 3) if embed else None
    for slot in (0, 1):
        b.debug_prefill_table(slot == 1)
        for at, k in ((0, 70), (70, f + 10)):
            assert b.prefill_form(k, at) == (1, 1 if k >= f and slot == 0 else 0), f"{cfg} {fmt}: prefill_form({k}, {at}), slot {slot}"
            if embed:
                assert b.prefill_embeddings(slot, rows[at:at + k], at) == at + k
            else:
                assert b.prefill(slot, ref.toks[at:at + k], at) == at + k
    b.debug_prefill_table(False)
    nl = ref.cfg.n_layers
    for x, y in zip(snapshot(b, 0, range(n), nl), snapshot(b, 1, range(n), nl)):
        assert_bit_equal(x, y, f"{cfg} {fmt}: a K/V row, block against table")
    am, lg = b.forward([0, 1], [int(ref.toks[n])] * 2, [n, n], logits=True)
    assert_bit_equal(lg[0], lg[1], f"{cfg} {fmt}: the decode step's logits, block against table")
    if not embed:
        check_ref_rows(b, ref, 1, range(n), f"{cfg} {fmt}: the table pass")
        assert_bit_equal(lg[0], ref.logits[n], f"{cfg} {fmt}: the decode step against the witness")


# ---------------------------------------------------------------------------------------------- C. ragged passes

def standing(b, fmt, ref, depths):
    """slot i holds toks[:depths[i]] -> one WSeq each"""
    for i, d in enumerate(depths):
        if d:
            prefill(b, fmt, i, ref.toks[:d])
    return [WSeq(ref, i, d) for i, d in enumerate(depths)]


@pytest.mark.parametrize("page_len", [64, 128])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q", SHORT, ids=ident)
def test_mixed_runs_on_quantised_pages(L, cfg, q, fmt, page_len):
    """tests/test_batch_runs.py::test_mixed_runs_in_a_skinny_pass on a quantised pool: runs of 1, 4, 1, 7 and 3 on slots standing at 65, 0, 128, 61 and
    252.  One launch scatters every row of a run; a later row of the run must read the earlier ones back quantised and take its own key and value in
    f32, which is what the sequential witness does.  The 7-row run covers 61 .. 67: it crosses a 64-key chunk and, at page_len 64, a page edge"""
    ref = witness(cfg, q, fmt, 256)
    what = f"{cfg} q{q} {fmt} pages of {page_len}"
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, 5)
    seqs = standing(b, fmt, ref, [65, 0, 128, 61, 252])
    run_pass(b, [(s, s.next(n), n) for s, n in zip(seqs, [1, 4, 1, 7, 3])], f"{what}: first pass")
    assert [s.n for s in seqs] == [66, 4, 129, 68, 255]
    assert [b.slot_pages(s.slot)[0] for s in seqs] == [pages_of(s.n, page_len) for s in seqs]
    run_pass(b, [(s, s.next(n), n) for s, n in zip(seqs, [3, 1, 2, 1, 1])], f"{what}: second pass")


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_multi_tile_ragged_pass(L, fmt):
    """R = 130 rows (tests/test_batch_runs.py's FORMS): a 70-row run from position 0 whose rows all see each other through one launch's pages"""
    cfg, q, page_len = "mini-llama", S.Q8_0, 64
    ref = witness(cfg, q, fmt, 256)
    lens, starts = RUN_FORMS[130], [0, 63, 64, 5, 100]
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, 5)
    seqs = standing(b, fmt, ref, starts)
    n_out = [(n, 0, 1, n, 1)[i] for i, n in enumerate(lens)]
    run_pass(b, [(s, s.next(n), no) for s, n, no in zip(seqs, lens, n_out)], f"{cfg} {fmt} R 130")
    check_slot_rows(b, seqs[0], [63, 64, 65], f"{cfg} {fmt} R 130: across the page edge")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q", DEEP, ids=ident)
def test_runs_across_a_score_pass_and_a_256_position_page_edge(L, cfg, q, fmt):
    """page_len 256: a 9-row run from 250 crosses the 256-key score pass and the page edge inside one launch; beside it a run across 512, one that
    ends at the last position, and one on an empty slot"""
    ref = witness(cfg, q, fmt)
    what = f"{cfg} q{q} {fmt} pages of 256"
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, 256, 4)
    seqs = standing(b, fmt, ref, [250, 508, 0, 1019])
    run_pass(b, [(s, s.next(n), n) for s, n in zip(seqs, [9, 9, 3, 5])], what)
    assert [b.slot_pages(s.slot) for s in seqs] == [(2, 0), (3, 0), (1, 0), (4, 0)]
    step(b, seqs[:3], [s.next()[0] for s in seqs[:3]], f"{what}: the decode pass behind the runs")


# ---------------------------------------------------------------------------------------------- D. copy on write, release, the context fork, the device loop

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q", [("mini-llama-1k", S.Q8_0), ("mini-gemma-1k", S.Q4_0)], ids=ident)
def test_unshare_release_and_context_fork_on_256_position_pages(L, cfg, q, fmt):
    """tests/test_batch_paged_deep.py's test of that name on a quantised pool: the whole-page copy of a write into a shared page is sized by the
    quantised page (pages_enqueue), release gives quantised pages back and they are written again, and the context's f32 cache is imported -
    quantised on the way - across 256-position pages"""
    ref = witness(cfg, q, fmt)
    what = f"{cfg} q{q} {fmt}"
    PL, n_pages = 256, 12
    nl = ref.cfg.n_layers
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, PL, 4, n_pages)
    # --- fork and un-share
    prefill(b, fmt, 0, ref.toks[:700])
    b.fork(0, 1, 700); b.fork(0, 2, 700)
    for s in range(3):
        assert b.slot_pages(s) == (3, 2), f"{what}: slot {s} after the forks"
    assert b.pages() == (PL, n_pages, n_pages - 5)
    at = [0, 255, 256, 299, 300, 309, 310, 511, 512, 699]
    before = {s: snapshot(b, s, at, nl) for s in (0, 2)}
    other = S.prompt_tokens(ref.cfg, 10, SEED + 1)
    prefill(b, fmt, 1, other, 300)                            # into the shared page 1: a whole-page copy first
    for s in (0, 2):
        for x, y in zip(before[s], snapshot(b, s, at, nl)):
            assert_bit_equal(x, y, f"{what}: slot {s} moved by slot 1's write into a shared page")
        check_ref_rows(b, ref, s, at, f"{what}: slot {s} beside slot 1's write")
    s1 = QSEQ[fmt](ref.img, 1)
    s1.feed(ref.toks[:300]); s1.feed(other)
    check_slot_rows(b, s1, range(300, 310), f"{what}: slot 1's own rows")
    check_ref_rows(b, ref, 1, [0, 255, 256, 299, 310, 511, 512, 699], f"{what}: the rows the page copy kept")
    assert b.slot_pages(1) == (3, 1) and b.slot_pages(0) == (3, 2) and b.slot_pages(2) == (3, 2) and b.pages()[2] == n_pages - 6
    step(b, [s1], [int(ref.toks[310])], f"{what}: slot 1 at 310, behind its write")
    # --- release
    keep = [0, 299, 300, 511]
    kept = snapshot(b, 2, keep, nl)
    b.release(2, 300)
    assert b.slot_pages(2) == (2, 2) and b.pages()[2] == n_pages - 5, "release(slot, 300) keeps two pages of 256 positions"
    for x, y in zip(kept, snapshot(b, 2, keep, nl)):
        assert_bit_equal(x, y, f"{what}: a kept position moved by the release")
    assert_reads_zero(b, 2, nl, [512, 699], f"{what}: a released position")
    prefill(b, fmt, 2, ref.toks[512:600], 512)
    assert b.slot_pages(2) == (3, 2)
    check_ref_rows(b, ref, 2, range(512, 600), f"{what}: rows 512 .. 599 written again")
    assert_reads_zero(b, 2, nl, [600, 699], f"{what}: behind the rewritten rows, in a page that was released and claimed again")
    am, lg = b.forward([2], [int(ref.toks[600])], [600], logits=True)
    assert_bit_equal(lg[0], ref.logits[600], f"{what}: the step at 600 after release and prefill")
    assert int(am[0]) == ref_argmax(ref.logits[600])
    check_ref_rows(b, ref, 2, [600], f"{what}: the row that step wrote")
    # --- fork from the context's own (contiguous, f32) cache: every row is quantised on the way in.  The context computed its rows over f32
    # keys, so from layer 1 on they are not the witness's: the step behind the fork is judged by a QSeq whose cache holds the round trip of the f32
    # oracle's rows (test_batch_paged_deep.reference, the same image and tokens), which is what the import must have left
    f32 = reference(cfg, q)
    assert f32.toks.tolist() == ref.toks.tolist()
    assert m.prefill_tokens(ref.toks[:700], 0) == 700
    free = b.pages()[2]
    b.fork(L.BATCH_CTX, 3, 700)
    assert b.slot_pages(3) == (3, 0) and b.pages()[2] == free - 3
    rt = ROUND_TRIP[fmt]
    for layer in range(nl):
        for p in (0, 255, 256, 511, 512, 699):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(3, w, layer, p), rt(m.kv_row(w, layer, p)), f"{what}: fork from the context, {'kv'[w]} layer {layer} pos {p}")
                assert_bit_equal(b.kv_row(3, w, layer, p), rt((f32.K, f32.V)[w][layer, p]), f"{what}: fork from the context against the oracle, {'kv'[w]} layer {layer} pos {p}")
    assert_reads_zero(b, 3, nl, [700], f"{what}: behind the forked rows")
    s3 = QSEQ[fmt](ref.img, 3)
    a = s3.orc.args
    for layer in range(nl):
        for w in (0, 1):
            for p in range(700):
                row = np.ctypeslib.as_array(O.lib().lmrs_ref_kv(s3.orc.h, w, layer, p), shape=(a.n_kv_heads * a.head_size,))
                row[:] = rt((f32.K, f32.V)[w][layer, p])
    s3.n = 700
    step(b, [s3], [int(ref.toks[700])], f"{what}: the step at 700 on the context's fork")


@pytest.mark.parametrize("n_rows", [4, 20])
@pytest.mark.parametrize("page_len", [64, 256])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q", DEEP, ids=ident)
def test_device_loop_across_deep_page_edges(L, cfg, q, fmt, page_len, n_rows):
    """generate_greedy of 12 steps from 250, 505 and 760: across the 256-key passes' edges at 256, 512 and 768, page edges of both lengths.  Rows cycle
    through the three starts; the first slot of a start is prefilled, the others are forks of it - equal rows.  Tokens against the witness's greedy
    branches, and the rows the loop left at both sides of the edges"""
    ref = witness(cfg, q, fmt)
    what = f"{cfg} q{q} {fmt} pages of {page_len}, {n_rows} rows"
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, n_rows)
    depth = [BRANCH_FROM[i % 3] for i in range(n_rows)]
    for i, d in enumerate(depth):
        if i < 3:
            prefill(b, fmt, i, ref.toks[:d])
        else:
            b.fork(i % 3, i, d)
    out = b.generate_greedy(list(range(n_rows)), [int(ref.toks[d]) for d in depth], depth, N_NEW)
    assert out.shape == (n_rows, N_NEW)
    for i, d in enumerate(depth):
        assert out[i].tolist() == ref.branch[d], f"{what}: row {i} (from {d})"
        assert b.slot_pages(i)[0] == pages_of(d + N_NEW, page_len), f"{what}: slot {i} after the loop"
    for s in sorted({0, 1, 2, n_rows - 3, n_rows - 2, n_rows - 1}):
        d = depth[s]
        for layer in range(ref.cfg.n_layers):
            for p in (d, BRANCH_EDGE[d] - 1, BRANCH_EDGE[d], d + N_NEW - 1):
                for w in (0, 1):
                    assert_bit_equal(b.kv_row(s, w, layer, p), ref.brows[d][w][layer, p - d], f"{what}: slot {s} {'kv'[w]} layer {layer} pos {p} left by the loop")


# ---------------------------------------------------------------------------------------------- E. stress recipes

N_STRESS = 7 + 320 + 2                                        # the Q4 block case: 7 rows, the floor's 320 behind them, two steps
STRESS = [("mini-llama", S.Q8_0, "peaked"), ("mini-llama", S.Q8_0, "outliers"), ("mini-llama", S.Q8_0, "combined"), ("mini-gemma", S.Q4_0, "softcap")]


@functools.lru_cache(maxsize=None)
def stress_run(cfg, q, recipe, fmt):
    """tests/test_batch_stress.py's oracle_run on a quantised cache: one QSeq run of 329 positions on the recipe's image - the class's cache extended to
    512 positions, which the block case needs - with the regime counters of every single position"""
    c = dataclasses.replace(S.CONFIGS[cfg], name=cfg + "-512", max_pos=512)
    img, c = SM.build(c, recipe, q, STRESS_SEED)
    return stats_run(img, c, fmt, N_STRESS, STRESS_SEED)


def reached(cfg, q, recipe, fmt, positions):
    """the recipe's witness (test_stress_regimes.check_witness) over exactly the positions a case compares, on the quantised run's own counters: what
    tests/test_batch_stress.py::test_every_gpu_case_compares_rows_that_reached_the_regime asks of an f32 case, asked here before the device is touched"""
    ref, stats = stress_run(cfg, q, recipe, fmt)
    pos = sorted(set(int(p) for p in positions))
    assert pos and 0 <= pos[0] and pos[-1] < N_STRESS
    check_witness(recipe, ref.cfg, q, summed(stats[p] for p in pos), ref.logits[pos], len(pos))
    return ref


@pytest.mark.parametrize("page_len", [64, 256])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q,recipe", STRESS, ids=ident)
def test_stress_recipes_through_the_table_pass(L, cfg, q, recipe, fmt, page_len):
    """tests/test_batch_stress.py::test_paged_table_pass's positions: 16 slots at D16, the odd ones forks of one prefilled slot, the even ones prefilled
    in two chunks, then three passes.  `outliers` leaves groups whose nibbles are all but one the zero nibble; `peaked` one-hot softmax rows, where a
    single wrong key changes the result"""
    ref = reached(cfg, q, recipe, fmt, step_positions(D16))
    what = f"{ref.cfg.name} q{q} {recipe} {fmt} pages of {page_len}"
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, 17)
    top = max(D16) + STRESS_STEPS
    prefill(b, fmt, 16, ref.toks[:top])
    seqs = []
    for i, d in enumerate(D16):
        if d and i % 2:
            b.fork(16, i, d)
        elif d // 2:
            prefill(b, fmt, i, ref.toks[:d // 2]); prefill(b, fmt, i, ref.toks[d // 2:d], d // 2)
        elif d:
            prefill(b, fmt, i, ref.toks[:d])
        seqs.append(WSeq(ref, i, d))
        check_slot_rows(b, seqs[-1], sorted({0, d // 2, d - 1}) if d else [], f"{what}: slot {i} made at depth {d}")
    assert b.slot_pages(11) == (pages_of(128, page_len), 128 // page_len), f"{what}: the fork at 128"
    for k in range(STRESS_STEPS):
        step(b, seqs, [s.next()[0] for s in seqs], f"{what} step {k}")


def stress_block_positions(fmt):
    f = FLOOR[fmt]
    return [7, 7 + f // 2, 7 + f - 1, 7 + f, 7 + f + 1]


@pytest.mark.parametrize("page_len", [64, 256])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cfg,q,recipe", STRESS, ids=ident)
def test_stress_recipes_through_block_attention(L, cfg, q, recipe, fmt, page_len):
    """tests/test_batch_stress.py::test_paged_block_attention at the format's floor: the floor's rows in one block chunk behind a 7-token prefill, K/V rows
    at its first, middle and last position, then two passes on that cache and on a fork of it; and the same rows forced through the table pass"""
    ref = reached(cfg, q, recipe, fmt, stress_block_positions(fmt))
    what = f"{ref.cfg.name} q{q} {recipe} {fmt} pages of {page_len} block"
    f = FLOOR[fmt]
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, 3)
    for slot in (0, 2):
        b.debug_prefill_table(slot == 2)
        prefill(b, fmt, slot, ref.toks[:7])
        prefill(b, fmt, slot, ref.toks[7:7 + f], 7, forced_table=slot == 2)
    b.debug_prefill_table(False)
    b.fork(0, 1, 7 + f)
    seqs = [WSeq(ref, i, 7 + f) for i in range(3)]
    for s in seqs:
        check_slot_rows(b, s, stress_block_positions(fmt)[:3] + BLOCK_ROWS, what)
    for k in range(2):
        step(b, seqs, [s.next()[0] for s in seqs], f"{what} step {k}")


# ---------------------------------------------------------------------------------------------- F. Gemma-2's window

N_WINDOW = 4360
WINDOW_STEPS = [p for p in deep_rules.GEMMA_WINDOW if p >= 4100]
assert WINDOW_STEPS == [4223, 4224, 4351, 4352]


@functools.lru_cache(maxsize=None)
def window_witness(fmt):
    """one QSeq run of 4360 positions on deep_rules.config("mini-gemma") - one layer, 8192 positions -: logits of the positions stepped, every K/V row"""
    cfg = deep_rules.config("mini-gemma")
    img = S.build_image(cfg, S.Q8_0, seed=deep_rules.SEED)
    toks = S.prompt_tokens(cfg, N_WINDOW, deep_rules.SEED)
    keep = set(range(4100, 4109)) | set(WINDOW_STEPS)
    seq, logits = QSEQ[fmt](img, 0), {}
    for p, t in enumerate(toks):
        lg = seq.feed([t])
        if p in keep:
            logits[p] = lg
    K, V = kv_rows(seq.orc, cfg.n_layers, range(N_WINDOW))
    for a in (toks, K, V):
        a.setflags(write=False)
    return Ref(cfg, img, toks, logits, K, V, {}, {})


@pytest.mark.parametrize("page_len", [64, 1024])
@pytest.mark.parametrize("fmt", FORMATS)
def test_gemma_window_on_quantised_pages(L, fmt, page_len):
    """one prefill of 4100 tokens - eight block chunks and a table chunk of 4 rows - and the same under debug_prefill_table: from 4097 keys on the window
    masks keys 0 .. pos - 4097.  Steps 4100 .. 4108, then - prefilling on - at 4223 | 4224 (the first 128-key value chunk wholly behind the window) and
    4351 | 4352 (the first 256-key score chunk)"""
    ref = window_witness(fmt)
    what = f"mini-gemma window {fmt} pages of {page_len}"
    m = L.Transformer(ref.img)
    b = qbatch(L, m, fmt, page_len, 2, 2 * pages_of(N_WINDOW, page_len))
    assert expected_form(fmt, 4100) == (9, 8)
    for slot in (0, 1):
        b.debug_prefill_table(slot == 1)
        prefill(b, fmt, slot, ref.toks[:4100], forced_table=slot == 1)
        assert b.slot_pages(slot) == (pages_of(4100, page_len), 0)
    seqs = [WSeq(ref, 0, 4100), WSeq(ref, 1, 4100)]
    for s in seqs:
        check_slot_rows(b, s, [p for p in deep_rules.CACHE_AT if p < 4100] + [4099], what)

    def steps(n):
        for _ in range(n):
            pos = seqs[0].n
            am, lg = b.forward([0, 1], seqs[0].next() * 2, [pos, pos], logits=True)
            for s in seqs:
                s.n = pos + 1
                assert_bit_equal(lg[s.slot], ref.logits[pos], f"{what}: slot {s.slot}: logits at {pos}")
                assert int(am[s.slot]) == ref_argmax(ref.logits[pos]), f"{what}: slot {s.slot}: argmax at {pos}"
                check_slot_rows(b, s, [pos], f"{what}: the row written at {pos}")

    steps(9)                                                 # 4100 .. 4108
    for upto in (4223, 4351):
        for s in seqs:                                       # a table chunk on either slot (slot 1 is forced anyway)
            prefill(b, fmt, s.slot, ref.toks[s.n:upto], s.n, forced_table=s.slot == 1)
            check_slot_rows(b, s, run_positions(s.n, upto - s.n), f"{what}: the prefill up to {upto}")
            s.n = upto
        steps(2)
    assert b.slot_pages(0) == (pages_of(4353, page_len), 0)


# ---------------------------------------------------------------------------------------------- G. pages above 2^32 bytes of a pool

@pytest.mark.parametrize("fmt", FORMATS)
def test_pages_above_4_gib_of_a_quantised_pool(L, fmt):
    """tests/test_batch_paged_deep.py::test_pages_high_in_a_pool_of_17_gb on quantised pages: mini-phi's geometry with three layers and 8192 positions,
    pages of 1024 positions, a pool of a little over 4 GiB.  The pool hands out pages 1, 2, 3, .. while nothing is released, and page p lies at
    p * page_bytes: burner slots 6 .. 63 claim a page per row at positions k * 1024 until the next page claimed is the first that lies wholly above
    2^32 bytes; a probe slot takes its first call there, and its fork the page above.  Short of memory the create call fails with the library's message."""
    cfg = dataclasses.replace(S.CONFIGS["mini-phi"], name="mini-phi-8k-3l", n_layers=3, max_pos=8192)
    img = S.build_image(cfg, S.Q8_0, seed=721)
    m = L.Transformer(img)
    PL, n_slots = 1024, 64
    nl, per_slot = m.args.n_layers, m.args.seq_len // PL
    small = qbatch(L, m, fmt, PL, 1, 1)                       # a pool of one page tells the page's size: every page number below follows from it
    page_bytes = small.kv_format()[2]
    small.close()
    target = -(-(1 << 32) // page_bytes)                      # the first page that starts at or above 2^32 bytes
    n_pages = target + 2
    assert target * page_bytes >= 1 << 32 > (target - 1) * page_bytes and target > 8
    toks = S.prompt_tokens(cfg, 73, 722)
    s = QSEQ[fmt](img, 0)
    s.feed(toks[:70])
    want_kv = {p: [[s.orc.kv_row(w, l, p) for w in (0, 1)] for l in range(nl)] for p in (0, 35, 69)}
    want_lg = [s.feed([t]) for t in toks[70:]]
    for k in range(3):
        want_kv[70 + k] = [[s.orc.kv_row(w, l, 70 + k) for w in (0, 1)] for l in range(nl)]
    b = qbatch(L, m, fmt, PL, n_slots, n_pages)
    claimed = lambda: n_pages - b.pages()[2]
    burners = list(range(6, n_slots))
    spots = [(slot, k) for k in range(per_slot) for slot in burners]     # every (slot, k) names a page nobody claimed; a call takes each slot once
    assert len(spots) >= target
    while claimed() < target - 1:
        n = min(len(burners), target - 1 - claimed())
        take, spots[:] = spots[:n], spots[n:]
        assert len({slot for slot, _ in take}) == n
        b.forward([slot for slot, _ in take], [1] * n, [k * PL for _, k in take])
    assert claimed() == target - 1

    def check_rows(slot, positions, what):
        for p in positions:
            for l in range(nl):
                for w in (0, 1):
                    assert_bit_equal(b.kv_row(slot, w, l, p), want_kv[p][l][w], f"{what}: slot {slot} {'kv'[w]} layer {l} pos {p}")

    probe, twin = 0, 1
    what = f"{fmt} page {target}, at {target * page_bytes} bytes"
    prefill(b, fmt, probe, toks[:70])
    assert claimed() == target and b.slot_pages(probe) == (1, 0)
    check_rows(probe, [0, 35, 69], f"{what}: prefill")
    assert_reads_zero(b, probe, nl, [70, 100, 1023], f"{what}: the claimed page was cleared")
    for k in range(3):
        am, lg = b.forward([probe], [int(toks[70 + k])], [70 + k], logits=True)
        assert_bit_equal(lg[0], want_lg[k], f"{what}: step {k}")
        assert int(am[0]) == ref_argmax(want_lg[k])
        check_rows(probe, [70 + k], f"{what}: step {k}")
    b.fork(probe, twin, 70)                                  # the partial page's rows into the next page up
    assert claimed() == target + 1 and b.slot_pages(twin) == (1, 0) and b.slot_pages(probe) == (1, 0)
    check_rows(twin, [0, 35, 69], f"{what}: the fork's copied rows")
    am, lg = b.forward([twin], [int(toks[70])], [70], logits=True)
    assert_bit_equal(lg[0], want_lg[0], f"{what}: the step on the fork")
    check_rows(twin, [70], f"{what}: the step on the fork")
    check_rows(probe, [0, 69, 70, 72], f"{what}: the probe after its fork was stepped")
