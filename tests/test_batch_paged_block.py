"""Prompts of a PAGED batch through block attention over the page table (launch_paged_attention_block, lm.rs_amd/csrc/lmrs_paged.inc): from MIN_ROWS rows
on (the measured crossover against the table pass, kPagedBlockMin in lmrs_api.hip; a contiguous batch starts at 16), lmrs_batch_prefill and
lmrs_batch_prefill_embeddings send a chunk through 64-query blocks whose key staging and value tiles look every address up in the slot's page row;
shorter chunks stay on the table pass and are held to the same references.  Judged against the CPU oracle (one shared run per model), against a wide batch the oracle already pins (embeddings), and
against the table pass the same batch took before (lmrs_batch_debug_prefill_table).  Every case also asserts what lmrs_batch_prefill_form says about
the calls it makes.  Every comparison is bit for bit.  No tolerances."""
import collections
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from test_batch import Seq, check_slot_rows, snapshot
from test_batch_embed import random_rows
from test_batch_paged_deep import check_ref_rows, config, make_batch, pages_of, zero_row
from tools import synth_lmrs as S

pytestmark = pytest.mark.gpu

N = 256
PL = 64
SEED = 811
MIN_ROWS = 112                                              # a paged batch's shortest chunk that takes block attention
# head sizes 64, 96, 128, Gemma's 256; and a Q4_0 file
CFGS = [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-llama3b", S.Q8_0), ("mini-gemma", S.Q8_0), ("mini-llama", S.Q4_0)]

Ref = collections.namedtuple("Ref", "cfg img toks logits K V")


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


@functools.lru_cache(maxsize=None)
def reference(cfg, q):
    """The oracle over the 256 positions of one seeded token run (test_batch_paged_deep.reference's fields, without the branches): read-only"""
    c = S.CONFIGS[cfg]
    img = S.build_image(c, q, seed=SEED)
    toks = S.prompt_tokens(c, N, SEED)
    orc = O.Oracle(img)
    logits = np.stack([orc.forward(int(toks[p]), p).copy() for p in range(N)])
    kv = [np.stack([np.stack([orc.kv_row(w, l, p) for p in range(N)]) for l in range(c.n_layers)]) for w in (0, 1)]
    for a in (toks, logits, kv[0], kv[1]):
        a.setflags(write=False)
    return Ref(c, img, toks, logits, kv[0], kv[1])


def check_zero(b, m, slot, positions, what):
    for layer in range(m.args.n_layers):
        for p in positions:
            for w in (0, 1):
                assert_bit_equal(b.kv_row(slot, w, layer, p), zero_row(m), f"{what}: slot {slot} {'kv'[w]} layer {layer} pos {p} was never written")


def decode_step(b, ref, slots, depths, what):
    """one pass: slot i feeds toks[depths[i]] at depths[i]; logits, argmax and the written row against the reference"""
    am, lg = b.forward(slots, [int(ref.toks[d]) for d in depths], depths, logits=True)
    for i, (s, d) in enumerate(zip(slots, depths)):
        assert_bit_equal(lg[i], ref.logits[d], f"{what}: decode row {i} (slot {s}, pos {d}): logits")
        assert int(am[i]) == ref_argmax(ref.logits[d]), f"{what}: decode row {i} (slot {s}, pos {d}): argmax"
        check_ref_rows(b, ref, s, [d], f"{what}: the decode step's row")


def prefill_as(b, ref, slot, start, n, what):
    """toks[start : start + n] into `slot`, after asserting the form the library says the call takes on a paged batch"""
    assert b.prefill_form(n, start) == (1, 1 if n >= MIN_ROWS else 0), f"{what}: prefill_form({n}, {start})"
    assert b.prefill(slot, ref.toks[start:start + n], start) == start + n


# ---------------------------------------------------------------------------------------------- 1. block edges

EDGES = [15, 16, 17, 63, 64, 65, 128, 129, 200]


@pytest.mark.parametrize("cfg,q", CFGS)
def test_block_edges(L, cfg, q):
    """one slot per length: lengths below the paged rule's row count (the table pass), two whole blocks, one row more, and a partial fourth block"""
    ref = reference(cfg, q)
    what = f"{cfg} q{q}"
    m = L.Transformer(ref.img)
    b = make_batch(L, m, PL, len(EDGES))
    for i, n in enumerate(EDGES):
        prefill_as(b, ref, i, 0, n, what)
        assert b.slot_pages(i) == (pages_of(n, PL), 0)
    for i, n in enumerate(EDGES):
        check_ref_rows(b, ref, i, range(n), f"{what}: prefill of {n}")
        check_zero(b, m, i, range(n, pages_of(n, PL) * PL), f"{what}: prefill of {n}")
    decode_step(b, ref, list(range(len(EDGES))), EDGES, what)


# ---------------------------------------------------------------------------------------------- 2. pos0 inside a chunk and a page

@pytest.mark.parametrize("cfg,q", CFGS)
def test_calls_that_start_inside_a_key_chunk(L, cfg, q):
    """70 + 100 + 16, 63 + 65 and 64 + 64: calls that start inside a page and a key chunk, one row short of the page edge, and on it - table passes under
    the paged rule; 70 + 120: the same start by block attention - its key chunk [64, 128) mixes rows of the first call with its own"""
    ref = reference(cfg, q)
    what = f"{cfg} q{q}"
    m = L.Transformer(ref.img)
    plans = [[70, 100, 16], [63, 65], [64, 64], [70, 120]]
    b = make_batch(L, m, PL, len(plans))
    for slot, plan in enumerate(plans):
        at = 0
        for n in plan:
            prefill_as(b, ref, slot, at, n, f"{what}: {plan}")
            at += n
        assert b.slot_pages(slot) == (pages_of(at, PL), 0)
        check_ref_rows(b, ref, slot, range(at), f"{what}: {plan}")
        check_zero(b, m, slot, range(at, pages_of(at, PL) * PL), f"{what}: {plan}")
    decode_step(b, ref, list(range(len(plans))), [sum(p) for p in plans], what)


# ---------------------------------------------------------------------------------------------- 3. scattered pages

@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("cfg,q", CFGS)
def test_scattered_pages(L, cfg, q, pieces):
    """two slots prefilled alternately in 64-token pieces - A, B, A, B: the pool hands out pages in order, so neither slot's pages are adjacent - then each
    slot's last positions in one call.  pieces = 1: 128 positions from 64 on; pieces = 2: the 127 positions from 128 on, the most that leaves the
    256-position fixtures a position to decode at."""
    ref = reference(cfg, q)
    what = f"{cfg} q{q} {pieces} pieces"
    m = L.Transformer(ref.img)
    b = make_batch(L, m, PL, 2)
    for k in range(pieces):
        for slot in (0, 1):
            prefill_as(b, ref, slot, k * PL, PL, what)
    start, n = pieces * PL, 128 if pieces == 1 else 127
    for slot in (0, 1):
        prefill_as(b, ref, slot, start, n, what)
    for slot in (0, 1):
        assert b.slot_pages(slot) == (pages_of(start + n, PL), 0)
        check_ref_rows(b, ref, slot, range(start + n), what)
    decode_step(b, ref, [0, 1], [start + n] * 2, what)


# ---------------------------------------------------------------------------------------------- 4. copy on write under a block pass

@pytest.mark.parametrize("n_other", [80, 120])
@pytest.mark.parametrize("cfg,q", CFGS)
def test_copy_on_write_under_a_block_pass(L, cfg, q, n_other):
    """n_other = 120: the fork's write is a block pass; 80: below the paged rule's row count, the table pass"""
    ref = reference(cfg, q)
    what = f"{cfg} q{q} {n_other} rows"
    nl = ref.cfg.n_layers
    m = L.Transformer(ref.img)
    b = make_batch(L, m, PL, 2)
    prefill_as(b, ref, 0, 0, 128, what)
    b.fork(0, 1, 128)
    assert b.slot_pages(0) == (2, 2) and b.slot_pages(1) == (2, 2)
    before = snapshot(b, 0, range(128), nl)
    other = S.prompt_tokens(ref.cfg, n_other, SEED + 1)
    end = 96 + n_other
    assert b.prefill_form(n_other, 96) == (1, 1 if n_other >= MIN_ROWS else 0)
    assert b.prefill(1, other, 96) == end                   # into the shared page [64, 128) - a whole-page copy first - and new pages
    s = Seq(ref.img, 1)
    s.feed(ref.toks[:96]); s.feed(other)
    check_slot_rows(b, s, range(end), f"{what}: the fork's own sequence")
    for x, y in zip(before, snapshot(b, 0, range(128), nl)):
        assert_bit_equal(x, y, f"{what}: the source moved by the fork's block pass")
    check_ref_rows(b, ref, 0, range(128), f"{what}: the source")
    assert b.slot_pages(0) == (2, 1) and b.slot_pages(1) == (pages_of(end, PL), 1), f"{what}: page [64, 128) is un-shared, page [0, 64) still shared"
    am, lg = b.forward([1], [5], [end], logits=True)
    assert_bit_equal(lg[0], s.feed([5]), f"{what}: the step behind the fork's prefill")


# ---------------------------------------------------------------------------------------------- 5. differential against the table pass

def both_routings(L, cfg, q, page_len, what):
    """530 tokens at 0 (two chunks: 512 rows by block attention, 18 rows below the paged rule's row count) and 300 at 530 on two paged batches of one
    model, one of them forced to the table pass: every K/V row of every layer and three decode steps' logits must be equal"""
    m = L.Transformer(S.build_image(config(cfg), q, seed=SEED))
    assert m.args.seq_len == 1024
    toks = S.prompt_tokens(config(cfg), 833, SEED + 2)
    got = []
    for force in (False, True):
        b = make_batch(L, m, page_len, 1)
        if force:
            b.debug_prefill_table(True)
        assert b.prefill_form(530, 0) == ((2, 0) if force else (2, 1)), f"{what}: prefill_form(530, 0), forced {force}"
        assert b.prefill_form(300, 530) == ((1, 0) if force else (1, 1)), f"{what}: prefill_form(300, 530), forced {force}"
        assert b.prefill(0, toks[:530], 0) == 530 and b.prefill(0, toks[530:830], 530) == 830
        assert b.slot_pages(0) == (pages_of(830, page_len), 0)
        out = []
        for k in range(3):
            am, lg = b.forward([0], [int(toks[830 + k])], [830 + k], logits=True)
            out.append(lg[0].copy())
        out += snapshot(b, 0, range(833), m.args.n_layers)
        got.append(out)
        if force:
            b.debug_prefill_table(False)
            assert b.prefill_form(530, 0) == (2, 1) and b.prefill_form(1024, 0) == (2, 2), f"{what}: the library's rule again"
        b.close()
    assert len(got[0]) == len(got[1])
    for i, (x, y) in enumerate(zip(*got)):
        assert_bit_equal(x, y, f"{what}: output {i} (3 decode logits, then k / v per layer and position): block attention against the table pass")


DIFF = [("mini-llama-1k", S.Q8_0), ("mini-llama3b-1k", S.Q8_0), ("mini-gemma-1k", S.Q8_0), ("mini-phi-long", S.Q8_0), ("mini-llama-1k", S.Q4_0)]


@pytest.mark.parametrize("page_len", [64, 256, 1024])
@pytest.mark.parametrize("cfg,q", DIFF)
def test_block_attention_equals_the_table_pass(L, cfg, q, page_len):
    both_routings(L, cfg, q, page_len, f"{cfg} q{q} page_len {page_len}")


def test_block_attention_equals_the_table_pass_with_scores_in_memory(L, monkeypatch):
    """LMRS_ATT_LDS_KEYS lowered at create: the memory-resident softmax runs between the two new launches"""
    monkeypatch.setenv("LMRS_ATT_LDS_KEYS", "64")
    both_routings(L, "mini-llama-1k", S.Q8_0, 64, "mini-llama-1k, scores in memory")


def test_block_attention_equals_the_table_pass_in_gemmas_long_forms(L, monkeypatch):
    """LMRS_ATT_LONG_BATCH_FORMS at create: Gemma-2's 64-key score form and 64-dim value slices (without it the short forms run, as in the cases above)"""
    monkeypatch.setenv("LMRS_ATT_LONG_BATCH_FORMS", "1")
    both_routings(L, "mini-gemma-1k", S.Q8_0, 64, "mini-gemma-1k, long-batch forms")


# ---------------------------------------------------------------------------------------------- 6. embeddings

@pytest.mark.parametrize("cfg", ["mini-phi", "mini-gemma"])
def test_embedding_rows_against_a_wide_batch(L, cfg):
    """130 rows at 0 (block attention) and 70 at 130 (on pages the table pass) with the residual asked for: block rows are in position order, so the
    residual comes straight from the pass; Gemma-2's window is taken on each call's first position.  The wide batch is pinned against the oracle by tests/test_batch_embed.py."""
    img = S.build_image(cfg, S.Q8_0, seed=SEED + 3)
    m = L.Transformer(img)
    rows = [random_rows(130, m.args.dim, SEED + 4), random_rows(70, m.args.dim, SEED + 5)]
    got = []
    for form in ("wide", PL):
        b = make_batch(L, m, form, 1)
        assert b.prefill_form(130, 0) == (1, 1) and b.prefill_form(70, 130) == (1, 1 if form == "wide" else 0), f"{cfg} {form}"
        out, at = [], 0
        for r in rows:
            keep = r.copy()
            end, res = b.prefill_embeddings(0, r, at, residual=True)
            assert end == at + len(r)
            assert_bit_equal(r, keep, "the caller's rows are never written")
            out.append(res.copy()); at = end
        out += snapshot(b, 0, range(200), m.args.n_layers)
        got.append(out)
        b.close()
    for i, (x, y) in enumerate(zip(*got)):
        assert_bit_equal(y, x, f"{cfg}: output {i} (two residual blocks, then k / v per layer and position): paged against wide")


# ---------------------------------------------------------------------------------------------- 7. pages above 2^32 floats

def test_block_attention_on_pages_above_2_pow_32_floats(L):
    """tests/test_batch_paged_deep.py::test_pages_high_in_a_pool_of_17_gb's recipe: single-row steps on burner slots claim pages until the next page
    claimed starts above 2^32 floats of the pool; then 130 tokens into a fresh slot by block attention and into another by the table pass: equal rows"""
    cfg = dataclasses.replace(S.CONFIGS["mini-phi"], name="mini-phi-8k", max_pos=8192)
    img = S.build_image(cfg, S.Q8_0, seed=721)
    m = L.Transformer(img)
    PLH, n_slots, n_pages = 1024, 64, 352
    a = m.args
    nl, per_slot = a.n_layers, a.seq_len // PLH
    stride = 2 * nl * PLH * a.n_kv_heads * a.head_size
    target = -(-(1 << 32) // stride)
    assert target + 2 <= n_pages
    b = L.Batch(m, n_slots, page_len=PLH, n_pages=n_pages)
    claimed = lambda: n_pages - b.pages()[2]
    burners = list(range(6, n_slots))
    spots = [(slot, k) for k in range(per_slot) for slot in burners]
    while claimed() < target:
        n = min(len(burners), target - claimed())
        take, spots[:] = spots[:n], spots[n:]
        b.forward([slot for slot, _ in take], [1] * n, [k * PLH for _, k in take])
    assert claimed() == target and (target + 1) * stride >= 1 << 32
    toks = S.prompt_tokens(cfg, 130, 722)
    assert b.prefill_form(130, 0) == (1, 1)
    assert b.prefill(0, toks, 0) == 130 and claimed() == target + 1
    b.debug_prefill_table(True)
    assert b.prefill_form(130, 0) == (1, 0)
    assert b.prefill(1, toks, 0) == 130 and claimed() == target + 2
    b.debug_prefill_table(False)
    for x, y in zip(snapshot(b, 0, range(131), nl), snapshot(b, 1, range(131), nl)):
        assert_bit_equal(x, y, f"page {target + 1} (block attention) against page {target + 2} (the table pass)")
    assert np.any(b.kv_row(0, 0, nl - 1, 129) != 0) and not np.any(b.kv_row(0, 0, nl - 1, 130))


# ---------------------------------------------------------------------------------------------- 8. errors, and the rule on a contiguous batch

def test_errors_and_the_rule(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=SEED + 6)
    m = L.Transformer(img)
    toks = S.prompt_tokens(cfg, 200, SEED + 7)
    b = L.Batch(m, 2, page_len=PL, n_pages=3)
    assert b.prefill(0, toks[:20], 0) == 20
    nl = m.args.n_layers
    for force in (False, True):                              # short of pages: the existing message, nothing changed - whichever form the call would take
        b.debug_prefill_table(force)
        before, rows = (b.pages(), b.slot_pages(0), b.slot_pages(1)), snapshot(b, 0, [0, 19, 20, 63], nl)
        assert b.prefill_form(200, 0) == (1, 0 if force else 1) and b.prefill_form(180, 20) == (1, 0 if force else 1)
        with pytest.raises(L.LmrsError, match=r"lmrs_batch_prefill: 4 pages wanted, 2 free"):
            b.prefill(1, toks, 0)
        with pytest.raises(L.LmrsError, match=r"lmrs_batch_prefill: 3 pages wanted, 2 free"):
            b.prefill(0, toks[20:], 20)
        assert (b.pages(), b.slot_pages(0), b.slot_pages(1)) == before
        for x, y in zip(rows, snapshot(b, 0, [0, 19, 20, 63], nl)):
            assert_bit_equal(x, y, "a refused prefill changed a row")
    b.debug_prefill_table(False)
    assert b.prefill(0, toks[20:100], 20) == 100             # the batch is still usable
    # refusals before any device work
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_prefill_form: start_pos \+ n = 257 exceeds seq_len = 256"):
        b.prefill_form(57, 200)
    lib = L.lib()
    one = ctypes.c_uint32()
    for args in ((b._h, 10, 0, None, ctypes.byref(one)), (b._h, 10, 0, ctypes.byref(one), None), (None, 10, 0, ctypes.byref(one), ctypes.byref(one))):
        assert lib.lmrs_batch_prefill_form(*args) != 0
        assert "lmrs_batch_prefill_form: NULL argument" in lib.lmrs_last_error().decode()
    for plain in (L.Batch(m, 2), L.Batch(m, 2, wide=True)):
        with pytest.raises(L.LmrsError, match=r"lmrs_batch_debug_prefill_table: not a paged batch"):
            plain.debug_prefill_table(True)
        # the rule on a contiguous batch: one row goes through the table pass, 2 .. 15 rows one workgroup per (head, row), block attention from 16 on
        assert [plain.prefill_form(n, 0) for n in (0, 1, 2, 15, 16, 256)] == [(0, 0), (1, 0), (1, 0), (1, 0), (1, 1), (1, 1)]
        assert plain.prefill_form(16, 240) == (1, 1)
        plain.close()
    rows = (0, 1, 15, 16, MIN_ROWS - 1, MIN_ROWS, 256)
    assert [b.prefill_form(n, 0) for n in rows] == [(0, 0)] + [(1, 0)] * 4 + [(1, 1)] * 2, "the paged rule starts at MIN_ROWS rows"


def test_the_rule_beyond_one_gib_of_score_slabs(L):
    """128 heads x 8 query blocks x T keys x 64 queries x 4 bytes: a 512-row chunk leaves block attention once T passes 4096 keys - on both kinds of
    batch (the library keeps at most 8192 positions, so 32 heads never get there)"""
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-128h", n_heads=128, n_layers=1, max_pos=8192)
    m = L.Transformer(S.build_image(cfg, S.Q8_0, seed=SEED + 8))
    assert m.args.seq_len == 8192
    for b in (L.Batch(m, 1), L.Batch(m, 1, page_len=1024, n_pages=2)):
        assert b.prefill_form(512, 3584) == (1, 1)           # T = 4096: exactly 1 GiB (512 rows: above either batch's row count)
        assert b.prefill_form(512, 3585) == (1, 0)
        assert b.prefill_form(1024, 3073) == (2, 1)          # the chunk at 3073 ends at 3585 keys, the one at 3585 at 4097
        assert b.prefill_form(120, 8000) == (1, 1)           # two blocks of up to 8120 keys
        b.close()
