"""Hostile activations through the batch passes.  tests/test_stress_regimes.py drives the recipes of tests/stress_models.py - underflowing and
subnormal softmax terms, saturated soft-caps, all-zero quantisation groups, outlier channels, SiLU / GELU at their extremes, exactly tied logits -
through the single-sequence paths; every lmrs_batch_* call has its own copies of that arithmetic (the skinny and stream GEMMs' epilogues, the row
quantisers, attention over a row table, the paged softmax, block attention over a page table, the batch's soft-cap, argmax, top-k, sampler, mask and
penalty kernels) and had only ever seen narrow Gaussian weights.  Here those calls run on the recipes.

The reference is ONE sequential oracle decode per (model, format, recipe) of N positions of one token sequence (oracle_run): every slot of a test holds a
prefix of that sequence, so a slot at depth d fed toks[d] must give the run's logits row d and write the run's K/V row d - a slot's state is a function
of its tokens alone.  Logits and K/V rows are compared bit for bit, tokens and indices by value.  No tolerances.

CPU tier (unmarked): the reference against test_stress_regimes.oracle_decode, and for every GPU case the recipe's witness (check_witness) over the
counters of exactly the positions that case compares.  GPU tier: the same witness again, before the device is touched, then the comparison."""
import collections
import dataclasses
import functools
import types

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax, run_positions
from penalty_rules import NONE, penalised
from test_batch import Seq, check_slot_rows, snapshot, step
from test_batch_mask import ban, masked
from test_batch_runs import run_pass
from test_batch_sample import KINDS
from test_stress_regimes import CASES, SEED, check_witness, h_quantiser_fused, image_of, oracle_decode, recipes_for
from test_topk import rank_row
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
N = 140
PL = 64
# the table attention's form changes (one wave's 64 keys, the 128-key pass) and the page edges of page_len 64; with 3 steps the deepest row ends at 133
D16 = [0, 2, 7, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 130, 100, 5]
STEPS = 3

Ref = collections.namedtuple("Ref", "img cfg toks rows K V stats")


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


# ---------------------------------------------------------------------------------------------- the reference: one oracle run, many slots

@functools.lru_cache(maxsize=None)
def oracle_run(cfg, q, recipe):
    """One sequential oracle decode of N positions of S.prompt_tokens(c, N, SEED) on the recipe's image -> the logits of every position, the K and V
    rows [layers, N, kv_dim], and the regime counters of every single position.  Read-only."""
    img, c = image_of(cfg, q, recipe)
    toks = S.prompt_tokens(c, N, SEED)
    orc = O.Oracle(img)
    rows, stats = [], []
    for pos, t in enumerate(toks):
        O.stats_reset()
        rows.append(orc.forward(int(t), pos).copy())
        stats.append(O.stats())
    rows = np.stack(rows)
    kv = [np.stack([np.stack([orc.kv_row(w, l, p) for p in range(N)]) for l in range(c.n_layers)]) for w in (0, 1)]
    for a in (toks, rows, kv[0], kv[1]):
        a.setflags(write=False)
    return Ref(img, c, toks, rows, kv[0], kv[1], tuple(stats))


def summed(stats):
    """the counters of several positions as one run's: integers add, the scale ratio is a maximum"""
    out = {}
    for st in stats:
        for k, v in st.items():
            out[k] = max(out.get(k, 0.0), v) if k == "max_scale_ratio" else out.get(k, 0) + v
    return out


def witness(cfg, q, recipe, positions):
    """check_witness over exactly `positions` of the shared run -> the run"""
    ref = oracle_run(cfg, q, recipe)
    pos = sorted(set(int(p) for p in positions))
    assert pos and 0 <= pos[0] and pos[-1] < N
    check_witness(recipe, ref.cfg, q, summed(ref.stats[p] for p in pos), ref.rows[pos], len(pos))
    return ref


class RefCache:
    """what check_slot_rows asks of an oracle, answered from the shared run"""

    def __init__(self, ref):
        self.ref, self.args = ref, types.SimpleNamespace(n_layers=ref.cfg.n_layers, vocab_size=ref.cfg.vocab_size)

    def kv_row(self, which, layer, pos):
        return (self.ref.K, self.ref.V)[which][layer, pos]


class RefSeq(Seq):
    """test_batch.Seq on the shared run: a slot standing at depth n holds toks[:n] and may only be fed toks[n]"""

    def __init__(self, ref, slot, n=0):
        self.slot, self.orc, self.n, self.ref = slot, RefCache(ref), n, ref

    def feed(self, toks):
        lg = None
        for t in toks:
            assert int(t) == int(self.ref.toks[self.n]), f"slot {self.slot} at {self.n}: the shared reference knows one token sequence only"
            lg = self.ref.rows[self.n]
            self.n += 1
        return lg

    def next(self, n=1):
        return [int(t) for t in self.ref.toks[self.n:self.n + n]]


def depths(n):
    return [D16[i % 16] for i in range(n)]


def populate(b, ref, ds, src, what, two_chunks=False):
    """slot i at depth ds[i], made both ways: odd slots by fork from slot `src`, prefilled with the whole run (src may be one of the slots: rows behind
    a slot's depth are never seen); even slots by prefill (two_chunks: toks[:d // 2], then the rest).  K/V rows of every slot at {0, d // 2, d - 1}."""
    assert b.prefill(src, ref.toks, 0) == N
    seqs = []
    for i, d in enumerate(ds):
        if d and i != src:
            if i % 2:
                b.fork(src, i, d)
            elif two_chunks and d // 2:
                assert b.prefill(i, ref.toks[:d // 2], 0) == d // 2 and b.prefill(i, ref.toks[d // 2:d], d // 2) == d
            else:
                assert b.prefill(i, ref.toks[:d], 0) == d
        s = RefSeq(ref, i, d)
        seqs.append(s)
        if d:
            check_slot_rows(b, s, sorted({0, d // 2, d - 1}), f"{what}: slot {i} made at depth {d}")
    return seqs


def steps(b, seqs, n, what, logits=True):
    for k in range(n):
        step(b, seqs, [s.next()[0] for s in seqs], f"{what} step {k}", logits=logits)


def step_positions(ds, n=STEPS):
    return [d + k for d in ds for k in range(n)]


def ident(v):
    if isinstance(v, S.ModelCfg):
        return v.name
    return {S.Q8_0: "q8", S.Q4_0: "q4"}.get(v, None) if isinstance(v, int) and not isinstance(v, bool) else None


WITNESSED = []                      # (GPU test, cfg, q, recipe, the positions it compares): the CPU tier's witness test runs over every entry


def cases(name, triples, positions):
    """the parameter list of GPU test `name`; positions(cfg, q, recipe, *more) -> the positions the case compares"""
    for t in triples:
        WITNESSED.append((name,) + tuple(t[:3]) + (tuple(sorted(set(positions(*t)))),))
    return triples


def by_recipe(pairs, recipes, gemma=()):
    return [(c, q, r) for c, q in pairs for r in tuple(recipes) + (tuple(gemma) if "gemma" in c else ())]


# ---------------------------------------------------------------------------------------------- 1. narrow batch: skinny GEMM, attention over the row table

SUBSET = [11, 3, 14]                # the fourth pass: three rows in shuffled slot order


def narrow_positions(cfg, q, recipe):
    return step_positions(D16) + [D16[i] + STEPS for i in SUBSET]


NARROW = cases("narrow", [(c, q, r) for c, q in CASES for r in recipes_for(c)], narrow_positions)


@gpu
@pytest.mark.parametrize("cfg,q,recipe", NARROW, ids=ident)
def test_narrow_batch(L, cfg, q, recipe):
    """16 rows at D16, three passes with logits (gemm_skinny_kernel's epilogues, rows_prologue_kernel, attention_table_kernel, softcap_rows_kernel and
    the per-row argmax), then three of the rows in shuffled order: argmax, logits and the written K/V row of every row"""
    ref = witness(cfg, q, recipe, narrow_positions(cfg, q, recipe))
    what = f"{ref.cfg.name} q{q} {recipe}"
    m = L.Transformer(ref.img); b = L.Batch(m, 16)
    seqs = populate(b, ref, D16, 15, what)
    steps(b, seqs, STEPS, what)
    steps(b, [seqs[i] for i in SUBSET], 1, f"{what}, slots {SUBSET}")
    b.close(); m.close()


@gpu
def test_batches_refuse_f32_stress_images(L):
    """unquantised files have no batched pass: the stress file's two f32 images stay with the single-sequence tests"""
    m = L.Transformer(image_of("mini-llama", S.Q_NONE, "peaked")[0])
    with pytest.raises(L.LmrsError, match="f32"):
        L.Batch(m, 2)
    m.close()


# ---------------------------------------------------------------------------------------------- 2. wide batch: the stream GEMM

def wide_positions(cfg, q, recipe, n):
    return step_positions(depths(n))


WIDE = cases("wide", [(c, q, r, 64) for c, q in CASES for r in recipes_for(c) if r != "tied_classifier"]
             + [(c, q, r, 33) for c, q in (("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)) for r in recipes_for(c) if r != "tied_classifier"], wide_positions)


@gpu
@pytest.mark.parametrize("cfg,q,recipe,n", WIDE, ids=ident)
def test_wide_batch(L, cfg, q, recipe, n):
    """n = 64 and 33 rows a pass, cycling through D16 (gemm_stream_kernel's epilogues at four and at three token tiles): three passes"""
    ref = witness(cfg, q, recipe, wide_positions(cfg, q, recipe, n))
    what = f"{ref.cfg.name} q{q} {recipe} {n} rows"
    m = L.Transformer(ref.img); b = L.Batch(m, 64, wide=True)
    seqs = populate(b, ref, depths(n), n - 1, what)
    steps(b, seqs, STEPS, what)
    b.close(); m.close()


# ---------------------------------------------------------------------------------------------- 3. ragged passes

STARTS = [0, 63, 64, 5, 100]
# R -> run lengths: the full skinny tile, the stream GEMM, the first ring-kernel size, a ragged multi-tile pass
LENS = {16: [1, 5, 7, 3], 40: [17, 1, 13, 9], 48: [21, 3, 20, 4], 130: [70, 3, 40, 16, 1]}


def n_outs(lens):
    return [(n, 0, 1, n, 1)[i] for i, n in enumerate(lens)]                    # every row, none, the last one


def ragged_positions(cfg, q, recipe, R):
    """the rows with outputs and the K/V rows run_pass(kv="ends") reads"""
    pos = []
    for d, n, no in zip(STARTS, LENS[R], n_outs(LENS[R])):
        pos += list(range(d + n - no, d + n)) + run_positions(d, n)
    return pos


RAGGED = cases("ragged", [(c, q, r, R) for c, q, r in by_recipe([("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q4_0)],
                                                                ("peaked", "dead_groups", "outliers", "glu_extremes", "combined"), gemma=("softcap",))
                          for R in sorted(LENS)], ragged_positions)


@gpu
@pytest.mark.parametrize("cfg,q,recipe,R", RAGGED, ids=ident)
def test_ragged_pass(L, cfg, q, recipe, R):
    """forward_runs over 4 - 5 slots (attention_runs_kernel, select_rows_kernel): R = 16 the skinny GEMM, 40 the stream GEMM, 48 and 130 the ring
    kernels - at 130 rows of a Q8_0 model with h quantised in w1/w3's epilogue, asserted through the library's own tile rule"""
    lens = LENS[R]
    assert sum(lens) == R
    ref = witness(cfg, q, recipe, ragged_positions(cfg, q, recipe, R))
    what = f"{ref.cfg.name} q{q} {recipe} R {R}"
    if q == S.Q8_0:
        assert h_quantiser_fused(L, ref.cfg, R) == (R == 130), f"{what}: the w1/w3 launch is not the one this case is for"
    m = L.Transformer(ref.img); b = L.Batch(m, len(lens) + 1)
    seqs = populate(b, ref, STARTS[:len(lens)] + [0], len(lens), what)[:len(lens)]
    run_pass(b, [(s, s.next(n), no) for s, n, no in zip(seqs, lens, n_outs(lens))], what, kv="ends")
    b.close(); m.close()


# ---------------------------------------------------------------------------------------------- 4. paged batches, page_len 64

def paged_batch(L, m, n_slots):
    return L.Batch(m, n_slots, page_len=PL, n_pages=n_slots * -(-m.args.seq_len // PL))


def paged_table_positions(cfg, q, recipe):
    return step_positions(D16)


PAGED_TABLE = cases("paged_table", by_recipe(CASES, ("peaked", "peaked_mild", "dead_groups", "combined"), gemma=("softcap",)), paged_table_positions)


@gpu
@pytest.mark.parametrize("cfg,q,recipe", PAGED_TABLE, ids=ident)
def test_paged_table_pass(L, cfg, q, recipe):
    """16 slots at D16, half of them forks of one prefilled slot (shared pages), half prefilled in two chunks below the block rule's row count
    (paged_attention_body behind a page row), then three passes whose rows cross the page edges at 64 and 128"""
    ref = witness(cfg, q, recipe, paged_table_positions(cfg, q, recipe))
    what = f"{ref.cfg.name} q{q} {recipe} paged"
    m = L.Transformer(ref.img); b = paged_batch(L, m, 17)
    seqs = populate(b, ref, D16 + [0], 16, what, two_chunks=True)[:16]
    assert b.slot_pages(11) == (2, 2), f"{what}: the fork at 128 shares its two pages with the source"
    steps(b, seqs, STEPS, what)
    b.close(); m.close()


BLOCK_ROWS = [7, 67, 126]


def paged_block_positions(cfg, q, recipe):
    return BLOCK_ROWS + [127, 128]


PAGED_BLOCK = cases("paged_block", by_recipe(CASES, ("peaked", "peaked_mild", "outliers", "glu_extremes"), gemma=("softcap",)), paged_block_positions)


def block_prefill(b, ref, slot, what, block):
    """toks[7:127] behind a 7-token prefill, after asserting the form the library says the 120 rows take"""
    assert b.prefill(slot, ref.toks[:7], 0) == 7
    assert b.prefill_form(120, 7) == (1, 1 if block else 0), f"{what}: prefill_form(120, 7)"
    assert b.prefill(slot, ref.toks[7:127], 7) == 127


@gpu
@pytest.mark.parametrize("cfg,q,recipe", PAGED_BLOCK, ids=ident)
def test_paged_block_attention(L, cfg, q, recipe):
    """120 prompt rows of a paged batch in one block chunk (block_paged_scores_kernel / _wide_kernel, the memory softmax, block_paged_values_kernel):
    K/V rows of every layer at 7, 67 and 126, then two passes on that cache and on a fork of it"""
    ref = witness(cfg, q, recipe, paged_block_positions(cfg, q, recipe))
    what = f"{ref.cfg.name} q{q} {recipe} block"
    m = L.Transformer(ref.img); b = paged_batch(L, m, 2)
    block_prefill(b, ref, 0, what, True)
    b.fork(0, 1, 127)
    seqs = [RefSeq(ref, 0, 127), RefSeq(ref, 1, 127)]
    for s in seqs:
        check_slot_rows(b, s, BLOCK_ROWS, what)
    steps(b, seqs, 2, what)
    b.close(); m.close()


def paged_both_positions(cfg, q, recipe):
    return range(127)


PAGED_BOTH = cases("paged_both", [("mini-llama", S.Q8_0, "peaked"), ("mini-gemma", S.Q8_0, "softcap")], paged_both_positions)


@gpu
@pytest.mark.parametrize("cfg,q,recipe", PAGED_BOTH, ids=ident)
def test_paged_block_attention_equals_the_table_pass(L, cfg, q, recipe):
    """the same 120 rows by block attention and, forced, by the table pass: bit-identical K/V rows at every position, and the reference's"""
    ref = witness(cfg, q, recipe, paged_both_positions(cfg, q, recipe))
    what = f"{ref.cfg.name} q{q} {recipe}"
    m = L.Transformer(ref.img); b = paged_batch(L, m, 2)
    block_prefill(b, ref, 0, what, True)
    b.debug_prefill_table(True)
    block_prefill(b, ref, 1, what, False)
    b.debug_prefill_table(False)
    nl = ref.cfg.n_layers
    for x, y in zip(snapshot(b, 0, range(127), nl), snapshot(b, 1, range(127), nl)):
        assert_bit_equal(x, y, f"{what}: block attention against the table pass")
    check_slot_rows(b, RefSeq(ref, 1, 127), range(127), f"{what}: the table pass")
    b.close(); m.close()


# ---------------------------------------------------------------------------------------------- 5. ties: the first maximum wins in every batch call

RUN_SLOTS, RUN_LENS = [8, 0, 11, 6, 2], [1, 4, 1, 7, 3]
GEN_SLOTS, N_NEW = [0, 1, 15, 2], 24
WIDE_ROWS = 40


def wide_run_len(i):
    return (1, 2, 1, 3)[i % 4]


def ties_positions(cfg, q, recipe, rows):
    """one forward over every row, then runs behind it (narrow: RUN_SLOTS; wide: every row) - the greedy tokens have oracles of their own"""
    ds = depths(rows)
    pos = list(ds)
    for i, n in (zip(RUN_SLOTS, RUN_LENS) if rows == 16 else ((i, wide_run_len(i)) for i in range(rows))):
        pos += range(ds[i] + 1, ds[i] + 1 + n)
    return pos


TIES = cases("ties", [(c, q, "tied_classifier", 16) for c, q in CASES]
             + [(c, q, "tied_classifier", WIDE_ROWS) for c, q in (("mini-llama", S.Q8_0), ("mini-gemma", S.Q8_0))], ties_positions)


def twins_rank_in_pairs(ref, positions):
    """in the reference's own ranking of a tied_classifier row, ranks 0 / 1 and 2 / 3 are a twin pair each, the lower index first"""
    half = ref.cfg.vocab_size // 2
    for p in sorted(set(positions)):
        r = rank_row(ref.rows[p])[:4]
        assert r[0] < half and r[1] == r[0] + half and r[2] < half and r[3] == r[2] + half, f"{ref.cfg.name} pos {p}: {r}"


def greedy_after(L, b, ref, seqs, what):
    """generate_greedy over `seqs` from their depths, fed toks[depth]: N_NEW tokens a row against the oracle's sequential greedy decode of the same
    sequence.  Rows at one depth hold one sequence, so one oracle serves them: it is fed the run once, then branches from the deepest depth down (a
    branch overwrites only oracle rows behind its own depth)."""
    V = ref.cfg.vocab_size
    pos = [s.n for s in seqs]
    out = b.generate_greedy([s.slot for s in seqs], [s.next()[0] for s in seqs], pos, N_NEW)
    assert out.shape == (len(seqs), N_NEW)
    o = Seq(ref.img, None)
    o.feed(ref.toks[:max(pos)])
    for d in sorted(set(pos), reverse=True):
        o.n = d
        t, want = int(ref.toks[d]), []
        for _ in range(N_NEW):
            t = ref_argmax(o.feed([t])); want.append(t)
        assert max(want) < V // 2, f"{what}: the reference's greedy tokens from {d} must be lower twins"
        for i, s in enumerate(seqs):
            if pos[i] == d:
                assert out[i].tolist() == want, f"{what}: row {i} (slot {s.slot} from {d}): greedy tokens"
                o.slot = s.slot
                check_slot_rows(b, o, [d, d + N_NEW // 2, d + N_NEW - 1], f"{what}: rows left by generate_greedy")


@gpu
@pytest.mark.parametrize("cfg,q,recipe,rows", TIES, ids=ident)
def test_first_maximum_wins_in_every_batch_call(L, cfg, q, recipe, rows):
    """Every logit has a bit-identical twin V / 2 rows away, in another chunk of the row's argmax (score_chunk_kernel / score_merge_kernel): forward
    without logits, forward_runs with k = 4 (topk_*: each twin pair with the lower index first) and generate_greedy's device loop (table_advance_kernel;
    40 rows of a wide batch: runs_advance_kernel) must all prefer the lower index, as sample_argmax's strict `>` does (sampler.rs:29-41)"""
    ref = witness(cfg, q, recipe, ties_positions(cfg, q, recipe, rows))
    twins_rank_in_pairs(ref, ties_positions(cfg, q, recipe, rows))
    V = ref.cfg.vocab_size
    what = f"{ref.cfg.name} q{q} tied, {rows} rows"
    m = L.Transformer(ref.img)
    b = L.Batch(m, 16) if rows == 16 else L.Batch(m, 64, wide=True)
    seqs = populate(b, ref, depths(rows), rows - 1, what)
    am = step(b, seqs, [s.next()[0] for s in seqs], what, logits=False)
    assert int(am.max()) < V // 2, f"{what}: forward picked an upper twin: {am}"
    work = [(seqs[i], seqs[i].next(n), n) for i, n in (zip(RUN_SLOTS, RUN_LENS) if rows == 16 else ((i, wide_run_len(i)) for i in range(rows)))]
    ams, want, (ti, tl) = run_pass(b, work, what, k=4, kv="ends")
    o = 0
    for (s, _, _), rws in zip(work, want):
        for r in rws:
            assert ti[o].tolist() == rank_row(r)[:4].tolist(), f"{what}: slot {s.slot}, output row {o}: top-4 indices {ti[o]}"
            o += 1
    assert o == ti.shape[0] and int(np.concatenate(ams).max()) < V // 2
    greedy_after(L, b, ref, [seqs[i] for i in GEN_SLOTS] if rows == 16 else seqs, what)
    b.close(); m.close()


def softcap_ties_positions(cfg, q, recipe):
    return D16


# Gemma's logit cap covers the first `dim` logits only (transformer.rs:375): at mini-gemma's vocabulary of 4096 the 1792 logits behind them stay in
# the thousands and hold the maximum.  With vocab_size == dim (stress_models.resolve's geometry for tied_classifier) every logit is capped and the
# rows' maxima are the many logits equal to 30.0; both geometries run.
GEMMA_CAPPED = dataclasses.replace(S.CONFIGS["mini-gemma"], name=f"mini-gemma-v{S.CONFIGS['mini-gemma'].dim}", vocab_size=S.CONFIGS["mini-gemma"].dim)
SOFTCAP_TIES = cases("softcap_ties", [(c, q, "softcap") for c in ("mini-gemma", GEMMA_CAPPED) for q in (S.Q8_0, S.Q4_0)], softcap_ties_positions)


def capped_maxima(ref, positions):
    """how many logits of each row sit on the cap, 30.0; where every logit is capped they are the row's tied maxima, at least eight of them"""
    rows = ref.rows[sorted(set(positions))]
    n = (rows == np.float32(30.0)).sum(axis=1)
    assert n.min() >= 2, f"{ref.cfg.name}: a row without two logits on the cap ({n})"
    if ref.cfg.vocab_size <= ref.cfg.dim:
        assert float(rows.max()) == 30.0 and n.min() >= 8, f"{ref.cfg.name}: every row needs eight maxima on the cap ({n})"
    return n


@gpu
@pytest.mark.parametrize("cfg,q,recipe", SOFTCAP_TIES, ids=ident)
def test_saturated_logit_cap_ties(L, cfg, q, recipe):
    """softcap_rows_kernel where tanh rounds to exactly 1: a row holds many logits equal to 30.0 - logits bit for bit, the argmax and the top-8
    indices; in the all-capped geometry those are the first eight of the tied maxima in ascending index order"""
    ref = witness(cfg, q, recipe, D16)
    capped_maxima(ref, D16)
    what = f"{ref.cfg.name} q{q} softcap"
    m = L.Transformer(ref.img); b = L.Batch(m, 16)
    seqs = populate(b, ref, D16, 15, what)
    ams, want, (ti, tl) = run_pass(b, [(s, s.next(), 1) for s in seqs], what, k=8)
    for i, (s, rws) in enumerate(zip(seqs, want)):
        assert ti[i].tolist() == rank_row(rws[0])[:8].tolist(), f"{what}: slot {s.slot}: top-8 indices {ti[i]}"
        if ref.cfg.vocab_size <= ref.cfg.dim:
            assert ti[i].tolist() == np.flatnonzero(rws[0] == np.float32(30.0))[:8].tolist()
    b.close(); m.close()


# ---------------------------------------------------------------------------------------------- 6. sampling on the device

SAMPLED_STEPS = 8
SAMPLED_RUNS = [(0, 1), (1, 4), (2, 1), (3, 7), (4, 3), (5, 2)]               # (slot, run length) of the ragged call; slot 5's run has no sampler


def sampled_positions(cfg, q, recipe):
    return step_positions(D16, SAMPLED_STEPS) + [D16[i] + SAMPLED_STEPS + n - 1 for i, n in SAMPLED_RUNS[:-1]]


SAMPLED = cases("sampled", [("mini-llama", S.Q8_0, "peaked"), ("mini-phi", S.Q8_0, "peaked_mild"), ("mini-gemma", S.Q8_0, "peaked"),
                            ("mini-gemma", S.Q8_0, "softcap"), ("mini-gemma", S.Q4_0, "softcap")], sampled_positions)


@gpu
@pytest.mark.parametrize("cfg,q,recipe", SAMPLED, ids=ident)
def test_batch_sampler_on_stress_logits(L, cfg, q, recipe):
    """batch_sample_*_kernel: forward_sample over 16 rows, eight passes, then one forward_runs_sample; every row keeps one sampler pair of a kind of
    test_batch_sample.KINDS.  The sampled token is compared, not fed back: a row's next input is the shared run's next token, and the reference
    samples from a copy of the run's row (softcap: logits of thousands before the cap, one-hot after the temperature)"""
    ref = witness(cfg, q, recipe, sampled_positions(cfg, q, recipe))
    V = ref.cfg.vocab_size
    what = f"{ref.cfg.name} q{q} {recipe}"
    m = L.Transformer(ref.img); b = L.Batch(m, 16)
    seqs = populate(b, ref, D16, 15, what)
    kinds = [KINDS[i % len(KINDS)] for i in range(16)]
    dev = [L.Sampler(V, k[0], k[1], 1000 + i) for i, k in enumerate(kinds)]
    orc = [O.Sampler(V, k[0], k[1], 1000 + i) for i, k in enumerate(kinds)]
    for k in range(SAMPLED_STEPS):
        pos = [s.n for s in seqs]
        got = b.forward_sample([s.slot for s in seqs], [s.next()[0] for s in seqs], pos, dev)
        want = [orc[i].sample(s.feed(s.next()).copy()) for i, s in enumerate(seqs)]
        assert got.tolist() == want, f"{what} step {k}: tokens {got.tolist()} vs the oracle's {want} (kinds {kinds})"
        if k in (0, SAMPLED_STEPS - 1):
            for s, p in zip(seqs, pos):
                check_slot_rows(b, s, [p], f"{what} step {k}")
    runs = [(i, seqs[i].n, seqs[i].next(n), dev[i] if i != 5 else None) for i, n in SAMPLED_RUNS]
    got = b.forward_runs_sample(runs)
    want = []
    for i, n in SAMPLED_RUNS:
        start, row = seqs[i].n, seqs[i].feed(seqs[i].next(n))
        want.append(orc[i].sample(row.copy()) if i != 5 else 0)
        check_slot_rows(b, seqs[i], run_positions(start, n), f"{what}: the ragged call")
    assert got.tolist() == want, f"{what}: forward_runs_sample {got.tolist()} vs the oracle's {want}"
    b.close(); m.close()


# ---------------------------------------------------------------------------------------------- 7. sinks on a tie

SINK_DEPTHS = [33, 64, 100, 5]      # row 0 masked, row 1 untouched, row 2 under a frequency penalty, row 3 untouched
FREQ = dict(repetition=1.0, presence=0.0, frequency=0.5, out_from=0)


def sinks_positions(cfg, q, recipe):
    return SINK_DEPTHS


SINKS = cases("sinks", [("mini-llama", S.Q8_0, "tied_classifier"), ("mini-phi", S.Q8_0, "tied_classifier")], sinks_positions)


def sink_rows(ref):
    """-> (the lower twins of the four rows' maxima, the mask of row 0, the record of row 2 up to its position, the rows as the sinks leave them)"""
    V = ref.cfg.vocab_size
    twins = [ref_argmax(ref.rows[d]) for d in SINK_DEPTHS]
    mask = ban(V, [twins[0]])
    d = SINK_DEPTHS[2]
    hist = [twins[2]] + [NONE] * (d - 1) + [int(ref.toks[d])]                   # only the lower twin occurs, and the token the pass itself records
    want = [masked(ref.rows[SINK_DEPTHS[0]], mask), ref.rows[SINK_DEPTHS[1]], penalised(ref.rows[d], hist, d, FREQ), ref.rows[SINK_DEPTHS[3]]]
    return twins, mask, hist, want


@gpu
@pytest.mark.parametrize("cfg,q,recipe", SINKS, ids=ident)
def test_sinks_move_a_tie_to_the_upper_twin(L, cfg, q, recipe):
    """mask_rows_kernel and penalty_rows_kernel in front of the argmax: a mask that clears only the lower twin of the row's maximum, and a frequency
    penalty over a record in which only the lower twin occurs, move the argmax to twin + V / 2; the untouched rows of the same pass keep the lower one"""
    ref = witness(cfg, q, recipe, SINK_DEPTHS)
    V = ref.cfg.vocab_size
    what = f"{ref.cfg.name} q{q} tied"
    twins, mask, hist, want = sink_rows(ref)
    m = L.Transformer(ref.img); b = L.Batch(m, 5)
    seqs = populate(b, ref, SINK_DEPTHS + [0], 4, what)[:4]
    b.set_masks([0], mask[None, :])
    b.set_penalties([2], **FREQ)
    b.set_history(2, hist[:-1], 0)
    am, lg = b.forward([0, 1, 2, 3], [s.next()[0] for s in seqs], SINK_DEPTHS, logits=True)
    for i in range(4):
        assert_bit_equal(lg[i], want[i], f"{what}: row {i} at {SINK_DEPTHS[i]}: logits")
        assert int(am[i]) == twins[i] + (V // 2 if i in (0, 2) else 0), f"{what}: row {i}: argmax {am[i]}, the lower twin is {twins[i]}"
    assert b.history(2, SINK_DEPTHS[2] + 1).tolist() == hist
    b.close(); m.close()


# ---------------------------------------------------------------------------------------------- 8. verify_tokens: the skinny GEMM on a context

VERIFY_AT, VERIFY_N = 60, 9


def verify_positions(cfg, q, recipe):
    return range(VERIFY_AT, VERIFY_AT + VERIFY_N)


VERIFY = cases("verify", by_recipe([("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)], ("peaked", "dead_groups", "glu_extremes", "tied_classifier")), verify_positions)


@gpu
@pytest.mark.parametrize("cfg,q,recipe", VERIFY, ids=ident)
def test_verify_tokens_under_stress(L, cfg, q, recipe):
    ref = witness(cfg, q, recipe, verify_positions(cfg, q, recipe))
    what = f"{ref.cfg.name} q{q} {recipe}"
    m = L.Transformer(ref.img)
    assert m.prefill_tokens(ref.toks[:VERIFY_AT], 0) == VERIFY_AT
    am, _ = m.verify_tokens(ref.toks[VERIFY_AT:VERIFY_AT + VERIFY_N], VERIFY_AT)
    assert am.tolist() == [ref_argmax(ref.rows[VERIFY_AT + j]) for j in range(VERIFY_N)], f"{what}: argmax of the nine rows"
    for p in (VERIFY_AT, VERIFY_AT + VERIFY_N - 1):
        for layer in range(ref.cfg.n_layers):
            assert_bit_equal(m.kv_row(0, layer, p), ref.K[layer, p], f"{what}: key row, layer {layer}, pos {p}")
            assert_bit_equal(m.kv_row(1, layer, p), ref.V[layer, p], f"{what}: value row, layer {layer}, pos {p}")
    m.close()


# ---------------------------------------------------------------------------------------------- CPU tier

AGAINST_DECODE = [("mini-llama", S.Q8_0, "peaked"), ("mini-llama", S.Q4_0, "dead_groups"), ("mini-llama3b", S.Q8_0, "combined"),
                  ("mini-phi", S.Q8_0, "glu_extremes"), ("mini-gemma", S.Q8_0, "softcap"), ("mini-gemma", S.Q4_0, "tied_classifier")]


@pytest.mark.parametrize("cfg,q,recipe", AGAINST_DECODE, ids=ident)
def test_the_shared_run_is_the_stress_files_decode(cfg, q, recipe):
    """the per-position counters add up to the whole run's (integers; the scale ratio's maximum is the run's), logits and K/V rows are that run's"""
    ref = oracle_run(cfg, q, recipe)
    img, c, toks, rows, kv, st = oracle_decode(cfg, q, recipe, N)
    assert c == ref.cfg and toks.tolist() == ref.toks.tolist()
    assert_bit_equal(ref.rows, rows, f"{c.name} q{q} {recipe}: logits")
    assert summed(ref.stats) == st
    for (w, l, p), row in kv.items():
        assert_bit_equal((ref.K, ref.V)[w][l, p], row, f"{c.name} q{q} {recipe}: {'kv'[w]} row, layer {l}, pos {p}")


@pytest.mark.parametrize("test,cfg,q,recipe,positions", WITNESSED, ids=lambda v: ident(v) or (f"{len(v)}pos" if isinstance(v, tuple) else None))
def test_every_gpu_case_compares_rows_that_reached_the_regime(test, cfg, q, recipe, positions):
    """what keeps a GPU test from comparing rows that never reached the regime: the recipe's witness over the case's compared positions"""
    ref = witness(cfg, q, recipe, positions)
    if test == "ties":
        twins_rank_in_pairs(ref, positions)
    if test == "softcap_ties":
        capped_maxima(ref, positions)
    if test == "sinks":
        V = ref.cfg.vocab_size
        twins, mask, hist, want = sink_rows(ref)
        for i, d in enumerate(SINK_DEPTHS):
            assert twins[i] < V // 2 and ref_argmax(want[i]) == twins[i] + (V // 2 if i in (0, 2) else 0), f"row {i} at {d}"
        assert hist[-1] % (V // 2) != twins[2], "the token the pass records must not be the maximum's twin"
