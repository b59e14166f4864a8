"""Repetition / presence / frequency penalties on batch slots over the token record the batch keeps on the device (lmrs_batch_set_penalties /
_clear_penalties / _penalty_info / _set_history / _history, include/lmrs_hip.h).  The reference is one CPU oracle PER SEQUENCE; its logits row is penalised
in numpy by penalty_rules.penalised - the header's rule, np.float32 scalars one operation at a time - before Sampler::sample (the oracle's), sample_argmax
(lmrs_ref_argmax) or the top-k definition (tests/test_topk.py).  Every comparison is exact: logits bit for bit, tokens and indices by value; the top-k
log-probabilities by test_topk's own rule."""
import ctypes
import dataclasses

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from penalty_rules import NONE, params, penalised
from test_batch import Seq as TokenSeq
from test_batch_embed import token_rows
from test_batch_mask import DEPTHS16, ban, masked
from test_batch_sample import KINDS, Seq as SampledSeq
from test_topk import rank_row, topk_rule
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
V = 4096


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


class Seq(TokenSeq):
    """test_batch.Seq that also keeps the record the device should hold: hist[i] = the token fed at position i"""

    def __init__(self, img, slot):
        super().__init__(img, slot)
        self.hist, self.par = [], None

    def feed(self, toks):
        self.hist.extend(int(t) for t in toks)
        return super().feed(toks)

    def want(self, tok):
        """feed one token -> (the oracle's row, the row under the sequence's penalties)"""
        row = self.feed([tok])
        return row, penalised(row, self.hist, self.n - 1, self.par)


def alphabet(seed, n=12):
    return np.random.default_rng(seed).choice(V, n, replace=False).astype(np.uint32)


def from_alphabet(alpha, n, seed):
    return alpha[np.random.default_rng(seed).integers(0, alpha.size, n)]


def set_penalties(b, seqs):
    """every sequence's .par (None: cleared) in one set_penalties call and one clear_penalties call; penalty_info says the same"""
    on = [s for s in seqs if s.par is not None]
    if on:
        b.set_penalties([s.slot for s in on], *([s.par[k] for s in on] for k in ("repetition", "presence", "frequency", "out_from")))
    b.clear_penalties([s.slot for s in seqs if s.par is None])
    for s in seqs:
        info = b.penalty_info(s.slot)
        if s.par is None:
            assert not info["active"], (s.slot, info)
        else:
            assert info == dict(active=True, out_from=s.par["out_from"], **{k: float(np.float32(s.par[k])) for k in ("repetition", "presence", "frequency")})


# ---------------------------------------------------------------------------------------------- 1. the record

@gpu
@pytest.mark.parametrize("paged", [False, True])
def test_the_record_follows_every_call_that_writes_kv_rows(L, paged):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=501)
    m = L.Transformer(img)
    b = L.Batch(m, 5, page_len=64, n_pages=24) if paged else L.Batch(m, 5)
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_history: the batch keeps no token record"):
        b.history(0, 1)
    none = lambda n: [NONE] * n
    b.set_history(0)                                                                  # no tokens: only switches the record on
    assert b.history(0, 256).tolist() == none(256) and b.history(4, 256).tolist() == none(256)
    # a prefill (70 tokens: two chunks' worth of pages on the paged batch)
    p0 = S.prompt_tokens(cfg, 70, 502)
    b.prefill(0, p0, 0)
    assert b.history(0, 70).tolist() == p0.tolist() and b.history(0, 5, 70).tolist() == none(5)
    # a ragged pass with two runs
    r0, r1 = [11, 12, 13], [21, 22, 23, 24, 25]
    b.forward_runs([(0, 70, r0, 1), (1, 0, r1, 2)])
    assert b.history(0, 4, 70).tolist() == r0 + [NONE] and b.history(1, 6).tolist() == r1 + [NONE]
    # a forward
    b.forward([1, 0], [31, 32], [5, 73])
    assert b.history(0, 75).tolist() == p0.tolist() + r0 + [32, NONE] and b.history(1, 7).tolist() == r1 + [31, NONE]
    # a fork copies the source's first n_pos entries
    b.set_history(2, [7] * 80)
    b.fork(0, 2, 74)
    assert b.history(2, 80).tolist() == b.history(0, 74).tolist() + [7] * 6
    # generate_greedy: the loop's own tokens are recorded on the device
    out = b.generate_greedy([0, 1, 2], [41, 42, 43], [74, 6, 74], 5)
    for r, (slot, pos, t) in enumerate(((0, 74, 41), (1, 6, 42), (2, 74, 43))):
        assert b.history(slot, 6, pos).tolist() == [t] + out[r, :4].tolist() + [NONE if slot != 2 else 7], (slot, out[r])
    # embedding rows read NONE: prefill_embeddings (several rows, one row) and an embedding run of the ragged pass
    e = m.get_embeddings(S.prompt_tokens(cfg, 7, 503)).reshape(7, -1)
    b.set_history(3, list(range(100, 110)))
    b.prefill_embeddings(3, e[:4], 0)
    assert b.history(3, 10).tolist() == none(4) + list(range(104, 110))
    b.prefill_embeddings(3, e[4:5], 5)
    assert b.history(3, 10).tolist() == none(4) + [104, NONE] + list(range(106, 110))
    b.forward_runs([(3, 6, e[5:7], 1), (4, 0, [51, 52], 0)])
    assert b.history(3, 10).tolist() == none(4) + [104, NONE, NONE, NONE, 108, 109] and b.history(4, 3).tolist() == [51, 52, NONE]
    # a fork from the context's own cache: unknown tokens
    b.fork(L.BATCH_CTX, 1, 4)
    assert b.history(1, 7).tolist() == none(4) + r1[4:] + [31, 42]
    # a prompt long enough for block attention on the paged batch (130 rows), behind a prefix
    p4 = S.prompt_tokens(cfg, 130, 504)
    b.prefill(4, p4, 2)
    assert b.history(4, 133).tolist() == [51, 52] + p4.tolist() + [NONE]
    # set_history with NONE entries, read back in part
    b.set_history(4, [NONE, 5, NONE], 1)
    assert b.history(4, 5).tolist() == [51, NONE, 5, NONE, int(p4[2])]
    b.close()


@gpu
def test_a_wide_step_records_every_row(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=505)
    m = L.Transformer(img); b = L.Batch(m, 20, wide=True)
    b.set_history(0)
    toks = [(37 * i + 5) % V for i in range(20)]
    pos = [(0, 3, 1)[i % 3] for i in range(20)]
    b.forward(list(range(20)), toks, pos)
    for i in range(20):
        assert b.history(i, 5).tolist() == [NONE] * pos[i] + [toks[i]] + [NONE] * (4 - pos[i]), i
    b.close()


# ---------------------------------------------------------------------------------------------- 2. forward

FORWARD_KINDS = ["boost", "rep", "freq", "boost", "all", "boost", "sink", None, "boost", "freq", "boost", "all", "boost", None, "rep", "boost"]


def forward_case(cfg, q):
    """the oracle side of test_forward_rows_under_penalties, GPU-free: image, sequences prefilled with prompts over a 12-token alphabet, and per step the
    rows, their input tokens, the oracle's rows and the penalised rows"""
    img = S.build_image(cfg, q, seed=511)
    alpha = alphabet(512)
    seqs, prompts = [], []
    for i, n in enumerate(DEPTHS16):
        s = Seq(img, i)
        s.par = params(FORWARD_KINDS[i], out_from=n // 2 if FORWARD_KINDS[i] == "freq" else None)
        prompts.append(from_alphabet(alpha, n, 513 + i))
        if n:
            s.feed(prompts[i])
        seqs.append(s)
    toks = [int(alpha[(5 * i + 1) % 12]) for i in range(16)]
    steps = []
    for step, order in enumerate((list(range(16)), list(range(15, -1, -1))[:11])):
        rows = [seqs[i] for i in order]
        pos = [s.n for s in rows]
        fed = [toks[s.slot] for s in rows]
        want = [s.want(toks[s.slot]) for s in rows]
        steps.append((rows, pos, fed, want))
        for s, (_, pen) in zip(rows, want):
            toks[s.slot] = ref_argmax(pen)
    return img, seqs, prompts, steps


def boost_changes(steps):
    """over the first step's boost rows: (rows whose unpenalised argmax is outside the record, those of them whose argmax the penalty changed)"""
    rows, pos, fed, want = steps[0]
    outside = [s.slot for s, p, (row, pen) in zip(rows, pos, want) if FORWARD_KINDS[s.slot] == "boost" and ref_argmax(row) not in s.hist[:p + 1]]
    changed = [s.slot for s, (row, pen) in zip(rows, want) if s.slot in outside and ref_argmax(pen) != ref_argmax(row)]
    return outside, changed


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_forward_rows_under_penalties(L, cfg, q):
    """16 rows at the depths the attention forms change at, penalised and unpenalised rows in one pass (mini-gemma: the soft cap in front of the penalty); a
    second batch on the same model that never had penalties or a record gives the unpenalised rows' bits"""
    img, seqs, prompts, steps = forward_case(cfg, q)
    m = L.Transformer(img)
    b, plain = L.Batch(m, 16), L.Batch(m, 16)
    set_penalties(b, seqs)                                                            # before the prefills: the record is on
    for i, n in enumerate(DEPTHS16):
        if n:
            b.prefill(i, prompts[i], 0); plain.prefill(i, prompts[i], 0)
    outside, changed = boost_changes(steps)
    # the oracle alone: boost makes the argmax a token of the record, so it changes wherever the unpenalised argmax is none - 7 of mini-llama's 16 rows.
    # mini-gemma's embedding table is its classifier: the unpenalised argmax of every row is the row's own input token (its logit ~17 against ~4 for the
    # runner-up), which the record holds by definition - no row of it can meet the condition, whatever the seeds; there the sink row shows a changed argmax
    assert outside == changed, (outside, changed)
    assert len(changed) >= 4 if cfg == "mini-llama" else outside == [], (cfg, outside, changed)
    for step, (rows, pos, fed, want) in enumerate(steps):
        slots = [s.slot for s in rows]
        am, lg = b.forward(slots, fed, pos, logits=True)
        am0, lg0 = plain.forward(slots, fed, pos, logits=True)
        for i, s in enumerate(rows):
            what = f"{cfg} q{q} step {step} row {i} (slot {s.slot}, pos {pos[i]}, {FORWARD_KINDS[s.slot]})"
            row, pen = want[i]
            assert_bit_equal(lg[i], pen, f"{what}: logits")
            assert int(am[i]) == ref_argmax(pen), f"{what}: argmax {am[i]} vs {ref_argmax(pen)}"
            assert_bit_equal(lg0[i], row, f"{what}: the batch without penalties")
            if s.par is None:
                assert_bit_equal(lg[i], lg0[i], f"{what}: an unpenalised row beside penalised ones")
                assert int(am[i]) == int(am0[i]), what
            elif FORWARD_KINDS[s.slot] == "boost":
                assert int(am[i]) in s.hist[:pos[i] + 1], f"{what}: the boosted argmax is no token of the record"
                if step == 0 and s.slot in outside:
                    assert int(am[i]) != int(am0[i]), f"{what}: the boost did not change the argmax"
            elif FORWARD_KINDS[s.slot] == "sink" and int(am0[i]) in s.hist[:pos[i] + 1]:
                assert int(am[i]) != int(am0[i]), f"{what}: the sink left a token of the record the argmax"      # (1e4 a count against logits of tens)
            assert b.history(s.slot, pos[i] + 1).tolist() == s.hist[:pos[i] + 1], what
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_history: the batch keeps no token record"):
        plain.history(0, 1)
    b.close(); plain.close()


# ---------------------------------------------------------------------------------------------- 3. order with masks

@gpu
def test_the_mask_is_applied_behind_the_penalty(L):
    cfg = "mini-gemma"
    img = S.build_image(cfg, S.Q4_0, seed=521)
    m = L.Transformer(img); b = L.Batch(m, 2)
    alpha = alphabet(522)
    seqs = [Seq(img, 0), Seq(img, 1)]
    seqs[0].par = params("all"); seqs[1].par = params("boost")
    set_penalties(b, seqs)
    for s, n in zip(seqs, (9, 70)):
        p = from_alphabet(alpha, n, 523 + s.slot)
        b.prefill(s.slot, p, 0); s.feed(p)
    pos = [s.n for s in seqs]
    want = [s.want(int(alpha[3])) for s in seqs]
    masks = [ban(V, [ref_argmax(pen), ref_argmax(row), 17]) for row, pen in want]     # the ban-list holds the PENALISED argmax (and the oracle's own)
    b.set_masks([0, 1], np.stack(masks))
    am, lg = b.forward([0, 1], [int(alpha[3])] * 2, pos, logits=True)
    for i, (row, pen) in enumerate(want):
        exp = masked(pen, masks[i])
        assert_bit_equal(lg[i], exp, f"slot {i}: the penalised row with -inf at the cleared bits")
        assert int(am[i]) == ref_argmax(exp) != ref_argmax(pen)
        assert np.array_equal(np.isneginf(lg[i]), ~masks[i])
    b.close()


# ---------------------------------------------------------------------------------------------- 4. forward_runs: every row of a run an output

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_every_row_of_a_run_sees_the_record_up_to_its_own_position(L, cfg, q):
    """the draft-verification shape: runs of 1, 5 and 16 tokens behind 0, 60 and 130 cached positions, all rows outputs, logits and the 8 first candidates per
    row.  The 16-token run ends with a token that occurs nowhere before: only its last row may show it penalised"""
    img = S.build_image(cfg, q, seed=531)
    m = L.Transformer(img); b = L.Batch(m, 3)
    alpha = alphabet(532)
    late = int(next(t for t in range(100, V) if t not in set(alpha.tolist())))
    seqs = [Seq(img, i) for i in range(3)]
    for s, kind in zip(seqs, ("rep", "freq", "all")):
        s.par = params(kind, out_from=58 if kind == "freq" else None)
    set_penalties(b, seqs)
    for s, n in zip(seqs, (0, 60, 130)):
        if n:
            p = from_alphabet(alpha, n, 533 + s.slot)
            b.prefill(s.slot, p, 0); s.feed(p)
    runs = [from_alphabet(alpha, n, 540 + i).tolist() for i, n in enumerate((1, 5, 16))]
    runs[2][-1] = late
    start = [s.n for s in seqs]
    want = [[s.want(t) for t in run] for s, run in zip(seqs, runs)]
    am, lg, ti, tl = b.forward_runs([(s.slot, start[s.slot], runs[s.slot], len(runs[s.slot])) for s in seqs], k=8, logits=True)
    o = 0
    for s, run, w in zip(seqs, runs, want):
        for j, (row, pen) in enumerate(w):
            where = f"{cfg} q{q}: slot {s.slot} row {j} of {len(run)} (output {o})"
            assert_bit_equal(lg[o], pen, f"{where}: logits")
            assert int(am[o]) == ref_argmax(pen), where
            assert ti[o].tolist() == rank_row(pen)[:8].tolist(), f"{where}: top-8 indices"
            with np.errstate(all="ignore"):
                topk_rule(tl[o:o + 1], ti[o:o + 1], pen[None, :], where)
            if s.slot == 2:                                                           # row j sees positions <= start + j only
                same = lg[o, late].view(np.uint32) == row[late].view(np.uint32)
                assert same == (j < len(run) - 1), f"{where}: the late token's logit {lg[o, late]} against the oracle's unpenalised {row[late]}"
            o += 1
    assert o == am.size == 22
    b.close()


# ---------------------------------------------------------------------------------------------- 5. generate_greedy

GREEDY_KINDS = ["sink", "all", "rep", "freq", None]


def greedy_case(L, b, img, cfg, depths, n_new, what):
    n = len(depths)
    alpha = alphabet(552)
    seqs = []
    for i, d in enumerate(depths):
        s = Seq(img, i)
        kind = GREEDY_KINDS[i % 5]
        s.par = params(kind, out_from=d if kind in ("sink", "freq") else None)       # sink / freq: from the prompt's end on
        seqs.append(s)
    set_penalties(b, seqs)
    for s, d in zip(seqs, depths):
        if d:
            p = from_alphabet(alpha, d, 553 + s.slot)
            b.prefill(s.slot, p, 0); s.feed(p)
    toks = [int(alpha[(3 * i + 2) % 12]) for i in range(n)]
    got = b.generate_greedy(list(range(n)), toks, depths, n_new)
    for i, s in enumerate(seqs):
        t = toks[i]
        for j in range(n_new):
            t = ref_argmax(s.want(t)[1])
            assert int(got[i, j]) == t, f"{what}: row {i} ({GREEDY_KINDS[i % 5]}) step {j}: {got[i, j]} vs the oracle loop's {t}"
        if GREEDY_KINDS[i % 5] == "sink":
            assert len(set(got[i].tolist()) | {toks[i]}) == n_new + 1, f"{what}: row {i}: a generated token repeats under the sink: {got[i].tolist()}"
        assert b.history(i, n_new, depths[i]).tolist() == [toks[i]] + got[i, :-1].tolist(), f"{what}: row {i}: the record of the loop's tokens"


@gpu
@pytest.mark.parametrize("form", ["rows", "wide", "paged"])
def test_generate_greedy_under_penalties(L, form):
    """24 steps: 5 rows through the row table, 20 rows through the long table, and a paged batch whose rows cross a page edge at positions 60 .. 84"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=551)
    m = L.Transformer(img)
    if form == "rows":
        b, depths = L.Batch(m, 5), [9, 0, 64, 1, 30]
    elif form == "wide":
        b, depths = L.Batch(m, 20, wide=True), [(0, 1, 7, 30, 2)[i % 5] + i // 5 for i in range(20)]
    else:
        b, depths = L.Batch(m, 5, page_len=64, n_pages=12), [60, 60, 58, 61, 60]
    greedy_case(L, b, img, cfg, depths, 24, form)
    b.close()


# ---------------------------------------------------------------------------------------------- 6. the sampled passes

@gpu
def test_sampled_passes_under_penalties(L):
    """forward_sample and forward_runs_sample, the six sampler kinds (argmax, sample_mult, peaked and flat top-p) under "all": each token is what the oracle's
    sampler gives on the penalised row"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=561)
    m = L.Transformer(img); b = L.Batch(m, 6)
    alpha = alphabet(562)
    par = params("all")
    b.set_penalties(list(range(6)), **par)
    seqs, hist = [], {}
    for i in range(6):
        s = SampledSeq(L, img, i, KINDS[i], 5600 + i)
        p = from_alphabet(alpha, (4, 0, 9, 17, 2, 33)[i], 563 + i)
        if p.size:
            b.prefill(i, p, 0); s.feed(p)
        hist[i] = p.tolist()
        seqs.append(s)
    last = {i: int(alpha[i]) for i in range(6)}
    for k, wide in enumerate((False, True, False, True)):
        rows = seqs if k % 2 == 0 else seqs[::-1]
        if wide:
            got = b.forward_runs_sample([(s.slot, s.n, [last[s.slot]], s.dev) for s in rows])
        else:
            got = b.forward_sample([s.slot for s in rows], [last[s.slot] for s in rows], [s.n for s in rows], [s.dev for s in rows])
        want = []
        for s in rows:
            hist[s.slot].append(last[s.slot])
            lg = penalised(s.feed([last[s.slot]]), hist[s.slot], s.n - 1, par)
            want.append(s.ref.sample(lg))
        assert got.tolist() == want, f"call {k}: tokens {got.tolist()} vs the oracle's {want}"
        for s, t in zip(rows, got.tolist()):
            last[s.slot] = t
    b.close()


# ---------------------------------------------------------------------------------------------- 7. deep

@gpu
def test_a_record_of_2048_tokens(L):
    """mini-llama-long: a slot at position 2047 whose record holds 2048 tokens over a 300-token alphabet - the full-length sort - and one at position 1024
    (the same sequence's prefix, so one oracle serves both)"""
    cfg = "mini-llama-long"
    img = S.build_image(cfg, S.Q8_0, seed=571)
    m = L.Transformer(img); b = L.Batch(m, 2)
    toks = from_alphabet(alphabet(572, 300), 2048, 573)
    pars = [params("all"), params("freq", out_from=512)]
    b.set_penalties([0, 1], *([p[k] for p in pars] for k in ("repetition", "presence", "frequency", "out_from")))
    b.prefill(0, toks[:2047], 0); b.prefill(1, toks[:1024], 0)
    orc = O.Oracle(img)
    rows = {}
    for i, t in enumerate(toks):
        lg = orc.forward(int(t), i)
        if i in (1024, 2047):
            rows[i] = lg.copy()
    am, lg = b.forward([0, 1], [int(toks[2047]), int(toks[1024])], [2047, 1024], logits=True)
    for r, (p, par) in enumerate(zip((2047, 1024), pars)):
        pen = penalised(rows[p], toks.tolist(), p, par)
        # (513 draws from 300 tokens behind out_from = 512 leave about 246 distinct ones; 2048 draws nearly all 300)
        assert (pen.view(np.uint32) != rows[p].view(np.uint32)).sum() >= 200, "the penalty should touch most of the alphabet"
        assert_bit_equal(lg[r], pen, f"position {p}: logits")
        assert int(am[r]) == ref_argmax(pen)
    b.close()


# ---------------------------------------------------------------------------------------------- 8. state

@gpu
def test_penalty_state(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=581)
    m = L.Transformer(img); b = L.Batch(m, 3)
    alpha = alphabet(582)
    seqs = [Seq(img, i) for i in range(3)]
    # prefills BEFORE the record exists: the device does not know these tokens
    early = [from_alphabet(alpha, n, 583 + i) for i, n in enumerate((6, 3, 0))]
    for s, p in zip(seqs, early):
        if p.size:
            b.prefill(s.slot, p, 0); s.feed(p)
    assert b.penalty_info(0) == dict(repetition=1.0, presence=0.0, frequency=0.0, out_from=0, active=False)
    for s in seqs:
        s.par = params("all", out_from=1)
    set_penalties(b, seqs)
    assert b.history(0, 6).tolist() == [NONE] * 6
    b.set_history(1, early[1])                                                        # slot 1's caller supplies them; slot 0's stay unknown
    known = {0: [NONE] * 6, 1: early[1].tolist(), 2: []}

    def step(what):
        pos = [s.n for s in seqs]
        toks = [int(alpha[(2 * s.slot + pos[s.slot]) % 12]) for s in seqs]
        am, lg = b.forward([0, 1, 2], toks, pos, logits=True)
        for i, s in enumerate(seqs):
            row = s.feed([toks[i]])
            known[i].append(toks[i])
            pen = penalised(row, known[i], pos[i], s.par)
            assert_bit_equal(lg[i], pen, f"{what}: slot {i}")
            assert int(am[i]) == ref_argmax(pen), f"{what}: slot {i}"
            if s.par is None:
                assert_bit_equal(lg[i], row, f"{what}: slot {i} without penalties")
            assert b.history(i, pos[i] + 1).tolist() == known[i], f"{what}: slot {i}"
        return lg

    lg = step("penalties set after the prefills")
    # slot 0 saw NONE for its prompt: only its own input token is penalised
    assert (lg[0].view(np.uint32) != seqs[0].orc.forward(known[0][-1], 6).view(np.uint32)).sum() <= 1
    b.set_history(0, early[0])
    known[0][:6] = early[0].tolist()
    step("after set_history")
    # a replacement, (1, 0, 0) = clearing, clear_penalties per slot and for all
    seqs[0].par = params("freq", out_from=2); seqs[1].par = None
    b.set_penalties([0, 1], [1.0, 1.0], [0.2, 0.0], [0.7, 0.0], [2, 5])
    assert b.penalty_info(1) == dict(repetition=1.0, presence=0.0, frequency=0.0, out_from=5, active=False)
    assert b.penalty_info(0)["active"] and b.penalty_info(0)["out_from"] == 2
    step("slot 0 replaced, slot 1 at (1, 0, 0)")
    seqs[2].par = None
    b.clear_penalties([2])
    step("after clear_penalties([2])")
    seqs[0].par = None
    b.clear_penalties()
    assert not any(b.penalty_info(i)["active"] for i in range(3))
    step("after clear_penalties()")                                                   # the unpenalised bits again; the record goes on
    b.close()


@gpu
def test_refusals_come_before_any_change_and_leave_everything_usable(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=591)
    m = L.Transformer(img); b = L.Batch(m, 3)
    lib = L.lib()
    alpha = alphabet(592)
    seqs = [Seq(img, i) for i in range(3)]
    seqs[1].par = params("all")
    set_penalties(b, seqs)
    for s, n in zip(seqs, (2, 5, 1)):
        p = from_alphabet(alpha, n, 593 + s.slot)
        b.prefill(s.slot, p, 0); s.feed(p)
    info1 = b.penalty_info(1)

    def valid(what):
        pos = [s.n for s in seqs]
        toks = [int(alpha[(pos[i] + i) % 12]) for i in range(3)]
        am, lg = b.forward([0, 1, 2], toks, pos, logits=True)
        for i, s in enumerate(seqs):
            row, pen = s.want(toks[i])
            assert_bit_equal(lg[i], pen, f"{what}: slot {i}")
            assert b.history(i, s.n).tolist() == s.hist, f"{what}: slot {i}"
        assert b.penalty_info(1) == info1 and not b.penalty_info(0)["active"], what

    u32 = lambda *v: np.array(v, np.uint32)
    f32 = lambda *v: np.array(v, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    one, zero, s17 = f32(*[1.5] * 17), f32(*[0.0] * 17), np.arange(17, dtype=np.uint32)
    z17 = np.zeros(17, np.uint32)
    sp = lambda n, slot, r=one, pr=zero, fr=zero, of=z17: lib.lmrs_batch_set_penalties(b._h, n, p(slot), p(r), p(pr), p(fr), p(of))
    out = np.zeros(8, np.uint32)
    fl, ui, ii = ctypes.c_float(), ctypes.c_uint32(), ctypes.c_int()
    R = ctypes.byref
    valid("first")
    cases = [
        (lambda: lib.lmrs_batch_set_penalties(None, 1, p(u32(0)), p(one), p(zero), p(zero), p(z17)), "lmrs_batch_set_penalties: NULL argument"),
        (lambda: sp(1, None), "lmrs_batch_set_penalties: NULL array"),
        (lambda: sp(1, u32(0), r=None), "lmrs_batch_set_penalties: NULL array"),
        (lambda: sp(1, u32(0), of=None), "lmrs_batch_set_penalties: NULL array"),
        (lambda: sp(17, s17), "lmrs_batch_set_penalties: n = 17 exceeds the batch's width of 16"),
        (lambda: sp(2, u32(0, 3)), "lmrs_batch_set_penalties: penalty 1: slot 3 of 3"),
        (lambda: sp(2, u32(2, 2)), "lmrs_batch_set_penalties: slot 2 appears twice"),
        (lambda: sp(2, u32(0, 2), r=f32(1.5, np.nan)), "lmrs_batch_set_penalties: penalty 1: slot 2: a value is not finite"),
        (lambda: sp(2, u32(0, 2), pr=f32(np.inf, 0)), "lmrs_batch_set_penalties: penalty 0: slot 0: a value is not finite"),
        (lambda: sp(2, u32(0, 2), fr=f32(0, -np.inf)), "lmrs_batch_set_penalties: penalty 1: slot 2: a value is not finite"),
        (lambda: sp(2, u32(0, 2), r=f32(1.5, 0.0)), "lmrs_batch_set_penalties: penalty 1: slot 2: repetition = 0.000000 is not above 0"),
        (lambda: sp(1, u32(0), r=f32(-2.0)), "lmrs_batch_set_penalties: penalty 0: slot 0: repetition = -2.000000 is not above 0"),
        (lambda: sp(2, u32(0, 2), of=u32(256, 257)), "lmrs_batch_set_penalties: penalty 1: slot 2: out_from = 257 exceeds seq_len = 256"),
        (lambda: lib.lmrs_batch_clear_penalties(None, 0, None), "lmrs_batch_clear_penalties: NULL argument"),
        (lambda: lib.lmrs_batch_clear_penalties(b._h, 1, None), "lmrs_batch_clear_penalties: NULL array"),
        (lambda: lib.lmrs_batch_clear_penalties(b._h, 17, p(s17)), "lmrs_batch_clear_penalties: n = 17 exceeds the batch's width of 16"),
        (lambda: lib.lmrs_batch_clear_penalties(b._h, 1, p(u32(3))), "lmrs_batch_clear_penalties: penalty 0: slot 3 of 3"),
        (lambda: lib.lmrs_batch_clear_penalties(b._h, 2, p(u32(1, 1))), "lmrs_batch_clear_penalties: slot 1 appears twice"),
        (lambda: lib.lmrs_batch_penalty_info(None, 0, R(fl), R(fl), R(fl), R(ui), R(ii)), "lmrs_batch_penalty_info: NULL argument"),
        (lambda: lib.lmrs_batch_penalty_info(b._h, 0, R(fl), R(fl), R(fl), R(ui), None), "lmrs_batch_penalty_info: NULL argument"),
        (lambda: lib.lmrs_batch_penalty_info(b._h, 3, R(fl), R(fl), R(fl), R(ui), R(ii)), "lmrs_batch_penalty_info: slot 3 of 3"),
        (lambda: lib.lmrs_batch_set_history(None, 0, 0, p(out), 1), "lmrs_batch_set_history: NULL argument"),
        (lambda: lib.lmrs_batch_set_history(b._h, 0, 0, None, 1), "lmrs_batch_set_history: NULL array"),
        (lambda: lib.lmrs_batch_set_history(b._h, 3, 0, p(out), 1), "lmrs_batch_set_history: slot 3 of 3"),
        (lambda: lib.lmrs_batch_set_history(b._h, 0, 250, p(out), 7), "lmrs_batch_set_history: start_pos + n = 257 exceeds seq_len = 256"),
        (lambda: lib.lmrs_batch_set_history(b._h, 0, 257, p(out), 0), "lmrs_batch_set_history: start_pos + n = 257 exceeds seq_len = 256"),
        (lambda: lib.lmrs_batch_set_history(b._h, 0, 0, p(u32(1, V, 2)), 3), "lmrs_batch_set_history: token 1 out of range"),
        (lambda: lib.lmrs_batch_history(None, 0, 0, 1, p(out)), "lmrs_batch_history: NULL argument"),
        (lambda: lib.lmrs_batch_history(b._h, 0, 0, 1, None), "lmrs_batch_history: NULL array"),
        (lambda: lib.lmrs_batch_history(b._h, 3, 0, 1, p(out)), "lmrs_batch_history: slot 3 of 3"),
        (lambda: lib.lmrs_batch_history(b._h, 0, 250, 7, p(out)), "lmrs_batch_history: start_pos + n = 257 exceeds seq_len = 256"),
    ]
    for fn, msg in cases:
        assert fn() != 0, msg
        assert lib.lmrs_last_error().decode().startswith(msg), (msg, lib.lmrs_last_error().decode())
        valid(f"after {msg!r}")
    # the Python wrapper's own checks
    with pytest.raises(L.LmrsError, match="repetition must be a scalar or hold one value per slot"):
        b.set_penalties([0, 1], repetition=[1.0, 2.0, 3.0])
    with pytest.raises(L.LmrsError, match="out_from must hold whole numbers"):
        b.set_penalties([0], out_from=-1)
    valid("last")
    b.close()


@gpu
def test_a_vocabulary_with_an_unwritten_tail_has_no_penalties(L):
    """vocabulary 4098 (Q8_0): the classifier writes 4096 of the 4098 logits - set_masks refuses such a batch and so does set_penalties; the record alone is
    served, and the batch goes on unpenalised"""
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-v4098", vocab_size=4098)
    img = S.build_image(cfg, S.Q8_0, seed=595)
    m = L.Transformer(img); b = L.Batch(m, 2)
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_set_penalties: the classifier leaves the last vocab_size % 4 logits unwritten"):
        b.set_penalties([0], repetition=1.3)
    assert not b.penalty_info(0)["active"]
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_history: the batch keeps no token record"):
        b.history(0, 1)
    s = TokenSeq(img, 0)
    am, lg = b.forward([0], [5], [0], logits=True)
    assert_bit_equal(lg[0], s.feed([5]), "slot 0 after the refusal")
    b.set_history(0, [4097, NONE])
    assert b.history(0, 3).tolist() == [4097, NONE, NONE]
    b.close()
