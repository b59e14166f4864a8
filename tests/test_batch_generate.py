"""lmrs_batch_generate (include/lmrs_hip.h): the batch's device loop whose rows end one by one - stop sets, budgets, samplers, log-probabilities.  The
reference is one CPU oracle PER SEQUENCE running the sequential forward; its row is penalised (penalty_rules.penalised) and masked (test_batch_mask.masked)
in numpy, the token chosen by lmrs_ref_argmax or the oracle's Sampler, and the loop's control is the stop rule written out below (ref_generate).  Tokens,
counts and codes are compared by value, K/V rows and logits bit for bit, log-probabilities within one f32 ulp of a float64 log-softmax of that row."""
import ctypes
import dataclasses

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, assert_within_one_ulp, log_softmax64, ref_argmax
from penalty_rules import params, penalised
from test_batch import check_slot_rows, snapshot
from test_batch_mask import ban, masked
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
BUDGET, STOP, STOP_MAX = 0, 1, 16
V = 4096


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def ref_generate(step, t0, budget, stop):
    """the contract's loop for one row: step(t) feeds t at the row's next position and returns the chosen token -> (outputs, finish code)"""
    out, t = [], t0
    while True:
        o = step(t)
        out.append(o)
        if o in stop:
            return out, STOP                                   # STOP wins over BUDGET; the stop token is reported and never fed
        if len(out) == budget:
            return out, BUDGET
        t = o


def rounds(n_out, ce):
    """the passes a row that ends after n_out tokens spends in the table when the host looks every ce passes"""
    return -(-n_out // ce) * ce


class Row:
    """one sequence: its slot, its own oracle, the record the device should hold, its penalties, mask and sampler (kind = (temperature, top_p, seed) or None)"""

    def __init__(self, L, img, slot, kind=None, par=None, mask=None, share=None):
        self.slot, self.orc, self.n, self.hist, self.par, self.mask, self.kind = slot, O.Oracle(img), 0, [], par, mask, kind
        self.dev = self.ref = None
        if share is not None:
            self.dev, self.ref, self.kind = share.dev, share.ref, share.kind
        elif kind is not None:
            self.dev, self.ref = L.Sampler(V, kind[0], kind[1], kind[2]), O.Sampler(V, kind[0], kind[1], kind[2])

    def feed(self, tok):
        """the oracle's forward of tok at the sequence's end -> the row as the sinks see it"""
        del self.hist[self.n:]
        self.hist.append(int(tok))
        row = self.orc.forward(int(tok), self.n).copy()
        self.n += 1
        return masked(penalised(row, self.hist, self.n - 1, self.par), self.mask)

    def choose(self, row):
        return self.ref.sample(row.copy()) if self.ref is not None else ref_argmax(row)

    def prefill(self, b, toks):
        if len(toks):
            b.prefill(self.slot, toks, self.n)
        for t in toks:
            self.feed(t)

    def continuation(self, t0, steps):
        """steps free-running steps from the sequence's end -> (tokens, the rows they were chosen from); the sequence's end moves on"""
        out, rows, t = [], [], t0
        for _ in range(steps):
            rows.append(self.feed(t))
            t = self.choose(rows[-1])
            out.append(t)
        return out, rows

    def rewind(self, n):
        self.n = n


def unused(outs, k, start=V - 1):
    """k tokens none of the given sequences holds"""
    have, got, t = set(int(x) for o in outs for x in o), [], start
    while len(got) < k:
        if t not in have:
            got.append(t)
        t -= 1
    return got


def expect(rows, firsts, conts, budgets, stops):
    """the stop rule over every row's free-running continuation -> (tokens, finish) per row; the rule must consume the continuation in order"""
    want = []
    for i in range(len(rows)):
        it, fed = iter(conts[i]), [firsts[i]]

        def step(t, it=it, fed=fed):
            assert t == fed[-1], "the rule feeds what it chose last"
            o = next(it)
            fed.append(o)
            return o
        want.append(ref_generate(step, firsts[i], budgets[i], set(stops[i])))
    return want


def not_vacuous(want, ces, frozen=2):
    n_out = [len(w[0]) for w in want]
    assert len(set(n_out)) >= 3, f"fewer than three different finishing steps: {n_out}"
    assert {w[1] for w in want} == {BUDGET, STOP}, "a finish code is missing"
    assert any(rounds(k, ce) - k >= frozen for k in n_out for ce in ces), f"no row stays frozen for {frozen} passes inside a chunk"


def check_call(b, rows, firsts, pos, budgets, stops, want, ce, what, samplers=None, logprobs=False):
    got = b.generate([r.slot for r in rows], firsts, pos, budgets, stop=stops, samplers=samplers, check_every=ce, logprobs=logprobs)
    toks, fin, stats = got[0], got[1], got[-1]
    for i, (w, f) in enumerate(want):
        assert toks[i].tolist() == w, f"{what}: row {i} (slot {rows[i].slot} from {pos[i]}): tokens {toks[i].tolist()} vs {w}"
        assert int(fin[i]) == f, f"{what}: row {i}: finish {fin[i]} vs {f}"
    n_out = [len(w[0]) for w in want]
    assert stats["passes"] == max(rounds(k, ce) for k in n_out), f"{what}: passes {stats}"
    assert stats["row_passes"] == sum(rounds(k, ce) for k in n_out), f"{what}: row passes {stats}"
    return got


# ---------------------------------------------------------------------------------------------- 1. stops and budgets, short table

DEPTHS = [65, 0, 128, 63, 200]
BUDGETS = [1, 2, 7, 12, 12]
FIRSTS = [3, 400, 77, 1000, 21]
BEHIND = 14


def five_rows(L, cfg, q, seed=601):
    """the model, a batch with the record on, five rows at DEPTHS with 14 other tokens behind each depth, their snapshots, continuations and stop sets"""
    img = S.build_image(cfg, q, seed=seed)
    m = L.Transformer(img); b = L.Batch(m, 5)
    b.set_history(0)
    gemma = cfg == "mini-gemma"
    rows = [Row(L, img, i, par=params("sink") if gemma and i else None) for i in range(5)]      # (Gemma's row 0 unpenalised: it stops on its own echo)
    pen = [r for r in rows if r.par]
    if pen:
        b.set_penalties([r.slot for r in pen], frequency=[r.par["frequency"] for r in pen])
    others, snaps = [], []
    for i, r in enumerate(rows):
        r.prefill(b, S.prompt_tokens(cfg, DEPTHS[i], seed + 1 + i))
        others.append(S.prompt_tokens(cfg, BEHIND, seed + 11 + i))
        b.prefill(r.slot, others[i], DEPTHS[i])
        snaps.append(snapshot(b, r.slot, range(DEPTHS[i], DEPTHS[i] + BEHIND), m.args.n_layers))
    conts = [r.continuation(FIRSTS[i], 12) for i, r in enumerate(rows)]
    outs = [c[0] for c in conts]
    stops = [[outs[0][0]], [], [outs[2][4]] + unused(outs, 2), [outs[3][9]], unused(outs, STOP_MAX, V - 100)]
    assert outs[2].index(outs[2][4]) == 4 and outs[3].index(outs[3][9]) == 9, "the stop tokens occur earlier in the oracle's own sequences"
    return m, b, rows, others, snaps, conts, stops


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_stops_and_budgets(L, cfg, q):
    m, b, rows, others, snaps, conts, stops = five_rows(L, cfg, q)
    want = expect(rows, FIRSTS, [c[0] for c in conts], BUDGETS, stops)
    assert [(len(w[0]), w[1]) for w in want] == [(1, STOP), (2, BUDGET), (5, STOP), (10, STOP), (12, BUDGET)]
    ces = (1, 3, 16)
    not_vacuous(want, ces)
    nl = m.args.n_layers
    for ce in ces:
        what = f"{cfg} q{q} check_every {ce}"
        check_call(b, rows, FIRSTS, DEPTHS, BUDGETS, stops, want, ce, what)
        for i, r in enumerate(rows):
            k = len(want[i][0])
            check_slot_rows(b, r, sorted({DEPTHS[i], DEPTHS[i] + k - 1}), what)
            assert b.history(r.slot, k, DEPTHS[i]).tolist() == [FIRSTS[i]] + want[i][0][:-1], f"{what}: the record of row {i}'s own positions"
            # the rows BEHIND the end: K/V bits and the record as the prefill left them
            now = snapshot(b, r.slot, range(DEPTHS[i], DEPTHS[i] + BEHIND), nl)
            for j, (x, y) in enumerate(zip(snaps[i], now)):
                if (j // 2) % BEHIND >= k:
                    assert_bit_equal(y, x, f"{what}: row {i}: a K/V row at or beyond pos + n_out changed")
            assert b.history(r.slot, BEHIND - k, DEPTHS[i] + k).tolist() == others[i][k:].tolist(), f"{what}: row {i}: the record beyond pos + n_out changed"
    # the state is a sequence's state: one forward feeds each row's last output at pos + n_out
    for i, r in enumerate(rows):
        r.rewind(DEPTHS[i] + len(want[i][0]))
    pos = [r.n for r in rows]
    am, lg = b.forward([r.slot for r in rows], [w[0][-1] for w in want], pos, logits=True)
    for i, r in enumerate(rows):
        row = r.feed(want[i][0][-1])
        assert_bit_equal(lg[i], row, f"{cfg} q{q}: the forward after the call, row {i}")
        assert int(am[i]) == ref_argmax(row)
        check_slot_rows(b, r, [pos[i]], f"{cfg} q{q}: the forward after the call")
    b.close()


# ---------------------------------------------------------------------------------------------- 2. table and form boundaries, wide and paged

def many_rows(L, img, b, n, n_early, early_at, budget):
    """n rows at depths 0 .. 8 but rows 1 and 2 at 60 and 62 with budget 10 (their runs cross the page edge at 64); the first n_early rows of the others
    stop at step early_at, and so does row 1 (its unreached second page stays held)"""
    cfg = "mini-llama"
    depths = [i % 9 for i in range(n)]; depths[1], depths[2] = 60, 62
    budgets = [budget] * n; budgets[1] = budgets[2] = 10
    rows = [Row(L, img, i) for i in range(n)]
    for i, r in enumerate(rows):
        r.prefill(b, S.prompt_tokens(cfg, depths[i], 700 + i))
    firsts = [(11 + 37 * i) % V for i in range(n)]
    outs = [r.continuation(firsts[i], budgets[i])[0] for i, r in enumerate(rows)]
    early = [1] + [i for i in range(3, n) if outs[i].index(outs[i][early_at]) == early_at][:n_early - 1]
    assert len(early) == n_early
    stops = [[outs[i][early_at]] if i in early else [] for i in range(n)]
    for i in early:
        assert outs[i].index(outs[i][early_at]) == early_at
    return rows, depths, budgets, firsts, outs, stops, early


@gpu
@pytest.mark.parametrize("n,n_early,early_at,budget", [(20, 5, 2, 6), (50, 4, 1, 5)])
@pytest.mark.parametrize("paged", [False, True])
def test_table_and_form_boundaries(L, paged, n, n_early, early_at, budget):
    """20 rows of which 5 stop at step 2: 20 -> 15 rows, the long table -> the 16-row table; 50 of which 4 stop at step 1: 50 -> 46, ring -> stream GEMMs.
    check_every 2: the look behind pass 4 (pass 2) finds them gone.  (With two passes a chunk a finished row is frozen for one pass at the most: the
    call is repeated at check_every 4, where the look behind pass 4 finds the same rows gone after two frozen passes.)"""
    img = S.build_image("mini-llama", S.Q8_0, seed=601)
    m = L.Transformer(img)
    b = L.Batch(m, 52, page_len=64, n_pages=60) if paged else L.Batch(m, 52, wide=True)
    rows, depths, budgets, firsts, outs, stops, early = many_rows(L, img, b, n, n_early, early_at, budget)
    want = expect(rows, firsts, outs, budgets, stops)
    not_vacuous(want, (2,), frozen=1)
    assert sum(1 for w in want if w[1] == STOP) == n_early and all(len(want[i][0]) == early_at + 1 for i in early)
    what = f"{'paged' if paged else 'wide'} {n} rows"
    free0 = b.pages()[2] if paged else None
    check_call(b, rows, firsts, depths, budgets, stops, want, 2, what)
    # the same call once more with four passes a chunk: the rows that STOPPED stay frozen behind their end and cross the boundary as dead rows of the table
    not_vacuous(want, (4,), frozen=2)
    if n == 50:
        assert all(rounds(len(want[i][0]), 4) - len(want[i][0]) >= 2 for i in early), "a stopped row is not frozen for two passes"
    check_call(b, rows, firsts, depths, budgets, stops, want, 4, what + ", check_every 4")
    for i, r in enumerate(rows):
        check_slot_rows(b, r, sorted({depths[i], depths[i] + len(want[i][0]) - 1}), what)
    if paged:
        # row 1 stopped at 60 + early_at + 1 <= 63: the page of [64, 70) was claimed with its budget and is still its own
        assert b.slot_pages(1) == (2, 0) and b.slot_pages(2) == (2, 0)
        free = b.pages()[2]
        assert free < free0
        b.release(1, depths[1] + len(want[1][0]))
        assert b.slot_pages(1) == (1, 0) and b.pages()[2] == free + 1
    # the state is a sequence's state
    for i, r in enumerate(rows):
        r.rewind(depths[i] + len(want[i][0]))
    pick = [0, 1, 2, 3, n - 1]
    am, lg = b.forward([rows[i].slot for i in pick], [want[i][0][-1] for i in pick], [rows[i].n for i in pick], logits=True)
    for k, i in enumerate(pick):
        assert_bit_equal(lg[k], rows[i].feed(want[i][0][-1]), f"{what}: the forward after the call, row {i}")
    b.close()


@gpu
def test_a_pool_too_small_for_the_budgets_changes_nothing(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 2, page_len=64, n_pages=3)
    rows = [Row(L, img, i) for i in range(2)]
    for i, r in enumerate(rows):
        r.prefill(b, S.prompt_tokens("mini-llama", 60, 720 + i))
    before = (b.pages(), b.slot_pages(0), b.slot_pages(1))
    assert before[0][2] == 1
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_generate: 2 pages wanted, 1 free \(the pool holds 3\)"):
        b.generate([0, 1], [5, 6], [60, 60], [10, 10])
    assert (b.pages(), b.slot_pages(0), b.slot_pages(1)) == before
    outs = [r.continuation(5 + i, 4)[0] for i, r in enumerate(rows)]
    toks, fin, stats = b.generate([0, 1], [5, 6], [60, 60], 4)
    assert [t.tolist() for t in toks] == outs and fin.tolist() == [BUDGET, BUDGET] and b.pages() == before[0]
    b.close()


# ---------------------------------------------------------------------------------------------- 3. samplers

SAMPLER_KINDS = [None, (0.0, 0.9, 11), (0.8, 1.0, 11), (1.5, 1.0, 12), (0.02, 1.0, 13), (0.8, 0.0, 12), (1.5, 0.0, 13)]


def sampled_rows(L, img, b, n):
    """n rows at small depths: SAMPLER_KINDS in turn, and every eighth row shares the sampler of the row before it"""
    rows = []
    for i in range(n):
        share = rows[-1] if i % 8 == 7 else None
        rows.append(Row(L, img, i, kind=SAMPLER_KINDS[i % 8] if share is None else None, share=share))
        rows[-1].prefill(b, S.prompt_tokens("mini-llama", [5, 0, 66, 3, 1, 9, 2, 7][i % 8], 800 + i))
    return rows


@gpu
@pytest.mark.parametrize("n", [8, 20])
def test_samplers(L, n):
    img = S.build_image("mini-llama", S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, n, wide=n > 16)
    rows = sampled_rows(L, img, b, n)
    assert rows[7].dev is rows[6].dev and sum(1 for r in rows if r.kind and r.kind[0] != 0.0) >= (6 if n == 8 else 14)
    depths = [r.n for r in rows]
    firsts = [(29 + 53 * i) % V for i in range(n)]
    budgets = [12 - i % 3 for i in range(n)]
    outs = [r.continuation(firsts[i], budgets[i])[0] for i, r in enumerate(rows)]
    # stops from each oracle's own sampled sequence: every third row at the first occurrence of its step-(2 + i % 5) token
    stops = [[outs[i][2 + i % 5]] if i % 3 == 0 else [] for i in range(n)]
    want = expect(rows, firsts, outs, budgets, stops)
    for i in range(0, n, 3):
        assert len(want[i][0]) == outs[i].index(outs[i][2 + i % 5]) + 1 and want[i][1] == STOP
    not_vacuous(want, (4,))
    for ce in (4, 1):
        check_call(b, rows, firsts, depths, budgets, stops, want, ce, f"{n} sampled rows check_every {ce}", samplers=[r.dev for r in rows])
    for i, r in enumerate(rows):
        check_slot_rows(b, r, [depths[i] + len(want[i][0]) - 1], f"{n} sampled rows")
    b.close()


# ---------------------------------------------------------------------------------------------- 4. log-probabilities

def want_logprobs(rows_seen, toks):
    x, mx, lse = log_softmax64(np.stack(rows_seen))
    return x[np.arange(len(toks)), np.asarray(toks, np.int64)] - mx - lse


@gpu
@pytest.mark.parametrize("sampled", [False, True])
def test_logprobs(L, sampled):
    """the rows of test 1 (greedy, stops and budgets) and of test 3 (samplers), two slots under masks and two under penalties"""
    img = S.build_image("mini-llama", S.Q8_0, seed=601)
    m = L.Transformer(img); n = 8 if sampled else 5
    b = L.Batch(m, n)
    b.set_history(0)
    rows = sampled_rows(L, img, b, n) if sampled else [Row(L, img, i) for i in range(n)]
    if not sampled:
        for i, r in enumerate(rows):
            r.prefill(b, S.prompt_tokens("mini-llama", DEPTHS[i], 602 + i))
    rows[1].mask, rows[2].mask = ban(V, range(100, 200)), ban(V, range(1000, 1100))
    b.set_masks([1, 2], np.stack([rows[1].mask, rows[2].mask]))
    rows[2].par, rows[3].par = params("all"), params("rep")
    b.set_penalties([2, 3], *([rows[i].par[k] for i in (2, 3)] for k in ("repetition", "presence", "frequency", "out_from")))
    depths = [r.n for r in rows]
    firsts = (FIRSTS + [9, 10, 11])[:n]
    budgets = (BUDGETS + [5, 9, 11])[:n]
    conts = [r.continuation(firsts[i], budgets[i]) for i, r in enumerate(rows)]
    outs = [c[0] for c in conts]
    stops = [[outs[i][min(len(outs[i]) - 1, 2 * i)]] if i % 2 == 0 else [] for i in range(n)]
    want = expect(rows, firsts, outs, budgets, stops)
    not_vacuous(want, (3,))
    samplers = [r.dev for r in rows] if sampled else None
    what = f"log-probabilities, {'sampled' if sampled else 'greedy'} rows"
    plain = check_call(b, rows, firsts, depths, budgets, stops, want, 3, what, samplers=samplers)
    toks, fin, lps, stats = check_call(b, rows, firsts, depths, budgets, stops, want, 3, what, samplers=samplers, logprobs=True)
    for i in range(n):
        assert toks[i].tolist() == plain[0][i].tolist()
        k = len(want[i][0])
        assert lps[i].shape == (k,) and np.all(np.isfinite(lps[i])) and np.all(lps[i] <= 0)
        assert_within_one_ulp(lps[i], want_logprobs(conts[i][1][:k], want[i][0]), f"{what}: row {i}")
    b.close()


# ---------------------------------------------------------------------------------------------- 5. slot state in the loop

@gpu
def test_slot_state_in_the_loop(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 4)
    b.set_history(0)
    prompt = S.prompt_tokens("mini-llama", 20, 603)
    free = Row(L, img, 0); free.prefill(b, prompt)
    out, _ = free.continuation(7, 8)
    stop = out[3]
    assert out.index(stop) == 3
    # a slot whose mask bans its stop token never stops
    b.fork(0, 1, 20)
    r = Row(L, img, 1, mask=ban(V, [stop]))
    for t in prompt:
        r.feed(t)
    b.set_masks([1], r.mask[None, :])
    banned, _ = r.continuation(7, 8)
    assert stop not in banned and banned[:3] == out[:3]
    toks, fin, stats = b.generate([1], [7], [20], 8, stop=[stop], check_every=3)
    assert toks[0].tolist() == banned and fin.tolist() == [BUDGET]
    # the mask cleared, from a fork of the same prefix: it stops where the oracle says
    b.clear_masks([1])
    b.fork(0, 2, 20)
    toks, fin, stats = b.generate([2], [7], [20], 8, stop=[stop], check_every=3)
    assert toks[0].tolist() == out[:4] and fin.tolist() == [STOP]
    # frequency / presence penalties with out_from at the call's start: the loop's own tokens count
    b.fork(0, 3, 20)
    p = Row(L, img, 3, par=params("freq", out_from=20))
    for t in prompt:
        p.feed(t)
    b.set_penalties([3], presence=p.par["presence"], frequency=p.par["frequency"], out_from=20)
    pen, _ = p.continuation(7, 10)
    toks, fin, stats = b.generate([3], [7], [20], 10, check_every=4)
    assert toks[0].tolist() == pen and fin.tolist() == [BUDGET]
    assert b.history(3, 10, 20).tolist() == [7] + pen[:-1]
    b.close()


# ---------------------------------------------------------------------------------------------- 6. no stops = the greedy loop

@gpu
@pytest.mark.parametrize("n", [5, 20])
def test_without_stops_it_is_the_greedy_loop(L, n):
    img = S.build_image("mini-llama", S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 2 * n, wide=True)
    depths = [(7 * i) % 70 for i in range(n)]
    for i in range(n):
        if depths[i]:
            b.prefill(i, S.prompt_tokens("mini-llama", depths[i], 900 + i), 0)
            b.fork(i, n + i, depths[i])
    firsts = [(3 + 91 * i) % V for i in range(n)]
    want = b.generate_greedy(list(range(n, 2 * n)), firsts, depths, 9)
    toks, fin, stats = b.generate(list(range(n)), firsts, depths, 9, check_every=4)
    assert np.array_equal(np.stack(toks), want) and fin.tolist() == [BUDGET] * n
    assert stats == dict(passes=12, row_passes=12 * n)
    b.close()


# ---------------------------------------------------------------------------------------------- 7. errors

@gpu
def test_errors_come_before_device_work_and_leave_everything_usable(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 3)
    r = Row(L, img, 0); r.prefill(b, S.prompt_tokens("mini-llama", 6, 604))
    good_out, _ = r.continuation(5, 3)
    T = m.args.seq_len
    lib = L.lib()

    def good(what):
        toks, fin, stats = b.generate([0], [5], [6], 3, stop=[V - 1])
        assert toks[0].tolist() == good_out and fin.tolist() == [BUDGET], what

    good("first")
    topp, other, mult = L.Sampler(V, 0.8, 0.9, 1), L.Sampler(V - 1, 0.8, 1.0, 1), L.Sampler(V, 0.8, 1.0, 1)
    name = "lmrs_batch_generate: "
    cases = [
        (dict(slots=[], tokens=[], pos=[], max_new=[]), "n = 0 is outside 1 .. 16"),
        (dict(slots=[0, 3], tokens=[1, 2], pos=[6, 0], max_new=2), "row 1: slot 3 of 3"),
        (dict(slots=[1, 1], tokens=[1, 2], pos=[0, 0], max_new=2), "slot 1 appears twice"),
        (dict(slots=[0, 1], tokens=[1, V], pos=[6, 0], max_new=2), "token 1 out of range"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, T - 3], max_new=[2, 4]), f"row 1: pos + max_new = {T + 1} exceeds seq_len = {T}"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=[2, 0]), "row 1: max_new is 0"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=2, stop=[[], list(range(17))]), "row 1: n_stop = 17 exceeds LMRS_STOP_MAX = 16"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=2, stop=[[1, V], []]), f"row 0: stop token 1 = {V} is not below vocab_size = {V}"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=2, check_every=0), "check_every is 0"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=2, samplers=[mult, topp]), "row 1: a top-p sampler"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=2, samplers=[None, other]), "row 1: the sampler was made for another vocabulary size"),
    ]
    for kw, msg in cases:
        with pytest.raises(L.LmrsError) as e:
            b.generate(**kw)
        assert str(e.value).startswith(name + msg), (msg, str(e.value))
        good(f"after {msg!r}")
    # a NULL required array, and n_stop without stop_tokens: straight at the C entry point
    u32 = lambda *v: np.array(v, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    a, out = u32(0), np.zeros(4, np.uint32)
    full = [b._h, 1, p(a), p(u32(5)), p(u32(6)), p(u32(2)), None, None, None, 1, p(out), None, p(out), p(out), None, None]
    for k in (2, 3, 4, 5, 10, 12, 13):
        args = list(full); args[k] = None
        assert lib.lmrs_batch_generate(*args) != 0 and lib.lmrs_last_error().decode().startswith(name + "NULL array"), k
        good(f"after a NULL argument {k}")
    args = list(full); args[0] = None
    assert lib.lmrs_batch_generate(*args) != 0 and lib.lmrs_last_error().decode().startswith(name + "NULL argument (the batch)")
    args = list(full); args[6] = p(u32(1))
    assert lib.lmrs_batch_generate(*args) != 0 and lib.lmrs_last_error().decode().startswith(name + "n_stop given without stop_tokens")
    good("after n_stop without stop_tokens")
    b.close()


@gpu
def test_a_vocabulary_with_an_unwritten_tail_takes_greedy_rows_only(L):
    """vocabulary 4098 (Q8_0): the classifier writes 4096 of the 4098 logits - sampled rows and log-probabilities are refused, greedy rows run"""
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-v4098", vocab_size=4098)
    img = S.build_image(cfg, S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 2)
    orc = O.Oracle(img)
    msg = r"^lmrs_batch_generate: the classifier leaves the last vocab_size % 4 logits unwritten"
    with pytest.raises(L.LmrsError, match=msg):
        b.generate([0], [5], [0], 3, samplers=[L.Sampler(4098, 0.8, 1.0, 1)])
    with pytest.raises(L.LmrsError, match=msg):
        b.generate([0], [5], [0], 3, logprobs=True)
    toks, fin, stats = b.generate([0], [5], [0], 3, samplers=[L.Sampler(4098, 0.0, 1.0, 1)])
    want, t = [], 5
    for j in range(3):
        t = ref_argmax(orc.forward(t, j)); want.append(t)
    assert toks[0].tolist() == want
    b.close()
