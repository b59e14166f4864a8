"""Token automata on batch slots (include/lmrs_hip.h): a slot's mask follows the token it chose, inside lmrs_batch_generate / _generate_topp and in every
per-call pass.  The reference is one CPU oracle PER SEQUENCE (test_batch_generate.Row) whose mask is set from the automaton's current state before each
feed (test_batch_mask.masked); the loop's control is the rule written out below.  Tokens, codes and states by value, logits and K/V rows bit for bit,
log-probabilities within one f32 ulp of a float64 log-softmax of the masked row."""
import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, assert_within_one_ulp, ref_argmax
from penalty_rules import params
from test_batch import check_slot_rows, snapshot
from test_batch_generate import BEHIND, BUDGET, DEPTHS, FIRSTS, STOP, V, Row, check_call, five_rows, rounds, want_logprobs
from test_batch_mask import masked
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
FINAL = 3
DEAD = 0xFFFFFFFF


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def random_automaton(L, r, final=None, vocab=V):
    """the issue's recipe: class_of uniform in 5 classes, 7 states, every next entry dead with probability 0.5, one entry per state kept live"""
    rng = np.random.default_rng(900 + r)
    class_of = rng.integers(0, 5, vocab).astype(np.uint16)
    nxt = rng.integers(0, 7, (7, 5)).astype(np.uint32)
    dead = rng.random((7, 5)) < 0.5
    dead[np.arange(7), rng.integers(0, 5, 7)] = False
    nxt[dead] = DEAD
    return L.TokenAutomaton(class_of, nxt, final)


def constrained(row, ta, q0, t0, steps):
    """`steps` free-running steps of the sequence under the automaton's masks -> (tokens, the rows they were chosen from, states): the j-th row is masked under
    states[j], token j moves to states[j + 1].  It ends early in a state that allows nothing.  The final flags play no part: they end rows, they mask nothing"""
    out, rows, states, t = [], [], [q0], t0
    for _ in range(steps):
        row.mask = ta.allowed(states[-1])
        if not row.mask.any():
            break
        rows.append(row.feed(t))
        t = row.choose(rows[-1])
        out.append(t)
        nx = int(ta.next[states[-1], ta.class_of[t]])
        assert nx != DEAD, "the oracle chose a token its mask had cleared"
        states.append(nx)
    row.mask = None
    return out, rows, states


def rule(out, states, final, budget, stop):
    """the contract's endings over a constrained continuation: STOP, then FINAL, then BUDGET"""
    for j, o in enumerate(out):
        if o in stop:
            return out[:j + 1], STOP
        if final[states[j + 1]]:
            return out[:j + 1], FINAL
        if j + 1 == budget:
            return out[:j + 1], BUDGET
    raise AssertionError("the continuation is shorter than the budget")


def attach_and_call(b, rows, tas, hs, q0, firsts, pos, budgets, stops, want, ce, what, **kw):
    """every slot back in its start state, the call judged by test_batch_generate.check_call, then every slot's state against the host walk"""
    b.attach([r.slot for r in rows], hs, q0)
    got = check_call(b, rows, firsts, pos, budgets, stops, want, ce, what, **kw)
    for i, r in enumerate(rows):
        q, k, ok = tas[i].walk(q0[i], want[i][0])
        assert ok and k == len(want[i][0])
        st = b.automaton_state(r.slot)
        assert st is not None and st[0] == q and st[1] == int(tas[i].allowed(q).sum()) and st[2] == bool(tas[i].final[q]), f"{what}: row {i}: state {st} vs the walk's {q}"
    return got


# ---------------------------------------------------------------------------------------------- 1. the mask builder alone

def builder_case(L, rng, vocab, n_classes, n_states):
    class_of = rng.integers(0, n_classes, vocab).astype(np.uint16)
    nxt = rng.integers(0, n_states, (n_states, n_classes)).astype(np.uint32)
    nxt[rng.random((n_states, n_classes)) < 0.5] = DEAD
    one = None
    if n_states >= 3:
        nxt[0, :] = 0                                                           # a state with everything live
        if n_classes >= 2:                                                      # a state with everything dead but one token: token `one` alone in class 1
            one = int(rng.integers(0, vocab))
            class_of[class_of == 1] = 0
            class_of[one] = 1
            nxt[1, :] = DEAD
            nxt[1, 1] = 2
    return L.TokenAutomaton(class_of, nxt), one


@gpu
@pytest.mark.parametrize("vocab", [2052, 4096, 33])
def test_the_mask_builder_against_numpy(L, vocab):
    """vocabulary 2052: a last word of 4 bits; 33: a last word of one"""
    rng = np.random.default_rng(vocab)
    for n_classes in (1, 2, 300, 65536):
        for n_states in (1, 3, 70):
            ta, one = builder_case(L, rng, vocab, n_classes, n_states)
            got = L.automaton_masks(ta)
            want = np.stack([ta.allowed(q) for q in range(n_states)])
            what = f"vocab {vocab}, {n_classes} classes, {n_states} states"
            assert got.shape == (n_states, (vocab + 31) // 32) and got.dtype == np.uint32
            assert np.array_equal(got, L.pack_mask(want)), what                  # (bit for bit: the bits at and above vocab are clear in pack_mask's words)
            if n_states >= 3:
                assert want[0].all(), what
                if one is not None:
                    assert want[1].nonzero()[0].tolist() == [one], what


# ---------------------------------------------------------------------------------------------- 2. the loop, short table

def five_constrained(L, cfg, q):
    m, b, rows, others, snaps, conts, _ = five_rows(L, cfg, q)
    tas = [random_automaton(L, r) for r in range(5)]
    q0 = [r % 7 for r in range(5)]
    cons = []
    for i, r in enumerate(rows):
        r.rewind(DEPTHS[i])
        cons.append(constrained(r, tas[i], q0[i], FIRSTS[i], 12))
        assert len(cons[i][0]) == 12
    # not vacuous: at least three of the five rows visit three states or more and leave their unconstrained continuation
    moved = [i for i in range(5) if len(set(cons[i][2])) >= 3 and cons[i][0] != conts[i][0]]
    assert len(moved) >= 3, f"{cfg}: rows {moved} only visit three states and differ from the free continuation"
    return m, b, rows, others, snaps, tas, q0, cons


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_the_loop_on_the_short_table(L, cfg, q):
    m, b, rows, others, snaps, tas, q0, cons = five_constrained(L, cfg, q)
    nl = m.args.n_layers
    hs = [b.automaton(ta) for ta in tas]
    # (a) the recipe as it stands: no state is final, every row runs to its budget of 12 under a mask that changes with every token
    want = [(c[0], BUDGET) for c in cons]
    for ce in (1, 3, 64):
        attach_and_call(b, rows, tas, hs, q0, FIRSTS, DEPTHS, [12] * 5, None, want, ce, f"{cfg} q{q} no finals, check_every {ce}")
    # (b) final states and stop sets, so that STOP, FINAL and BUDGET all occur; row 1's stop token is the one that enters its final state: STOP wins
    enter = lambda i, state: cons[i][2][1:].index(state)                        # the step whose token first enters `state`
    fstate = {0: cons[0][2][3], 1: cons[1][2][3], 4: cons[4][2][6]}
    finals = [np.zeros(7, bool) for _ in range(5)]
    for i, s in fstate.items():
        finals[i][s] = True
    j1 = enter(1, fstate[1])
    assert cons[1][0].index(cons[1][0][j1]) == j1, "row 1's stop token occurs before it enters the final state"
    stops = [[], [cons[1][0][j1]], [cons[2][0][4]], [], []]
    budgets = [12, 12, 12, 7, 12]
    tfs = [random_automaton(L, r, finals[r]) for r in range(5)]
    hf = [b.automaton(ta) for ta in tfs]
    want = [rule(cons[i][0], cons[i][2], finals[i], budgets[i], set(stops[i])) for i in range(5)]
    assert {w[1] for w in want} == {BUDGET, STOP, FINAL}, [(len(w[0]), w[1]) for w in want]
    assert want[1] == (cons[1][0][:j1 + 1], STOP) and finals[1][cons[1][2][j1 + 1]], "STOP over FINAL is not pinned"
    assert want[0][1] == FINAL and want[3] == (cons[3][0][:7], BUDGET)
    ces = (1, 3, 64)
    assert any(rounds(len(w[0]), ce) - len(w[0]) >= 2 for w in want for ce in ces), "no row is frozen for two passes inside a chunk"
    for ce in ces:
        what = f"{cfg} q{q} finals and stops, check_every {ce}"
        attach_and_call(b, rows, tfs, hf, q0, FIRSTS, DEPTHS, budgets, stops, want, ce, what)
        for i, r in enumerate(rows):
            k = len(want[i][0])
            check_slot_rows(b, r, sorted({DEPTHS[i], DEPTHS[i] + k - 1}), what)
            assert b.history(r.slot, k, DEPTHS[i]).tolist() == [FIRSTS[i]] + want[i][0][:-1], f"{what}: the record of row {i}'s own positions"
            if k < BEHIND:                                                      # (part (a) wrote 12 of the 14 positions behind the depth: the last two still show)
                now = snapshot(b, r.slot, range(DEPTHS[i] + 12, DEPTHS[i] + BEHIND), nl)
                was = snapshot_part(snaps[i], nl, 12)
                for x, y in zip(was, now):
                    assert_bit_equal(y, x, f"{what}: row {i}: a K/V row beyond pos + n_out changed")
                assert b.history(r.slot, BEHIND - 12, DEPTHS[i] + 12).tolist() == others[i][12:].tolist(), f"{what}: row {i}: the record beyond pos + n_out changed"
    b.close()


def snapshot_part(snap, n_layers, first):
    """test_batch.snapshot's list over range(depth, depth + BEHIND), cut to the positions from depth + first on"""
    return [snap[(l * BEHIND + p) * 2 + w] for l in range(n_layers) for p in range(first, BEHIND) for w in (0, 1)]


@gpu
def test_no_row_beyond_the_end_changes(L):
    """one call on untouched slots: K/V rows and record entries at and beyond pos + n_out are as the prefill left them (rows that end after 1, 3 and 7 tokens)"""
    m, b, rows, others, snaps, tas, q0, cons = five_constrained(L, "mini-llama", S.Q8_0)
    nl = m.args.n_layers
    finals = [np.zeros(7, bool) for _ in range(5)]
    finals[0][cons[0][2][1]] = True                                             # row 0 ends with its first token
    finals[2][cons[2][2][3]] = True
    budgets = [12, 7, 12, 12, 3]
    tfs = [random_automaton(L, r, finals[r]) for r in range(5)]
    hf = [b.automaton(ta) for ta in tfs]
    want = [rule(cons[i][0], cons[i][2], finals[i], budgets[i], set()) for i in range(5)]
    assert want[0] == (cons[0][0][:1], FINAL) and want[2][1] == FINAL and want[4] == (cons[4][0][:3], BUDGET)
    attach_and_call(b, rows, tfs, hf, q0, FIRSTS, DEPTHS, budgets, None, want, 4, "beyond the end")
    for i, r in enumerate(rows):
        k = len(want[i][0])
        now = snapshot(b, r.slot, range(DEPTHS[i], DEPTHS[i] + BEHIND), nl)
        for j, (x, y) in enumerate(zip(snaps[i], now)):
            if (j // 2) % BEHIND >= k:
                assert_bit_equal(y, x, f"row {i}: a K/V row at or beyond pos + n_out changed")
        assert b.history(r.slot, BEHIND - k, DEPTHS[i] + k).tolist() == others[i][k:].tolist(), f"row {i}: the record beyond pos + n_out changed"
    b.close()


# ---------------------------------------------------------------------------------------------- 3. long table and paged

@gpu
@pytest.mark.parametrize("paged", [False, True])
def test_the_long_table_and_a_paged_batch(L, paged):
    """20 rows, two automata shared by ten slots each in different states; the rows that end early take the call from the long table to the 16-row table"""
    cfg, n, budget = "mini-llama", 20, 6
    img = S.build_image(cfg, S.Q8_0, seed=601)
    m = L.Transformer(img)
    b = L.Batch(m, 22, page_len=64, n_pages=40) if paged else L.Batch(m, 22, wide=True)
    depths = [i % 9 for i in range(n)]; depths[1], depths[2] = 60, 62           # (their runs cross the page edge at 64)
    rows = [Row(L, img, i) for i in range(n)]
    for i, r in enumerate(rows):
        r.prefill(b, S.prompt_tokens(cfg, depths[i], 700 + i))
    firsts = [(11 + 37 * i) % V for i in range(n)]
    final = [np.zeros(7, bool), np.zeros(7, bool)]
    final[1][[2, 5]] = True
    two = [random_automaton(L, 0, final[0]), random_automaton(L, 1, final[1])]
    handles = [b.automaton(ta) for ta in two]
    tas, hs, q0 = [two[i % 2] for i in range(n)], [handles[i % 2] for i in range(n)], [(i // 2) % 7 for i in range(n)]
    cons = [constrained(r, tas[i], q0[i], firsts[i], budget) for i, r in enumerate(rows)]
    stops = [[cons[i][0][2]] if i % 6 == 0 else [] for i in range(n)]
    want = [rule(cons[i][0], cons[i][2], final[i % 2], budget, set(stops[i])) for i in range(n)]
    early = [i for i in range(n) if len(want[i][0]) <= 3]
    assert 4 <= len(early) <= 16 and {w[1] for w in want} == {BUDGET, STOP, FINAL}, [(len(w[0]), w[1]) for w in want]
    assert len({(i % 2, q0[i]) for i in range(n)}) >= 12
    what = f"{'paged' if paged else 'wide'} 20 rows"
    for ce in (2, 4):
        attach_and_call(b, rows, tas, hs, q0, firsts, depths, [budget] * n, stops, want, ce, f"{what}, check_every {ce}")
    for i, r in enumerate(rows):
        check_slot_rows(b, r, sorted({depths[i], depths[i] + len(want[i][0]) - 1}), what)
    # an automaton in use is not destroyed; detached from every slot it is
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_automaton_destroy: 10 slots are attached"):
        b.drop_automaton(handles[0])
    b.attach(list(range(0, n, 2)), None)
    b.drop_automaton(handles[0])
    assert b.automaton_state(0) is None and b.automaton_state(1) is not None
    b.close()


# ---------------------------------------------------------------------------------------------- 4. labels

@gpu
def test_labels_end_final_and_the_leaf_refuses_a_pass(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 4)
    labels = [[50], [60, 61], [60, 62, 63]]
    ta = L.TokenAutomaton.from_sequences(V, labels)
    h = b.automaton(ta)
    depths = [5, 0, 33, 9]
    rows = [Row(L, img, i) for i in range(4)]
    for i, r in enumerate(rows):
        r.prefill(b, S.prompt_tokens(cfg, depths[i], 930 + i))
    firsts = [3, 400, 77, 1000]
    cons = [constrained(r, ta, 0, firsts[i], 5) for i, r in enumerate(rows)]
    want = [rule(c[0], c[2], ta.final.astype(bool), 5, set()) for c in cons]
    assert all(w[1] == FINAL and w[0] in labels for w in want), want
    for ce in (1, 4):
        attach_and_call(b, rows, [ta] * 4, [h] * 4, [0] * 4, firsts, depths, [5] * 4, None, want, ce, f"labels, check_every {ce}")
    # the leaf allows nothing: no pass may ask for a row of that slot; the other slots are not in the way
    st = b.automaton_state(0)
    assert st[1] == 0 and st[2] and b.mask_info(0) is None
    pos0 = depths[0] + len(want[0][0])
    with pytest.raises(L.LmrsError, match=rf"^lmrs_batch_forward: row 0: slot 0 stands in final state {st[0]} of its automaton, which allows no token"):
        b.forward([0], [want[0][0][-1]], [pos0])
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_forward_runs: run 0: slot 0 stands in final state"):
        b.forward_runs([(0, pos0, [want[0][0][-1]], 1)])
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_generate: row 0: slot 0 stands in final state"):
        b.generate([0], [want[0][0][-1]], [pos0], 2)
    assert b.automaton_state(0) == st
    b.forward_runs([(0, pos0, [want[0][0][-1]], 0)])                            # (K/V rows only: no output row, nothing to mask)
    # back at the root it works
    b.attach([0], h, 0)
    am, lg = b.forward([0], [want[0][0][-1]], [pos0], logits=True)
    rows[0].rewind(pos0)
    rows[0].mask = ta.allowed(0)
    row = rows[0].feed(want[0][0][-1])
    assert_bit_equal(lg[0], row, "the forward after the re-attach")
    assert int(am[0]) == ref_argmax(row) and int(am[0]) in (50, 60)
    assert b.automaton_state(0)[0] == 0, "a forward moves no state"
    b.close()


# ---------------------------------------------------------------------------------------------- 5. samplers

@gpu
def test_sample_mult_rows_in_the_loop(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 5)
    kinds = [(0.8, 1.0, 11), (1.5, 1.0, 12), None, (0.8, 0.0, 12), (1.5, 0.0, 13)]
    rows = [Row(L, img, i, kind=k) for i, k in enumerate(kinds)]
    for i, r in enumerate(rows):
        r.prefill(b, S.prompt_tokens(cfg, [5, 0, 66, 3, 1][i], 800 + i))
    depths = [r.n for r in rows]
    final = np.zeros(7, bool); final[4] = True
    tas = [random_automaton(L, r, final if r == 1 else None) for r in range(5)]
    hs = [b.automaton(ta) for ta in tas]
    q0 = [3, 1, 0, 6, 2]
    firsts = [29, 82, 135, 188, 241]
    cons = [constrained(r, tas[i], q0[i], firsts[i], 10) for i, r in enumerate(rows)]
    want = [rule(c[0], c[2], tas[i].final.astype(bool), 10, set()) for i, c in enumerate(cons)]
    assert sum(len(set(c[2])) >= 3 for c in cons) >= 3
    for ce in (4, 1):
        attach_and_call(b, rows, tas, hs, q0, firsts, depths, [10] * 5, None, want, ce, f"sample_mult rows, check_every {ce}", samplers=[r.dev for r in rows])
    b.close()


@gpu
def test_a_topp_row_and_an_argmax_row_with_logprobs(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 2)
    kinds = [(1.0, 0.9, 21), None]
    rows = [Row(L, img, i) for i in range(2)]
    rows[0].ref = O.Sampler(V, *kinds[0])
    for i, r in enumerate(rows):
        r.prefill(b, S.prompt_tokens(cfg, [6, 30][i], 850 + i))
    depths = [r.n for r in rows]
    tas = [random_automaton(L, 2), random_automaton(L, 3)]
    hs = [b.automaton(ta) for ta in tas]
    q0, firsts, budgets = [1, 4], [3, 400], [9, 12]
    cons = [constrained(r, tas[i], q0[i], firsts[i], budgets[i]) for i, r in enumerate(rows)]
    stops = [[cons[0][0][5]], []]
    want = [rule(cons[i][0], cons[i][2], np.zeros(7, bool), budgets[i], set(stops[i])) for i in range(2)]
    # the vector the top-p sampler must hold afterwards: a host sampler fed the masked rows the oracle chose from
    host = L.Sampler(V, *kinds[0])
    for row in cons[0][1][:len(want[0][0])]:
        host.sample(row.copy())
    for ce in (3, 1):
        dev = L.Sampler(V, *kinds[0])
        b.attach([0, 1], hs, q0)
        toks, fin, lps, stats = b.generate_topp([0, 1], firsts, depths, budgets, stop=stops, samplers=[dev, None], check_every=ce, logprobs=True)
        for i, (w, f) in enumerate(want):
            assert toks[i].tolist() == w and int(fin[i]) == f, f"check_every {ce}: row {i}: {toks[i].tolist()} vs {w}"
            assert_within_one_ulp(lps[i], want_logprobs(cons[i][1][:len(w)], w), f"check_every {ce}: log-probabilities, row {i}")
            assert b.automaton_state(i)[0] == tas[i].walk(q0[i], w)[0]
        vec, ordered = dev.candidates()
        assert ordered and vec.tobytes() == host.candidates()[0].tobytes(), f"check_every {ce}: the top-p sampler's vector after the call"
    b.close()


# ---------------------------------------------------------------------------------------------- 6. the per-call passes

@gpu
def test_per_call_passes_equal_the_same_call_under_the_states_mask(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=601)
    m = L.Transformer(img)
    a, s = L.Batch(m, 2), L.Batch(m, 2)                                         # a: slot 0 under an automaton; s: slot 0 under set_masks of the same state
    prompt = S.prompt_tokens(cfg, 20, 940)
    for b in (a, s):
        b.prefill(0, prompt, 0)
        b.prefill(1, prompt[:7], 0)
    ta = random_automaton(L, 4)
    h = a.automaton(ta)
    a.attach([0], h, 5)
    q = 5
    for step, toks in enumerate([[7], [9, 300]]):
        s.set_masks([0], ta.allowed(q)[None, :])
        assert a.mask_info(0) == s.mask_info(0) == int(ta.allowed(q).sum())
        x, y = (b.forward([0, 1], [5, 6], [20, 7], logits=True) for b in (a, s))
        assert np.array_equal(x[0], y[0])
        assert_bit_equal(x[1], y[1], f"forward in state {q}")
        assert np.isneginf(x[1][0]).sum() == V - int(ta.allowed(q).sum()) and not np.isneginf(x[1][1]).any()
        x, y = (b.forward_runs([(0, 20, [5, 8, 11], 2), (1, 7, [6], 1)], k=5, logits=True) for b in (a, s))
        for u, v in zip(x, y):
            assert_bit_equal(u, v, f"forward_runs with two outputs and top-5 in state {q}")
        assert ta.allowed(q)[x[2][:2]].all(), "a top-k candidate of the automaton's rows is not allowed"
        for kind in [(0.0, 1.0, 1), (0.8, 1.0, 11), (1.0, 0.9, 21)]:
            x, y = (b.forward_sample([0, 1], [5, 6], [20, 7], [L.Sampler(V, *kind), L.Sampler(V, *kind)]) for b in (a, s))
            assert x.tolist() == y.tolist() and ta.allowed(q)[x[0]], f"forward_sample {kind} in state {q}"
        assert a.automaton_state(0)[0] == q, "a per-call pass moved the state"
        # advance moves it; a token the state does not allow fails the call and changes nothing
        ok = [int(t) for t in ta.allowed(q).nonzero()[0][:1]]
        q2 = ta.walk(q, ok)[0]
        bad = int((~ta.allowed(q2)).nonzero()[0][0])
        with pytest.raises(L.LmrsError, match=rf"^lmrs_batch_automaton_advance: token 1 = {bad} is not allowed in state {q2} "):
            a.advance(0, ok + [bad])
        assert a.automaton_state(0)[0] == q
        a.advance(0, ok)
        assert a.automaton_state(0)[0] == q2
        q = q2
    # k above the state's count is refused, as under a mask
    one = L.TokenAutomaton.from_sequences(V, [[5, 6], [5, 7, 8]])
    h1 = a.automaton(one)
    a.attach([0], h1, 0)
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_forward_runs: run 0: slot 0: k = 2 exceeds the 1 tokens its automaton's state allows"):
        a.forward_runs([(0, 20, [5], 1)], k=2)
    assert a.forward_runs([(0, 20, [5], 1)], k=1)[0].tolist() == [5]
    a.close(); s.close()


# ---------------------------------------------------------------------------------------------- 7. penalties in front of the automaton

@gpu
def test_penalties_are_applied_in_front_of_the_automaton(L):
    cfg = "mini-gemma"
    img = S.build_image(cfg, S.Q4_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 1)
    b.set_history(0)
    r = Row(L, img, 0, par=params("sink"))                                      # (the kinds with milder parameters leave this row's tokens as they are)
    b.set_penalties([0], *([r.par[k]] for k in ("repetition", "presence", "frequency", "out_from")))
    r.prefill(b, S.prompt_tokens(cfg, 40, 950))
    ta = random_automaton(L, 5)
    h = b.automaton(ta)
    out, seen, states = constrained(r, ta, 2, 77, 10)
    r.rewind(40)
    r.par = None
    plain = constrained(r, ta, 2, 77, 10)[0]
    assert plain != out, "the penalties change nothing on this row"
    b.attach([0], h, 2)
    toks, fin, lps, stats = b.generate([0], [77], [40], 10, check_every=3, logprobs=True)
    assert toks[0].tolist() == out and fin.tolist() == [BUDGET]
    assert_within_one_ulp(lps[0], want_logprobs(seen, out), "log-probabilities of the penalised, masked rows")
    b.close()


# ---------------------------------------------------------------------------------------------- 8. refusals

@gpu
def test_refusals_come_before_device_work_and_leave_everything_usable(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 3)
    r = Row(L, img, 0); r.prefill(b, S.prompt_tokens(cfg, 6, 604))
    ta = random_automaton(L, 6)
    trie = L.TokenAutomaton.from_sequences(V, [[9]])
    h, ht = b.automaton(ta), b.automaton(trie)
    b.attach([0], h, 2)
    good_out = constrained(r, ta, 2, 5, 3)[0]

    def good(what):
        b.attach([0], h, 2)
        toks, fin, stats = b.generate([0], [5], [6], 3)
        assert toks[0].tolist() == good_out and fin.tolist() == [BUDGET], what
        b.attach([0], h, 2)

    good("first")
    b.set_masks([1], np.ones((1, V), bool))
    other = L.Batch(m, 1)
    ho = other.automaton(ta)
    cases = [
        (lambda: b.attach([1], h, 0), "lmrs_batch_attach_automaton: row 0: slot 1: the slot has a mask"),
        (lambda: b.set_masks([2, 0], np.ones((2, V), bool)), "lmrs_batch_set_masks: mask 1: slot 0 has an automaton"),
        (lambda: b.attach([2], h, 7), "lmrs_batch_attach_automaton: row 0: slot 2: start state 7 of 7"),
        (lambda: b.attach([2], ht, 1), "lmrs_batch_attach_automaton: row 0: slot 2: start state 1 is final and allows no token"),
        (lambda: b.attach([2], ho, 0), "lmrs_batch_attach_automaton: row 0: slot 2: not an automaton of this batch"),
        (lambda: b.attach([2, 2], h, 0), "lmrs_batch_attach_automaton: slot 2 appears twice"),
        (lambda: b.attach([3], h, 0), "lmrs_batch_attach_automaton: row 0: slot 3 of 3"),
        (lambda: b.generate_greedy([0], [5], [6], 3), "lmrs_batch_generate_greedy: row 0: slot 0 has an automaton"),
        (lambda: b.drop_automaton(h), "lmrs_batch_automaton_destroy: 1 slots are attached"),
        (lambda: b.drop_automaton(ho), "lmrs_batch_automaton_destroy: not an automaton of this batch"),
        (lambda: b.advance(2, [1]), "lmrs_batch_automaton_advance: slot 2 has no automaton"),
        (lambda: b.automaton(L.TokenAutomaton(ta.class_of, np.full((7, 5), DEAD, np.uint32))), "lmrs_batch_automaton_create: state 0 is not final and every class of it is dead"),
    ]
    for call, msg in cases:
        with pytest.raises(L.LmrsError) as e:
            call()
        assert str(e.value).startswith(msg), (msg, str(e.value))
        assert b.automaton_state(0)[0] == 2 and b.automaton_state(2) is None and b.mask_info(1) == V, f"after {msg!r}"
        good(f"after {msg!r}")
    # fork and release neither copy nor clear the attachment
    b.clear_masks([1])
    b.fork(0, 1, 6)
    assert b.automaton_state(1) is None and b.automaton_state(0)[0] == 2
    # a seventeenth automaton
    more = [b.automaton(trie) for _ in range(L.AUTOMATA_MAX - 2)]
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_automaton_create: the batch holds LMRS_AUTOMATA_MAX = 16 automata already"):
        b.automaton(trie)
    b.drop_automaton(more[0])
    b.automaton(trie)
    good("after the seventeenth automaton")
    other.close(); b.close()


@gpu
def test_a_vocabulary_with_an_unwritten_tail_has_no_automata(L):
    import dataclasses
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-v4098", vocab_size=4098)
    m = L.Transformer(S.build_image(cfg, S.Q8_0, seed=601)); b = L.Batch(m, 1)
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_automaton_create: the classifier leaves the last vocab_size % 4 logits unwritten"):
        b.automaton(random_automaton(L, 0, vocab=4098))
    b.close()


# ---------------------------------------------------------------------------------------------- 9. a batch without automata

@gpu
def test_a_batch_without_automata_runs_the_loop_it_ran(L):
    """no slot attached - with and without an automaton created on the batch - the loop gives generate_greedy's tokens and the same statistics"""
    cfg, n = "mini-llama", 5
    img = S.build_image(cfg, S.Q8_0, seed=601)
    m = L.Transformer(img); b = L.Batch(m, 2 * n, wide=True)
    depths = [(7 * i) % 70 for i in range(n)]
    for i in range(n):
        if depths[i]:
            b.prefill(i, S.prompt_tokens(cfg, depths[i], 900 + i), 0)
    firsts = [(3 + 91 * i) % V for i in range(n)]

    def run():
        for i in range(n):
            b.fork(i, n + i, depths[i]) if depths[i] else None
        want = b.generate_greedy(list(range(n, 2 * n)), firsts, depths, 9)
        toks, fin, stats = b.generate(list(range(n)), firsts, depths, 9, check_every=4)
        assert np.array_equal(np.stack(toks), want) and fin.tolist() == [BUDGET] * n
        assert stats == dict(passes=12, row_passes=12 * n)
        return want

    first = run()
    h = b.automaton(random_automaton(L, 0))
    b.attach([n], h, 0)
    b.attach([n], None)
    assert np.array_equal(run(), first) and all(b.automaton_state(i) is None for i in range(2 * n))
    b.close()
