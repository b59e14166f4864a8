"""lmrs_batch_generate_topp (include/lmrs_hip.h): the batch's device loop with top-p rows, their candidate vectors resident on the device for the length
of the call.  The launches alone (lmrs_op_topp_rows) are compared with the rule written out in tests/topp_rules.py and with lmrs_sampler_topp_pairs, tokens
and whole vectors bit for bit; the loop with one CPU oracle and one O.Sampler PER SEQUENCE, as tests/test_batch_generate.py does for the other samplers -
and afterwards every top-p sampler's vector with the one a host sampler holds after the same rows.

The synthetic models' rows are so alike from step to step that a sampler's stale entries hardly ever reach the part of the vector the draw looks at.  The
peaked samplers here have therefore been USED before the call, once, on a row of 400 equally likely tokens (WARM): entries [n0, 400) of that call are the
stale state the first steps merge with, and the seeds are chosen (on the CPU, asserted below) so that tokens differ from what a fresh sampler gives."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as O
import topp_rules as TR
from parity_rules import assert_within_one_ulp
from penalty_rules import params
from test_batch import check_slot_rows
from test_batch_generate import BUDGET, STOP, V, Row, expect, not_vacuous, rounds, want_logprobs
from test_batch_generate_topp_host import hand_cases
from test_batch_mask import ban
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
NO_CANDIDATE = 2
CFG = "mini-llama"
WARM = 400
# row i of the loop tests takes KINDS[i % 8]: "peak" = (0.15, 0.99, PEAK_SEED[i]), warmed; the flat sampler's n0 exceeds half the vocabulary
KINDS = [None, (0.8, 1.0, 11), "peak", (1.0, 0.9, 21), (1.0, 0.05, 22), "peak", (0.0, 0.9, 5), (1.5, 0.0, 13)]
PEAK_SEED = {2: 35, 5: 35, 10: 187, 13: 38, 18: 39}
DEPTH = [5, 0, 66, 3, 1, 9, 2, 7]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


@functools.lru_cache(maxsize=None)
def image():
    return S.build_image(CFG, S.Q8_0, seed=601)


def is_topp(kind):
    return kind is not None and kind[0] != 0.0 and 0.0 < kind[1] < 1.0


def warm_row(seed):
    row = np.full(V, -30.0, np.float32)
    row[np.random.default_rng(seed).choice(V, WARM, replace=False)] = 0.0
    return row


def kind_of(i):
    k = KINDS[i % 8]
    return (0.15, 0.99, PEAK_SEED[i]) if k == "peak" else k


def warmed(i):
    return KINDS[i % 8] == "peak"


def arm(make, kind, warm):
    """a new sampler of `kind` (make: L.Sampler or O.Sampler), used once before if warm"""
    s = make(V, *kind)
    if warm:
        s.sample(warm_row(kind[2]))
    return s


def n0_of(row, kind):
    x = row / np.float32(kind[0])
    e = np.exp(x - x.max(), dtype=np.float32)
    return int(np.count_nonzero(e / e.sum(dtype=np.float32) >= np.float32((1.0 - kind[1]) / (V - 1))))


class Scene:
    pass


@functools.lru_cache(maxsize=None)
def scene(n):
    """everything the loop tests need that the CPU can say, once per row count: the rows' oracles after their continuations, what the call must return,
    the vectors the top-p samplers must hold afterwards - and the two witnesses that the case is not vacuous"""
    import lmrs_amd as L
    sc = Scene()
    sc.rows = [Row(L, image(), i) for i in range(n)]
    sc.kinds = [kind_of(i) for i in range(n)]
    sc.prompts = [S.prompt_tokens(CFG, DEPTH[i % 8], 800 + i) for i in range(n)]
    sc.firsts = [(29 + 53 * i) % V for i in range(n)]
    sc.budgets = [12 - i % 3 for i in range(n)]
    sc.depths = [len(p) for p in sc.prompts]
    conts = []
    for i, r in enumerate(sc.rows):
        for t in sc.prompts[i]:
            r.feed(t)
        r.ref = arm(O.Sampler, sc.kinds[i], warmed(i)) if sc.kinds[i] else None
        conts.append(r.continuation(sc.firsts[i], sc.budgets[i]))
    outs = [c[0] for c in conts]
    # stops from each oracle's own sequence: a flat top-p row at its fifth token, every third of the others as test_samplers
    at = lambda i: 4 if i % 8 == 3 else 2 + i % 5 if i % 3 == 0 else None
    sc.stops = [[outs[i][at(i)]] if at(i) is not None else [] for i in range(n)]
    sc.want = expect(sc.rows, sc.firsts, outs, sc.budgets, sc.stops)
    sc.topp = [i for i in range(n) if is_topp(sc.kinds[i])]
    # the vector every top-p sampler must hold afterwards: a host sampler fed the rows the oracle chose from
    sc.vec = {}
    for i in sc.topp:
        host = arm(L.Sampler, sc.kinds[i], warmed(i))
        for row in conts[i][1][:len(sc.want[i][0])]:
            host.sample(row.copy())
        sc.vec[i] = host.candidates()[0]
    # not vacuous (1): the stale state matters - tokens of at least two rows differ from what a fresh sampler gives on the same row
    sc.stale = [i for i in sc.topp if any(O.Sampler(V, *sc.kinds[i]).sample(conts[i][1][j].copy()) != sc.want[i][0][j] for j in range(len(sc.want[i][0])))]
    # (2): a top-p row that stops at least two passes before its chunk of four ends - frozen in the table with its vector on the device
    sc.frozen = [i for i in sc.topp if sc.want[i][1] == STOP and rounds(len(sc.want[i][0]), 4) - len(sc.want[i][0]) >= 2]
    sc.flat_n0 = [n0_of(conts[i][1][0], sc.kinds[i]) for i in range(n) if i % 8 == 3]
    return sc


def test_the_loop_cases_are_not_vacuous():
    """on the CPU, before any device runs: the seeds and temperatures were searched with the oracle until both witnesses hold"""
    for n in (8, 20):
        sc = scene(n)
        assert len(sc.stale) >= 2, f"{n} rows: the stale state changes tokens of rows {sc.stale} only"
        assert sc.frozen, f"{n} rows: no top-p row stops two passes before its chunk ends: {[(len(w[0]), w[1]) for w in sc.want]}"
        assert all(k > V // 2 for k in sc.flat_n0), sc.flat_n0
        not_vacuous(sc.want, (4,))
        assert {"peak"} < {KINDS[i % 8] for i in sc.topp} and len(sc.topp) >= (4 if n == 8 else 10)


def dev_samplers(L, sc):
    return [arm(L.Sampler, k, warmed(i)) if k else None for i, k in enumerate(sc.kinds)]


def check_topp_call(L, b, sc, ce, what, idx=None, logprobs=False):
    idx = list(range(len(sc.rows))) if idx is None else idx
    devs = dev_samplers(L, sc)
    got = b.generate_topp([sc.rows[i].slot for i in idx], [sc.firsts[i] for i in idx], [sc.depths[i] for i in idx], [sc.budgets[i] for i in idx],
                          stop=[sc.stops[i] for i in idx], samplers=[devs[i] for i in idx], check_every=ce, logprobs=logprobs)
    toks, fin, stats = got[0], got[1], got[-1]
    for k, i in enumerate(idx):
        w, f = sc.want[i]
        assert toks[k].tolist() == w, f"{what}: row {i} ({sc.kinds[i]}): tokens {toks[k].tolist()} vs {w}"
        assert int(fin[k]) == f, f"{what}: row {i}: finish {fin[k]} vs {f}"
    n_out = [len(sc.want[i][0]) for i in idx]
    assert stats == dict(passes=max(rounds(k, ce) for k in n_out), row_passes=sum(rounds(k, ce) for k in n_out)), f"{what}: {stats}"
    for i in idx:
        if i in sc.vec:
            vec, ordered = devs[i].candidates()
            assert ordered and vec.tobytes() == sc.vec[i].tobytes(), f"{what}: row {i} ({sc.kinds[i]}): the sampler's vector after the call"
    return got


# ---------------------------------------------------------------------------------------------- 1. the launches alone

def op_case(rng, n, n0, state, ties):
    idx = np.sort(rng.choice(n, n0, replace=False))
    prob = (rng.integers(1, 6, n0) / np.float32(8 * max(n0, 1))).astype(np.float32) if ties else (rng.random(n0, np.float32) + np.float32(1e-3)) / np.float32(max(n0, 1))
    return TR.pairs(prob, idx)


@gpu
@pytest.mark.parametrize("n", [5, 4096, 8193, 20000])
def test_op_topp_rows_against_the_rule_and_the_host_sampler(L, n):
    """three chained calls per row (stale state in play), rows of different n0 in one call, 64 rows and 1 row"""
    rng = np.random.default_rng(n)
    n0s = sorted({k for k in (0, 1, 2, 63, 64, 65, n // 2, n) if k <= n})
    for n_rows in (64, 1):
        top_p = rng.choice(np.float32([0.05, 0.5, 0.9, 0.999]), n_rows)
        seeds = rng.integers(1, 1 << 30, n_rows)
        hosts = [L.Sampler(n, 1.0, float(top_p[r]), int(seeds[r])) for r in range(n_rows)]
        rnd = np.float32([h.info()[3] for h in hosts])
        state = np.zeros((n_rows, n), TR.PAIR)
        for r in range(0, n_rows, 3):                                 # every third row starts from a vector that is not all zero: large stale entries
            state[r] = TR.pairs(np.sort(rng.random(n, np.float32))[::-1] / np.float32(4), rng.permutation(n))
            hosts[r].set_candidates(state[r])
        for call in range(3):
            n0 = np.uint32([n0s[(r + call * 3) % len(n0s)] for r in range(n_rows)]) if n_rows > 1 else np.uint32([[n, n // 2, 0][call] if n > 5 else [5, 2, 0][call]])
            cand = np.zeros((n_rows, n), TR.PAIR)
            for r in range(n_rows):
                cand[r, :n0[r]] = op_case(rng, n, int(n0[r]), state[r], ties=r % 2 == 0)
            tok, status, new = L.op_topp_rows(cand, n0, top_p, rnd, state)
            for r in range(n_rows):
                wtok, wnew = TR.step(cand[r], int(n0[r]), state[r], top_p[r], rnd[r])
                htok, hnew = TR.host_step(L, hosts[r], cand[r], int(n0[r]))
                what = f"n {n}, {n_rows} rows, call {call}, row {r} (n0 {n0[r]})"
                assert wtok == htok and wnew.tobytes() == hnew.tobytes(), f"{what}: the rule and the host sampler disagree"
                assert int(status[r]) == (1 if wtok is None else 0) and int(tok[r]) == (wtok or 0), f"{what}: token {tok[r]} status {status[r]} vs {wtok}"
                assert new[r].tobytes() == wnew.tobytes(), f"{what}: the vector"
            state = new


@gpu
def test_op_topp_rows_on_the_hand_made_ties(L):
    for name, n, top_p, seed, steps, start in hand_cases():
        s = L.Sampler(n, 1.0, top_p, seed)
        state = (np.zeros(n, TR.PAIR) if start is None else start)[None, :]
        for k, (cand, n0) in enumerate(steps):
            full = np.zeros((1, n), TR.PAIR); full[0, :n0] = cand
            tok, status, new = L.op_topp_rows(full, [n0], [top_p], [s.info()[3]], state)
            wtok, wnew = TR.step(cand, n0, state[0], top_p, s.info()[3])
            assert int(status[0]) == (wtok is None) and int(tok[0]) == (wtok or 0) and new[0].tobytes() == wnew.tobytes(), f"{name}, step {k}"
            state = new


# ---------------------------------------------------------------------------------------------- 2. the loop

def batch_for(L, m, n, paged):
    return L.Batch(m, n, page_len=64, n_pages=n + 8) if paged else L.Batch(m, n, wide=n > 16)


@gpu
@pytest.mark.parametrize("n", [8, 20])
@pytest.mark.parametrize("paged", [False, True])
def test_the_loop_with_mixed_samplers(L, n, paged):
    sc = scene(n)
    assert len(sc.stale) >= 2 and sc.frozen, "vacuous: see test_the_loop_cases_are_not_vacuous"
    m = L.Transformer(image()); b = batch_for(L, m, n, paged)
    for i, r in enumerate(sc.rows):
        if len(sc.prompts[i]):
            b.prefill(r.slot, sc.prompts[i], 0)
    for ce in (4, 1):
        check_topp_call(L, b, sc, ce, f"{'paged' if paged else 'contiguous'} {n} rows check_every {ce}")
    for i, r in enumerate(sc.rows):
        check_slot_rows(b, r, sorted({sc.depths[i], sc.depths[i] + len(sc.want[i][0]) - 1}), f"{n} rows")
    # lmrs_batch_generate itself still refuses the row, and takes the call without it
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_generate: row 2: a top-p sampler \(top_p = 0\.99"):
        b.generate([r.slot for r in sc.rows], sc.firsts, sc.depths, sc.budgets, samplers=dev_samplers(L, sc))
    b.close()


# ---------------------------------------------------------------------------------------------- 4. continuation

@gpu
def test_two_calls_and_a_sampled_step_continue_one_run(L):
    m = L.Transformer(image()); b = L.Batch(m, 3)
    kinds = [(0.15, 0.99, 38), (1.0, 0.9, 21), (1.0, 0.05, 22)]
    rows = [Row(L, image(), i) for i in range(3)]
    devs = [arm(L.Sampler, k, i == 0) for i, k in enumerate(kinds)]
    for i, r in enumerate(rows):
        r.ref = arm(O.Sampler, kinds[i], i == 0)
        r.prefill(b, S.prompt_tokens(CFG, 4 + i, 830 + i))
    depths = [r.n for r in rows]
    firsts = [17, 170, 1700]
    outs = [r.continuation(firsts[i], 5 + 4 + 1)[0] for i, r in enumerate(rows)]
    t1, f1, _ = b.generate_topp([0, 1, 2], firsts, depths, 5, samplers=devs, check_every=4)
    t2, f2, _ = b.generate_topp([0, 1, 2], [int(t[-1]) for t in t1], [d + 5 for d in depths], 4, samplers=devs, check_every=3)
    nxt = b.forward_runs_sample([(i, depths[i] + 9, [int(t2[i][-1])], devs[i]) for i in range(3)])
    for i in range(3):
        got = t1[i].tolist() + t2[i].tolist() + [int(nxt[i])]
        assert got == outs[i], f"row {i} ({kinds[i]}): {got} vs {outs[i]}"
    assert f1.tolist() == f2.tolist() == [BUDGET] * 3
    for i, r in enumerate(rows):
        check_slot_rows(b, r, [depths[i] + 9], "the step after the two calls")
    b.close()


# ---------------------------------------------------------------------------------------------- 5. no candidate

NONE_KIND = (1.0e6, 1.0e-5, 3)                                  # every probability is about 1 / V, below the cutoff (1 - top_p) / (V - 1)


@gpu
def test_a_row_without_a_candidate_ends_with_its_own_code(L):
    m = L.Transformer(image()); b = L.Batch(m, 4)
    b.set_history(0)
    kinds = [None, NONE_KIND, (0.15, 0.99, 38), (0.8, 1.0, 11)]
    rows = [Row(L, image(), i) for i in range(4)]
    for i, r in enumerate(rows):
        r.ref = arm(O.Sampler, kinds[i], i == 2) if kinds[i] else None
        r.prefill(b, S.prompt_tokens(CFG, 3 + i, 840 + i))
    depths = [r.n for r in rows]
    firsts = [9, 90, 900, 1900]
    # the CPU first: the reference's sampler reports the failure for exactly that step
    failed = rows[1].feed(firsts[1])
    with pytest.raises(RuntimeError, match="no candidate above the cutoff"):
        rows[1].ref.sample(failed.copy())
    assert n0_of(failed, NONE_KIND) == 0
    outs = {i: rows[i].continuation(firsts[i], 6)[0] for i in (0, 2, 3)}
    devs = [arm(L.Sampler, k, i == 2) if k else None for i, k in enumerate(kinds)]
    held = TR.pairs(np.sort(np.random.default_rng(5).random(V, np.float32))[::-1] / np.float32(8), np.random.default_rng(6).permutation(V))
    devs[1].set_candidates(held)
    for ce in (4, 1):
        devs[2] = arm(L.Sampler, kinds[2], True)
        toks, fin, stats = b.generate_topp([0, 1, 2, 3], firsts, depths, 6, samplers=devs, check_every=ce)
        assert fin.tolist() == [BUDGET, NO_CANDIDATE, BUDGET, BUDGET] and L.FINISH_NO_CANDIDATE == NO_CANDIDATE
        assert toks[1].size == 0, "the step without a candidate reports no token"
        for i in (0, 2, 3):
            assert toks[i].tolist() == outs[i], f"check_every {ce}: row {i} beside the row that ended: {toks[i].tolist()} vs {outs[i]}"
        assert stats == dict(passes=rounds(6, ce), row_passes=3 * rounds(6, ce) + rounds(1, ce)), stats
        vec, ordered = devs[1].candidates()
        assert ordered and vec.tobytes() == held.tobytes(), "the failed step changed the sampler's vector"
        # the forward ran: its K/V row and record entry are written
        check_slot_rows(b, rows[1], [depths[1]], "the row without a candidate")
        assert b.history(1, 1, depths[1]).tolist() == [firsts[1]]
    # the batch is usable afterwards, the ended row's slot included
    rows[1].rewind(depths[1])
    rows[1].ref = None
    want = rows[1].continuation(firsts[1], 3)[0]
    toks, fin, _ = b.generate_topp([1], [firsts[1]], [depths[1]], 3)
    assert toks[0].tolist() == want and fin.tolist() == [BUDGET]
    b.close()


# ---------------------------------------------------------------------------------------------- 6. log-probabilities, masks and penalties

@gpu
def test_logprobs_masks_and_penalties_with_topp_rows(L):
    m = L.Transformer(image()); b = L.Batch(m, 5)
    b.set_history(0)
    kinds = [(0.15, 0.99, 38), (1.0, 0.9, 21), (1.0, 0.05, 22), (0.8, 1.0, 11), None]
    rows = [Row(L, image(), i) for i in range(5)]
    rows[1].mask, rows[2].mask = ban(V, range(100, 200)), ban(V, range(1000, 1100))
    b.set_masks([1, 2], np.stack([rows[1].mask, rows[2].mask]))
    rows[2].par, rows[3].par = params("all"), params("rep")
    b.set_penalties([2, 3], *([rows[i].par[k] for i in (2, 3)] for k in ("repetition", "presence", "frequency", "out_from")))
    for i, r in enumerate(rows):
        r.ref = arm(O.Sampler, kinds[i], i == 0) if kinds[i] else None
        r.prefill(b, S.prompt_tokens(CFG, [6, 0, 30, 3, 1][i], 850 + i))
    depths = [r.n for r in rows]
    firsts, budgets = [3, 400, 77, 1000, 21], [5, 7, 9, 12, 12]
    conts = [r.continuation(firsts[i], budgets[i]) for i, r in enumerate(rows)]
    outs = [c[0] for c in conts]
    stops = [[outs[0][1]], [], [outs[2][4]], [], [outs[4][8]]]
    want = expect(rows, firsts, outs, budgets, stops)
    not_vacuous(want, (3,))
    for lp in (False, True):
        devs = [arm(L.Sampler, k, i == 0) if k else None for i, k in enumerate(kinds)]
        got = b.generate_topp([0, 1, 2, 3, 4], firsts, depths, budgets, stop=stops, samplers=devs, check_every=3, logprobs=lp)
        for i, (w, f) in enumerate(want):
            assert got[0][i].tolist() == w and int(got[1][i]) == f, f"logprobs {lp}: row {i} ({kinds[i]}): {got[0][i].tolist()} vs {w}"
    for i in range(5):
        k = len(want[i][0])
        assert got[2][i].shape == (k,) and np.all(np.isfinite(got[2][i])) and np.all(got[2][i] <= 0)
        assert_within_one_ulp(got[2][i], want_logprobs(conts[i][1][:k], want[i][0]), f"log-probabilities, row {i} ({kinds[i]})")
    assert all(int(t) not in range(100, 200) for t in got[0][1]) and all(int(t) not in range(1000, 1100) for t in got[0][2])
    b.close()


# ---------------------------------------------------------------------------------------------- 7. errors

@gpu
def test_errors_come_before_device_work_and_leave_everything_usable(L):
    m = L.Transformer(image()); b = L.Batch(m, 3)
    r = Row(L, image(), 0); r.prefill(b, S.prompt_tokens(CFG, 6, 604))
    kind = (0.15, 0.99, 38)
    r.ref = arm(O.Sampler, kind, True)
    good_out, _ = r.continuation(5, 3)
    T = m.args.seq_len
    lib = L.lib()

    def good(what):
        toks, fin, stats = b.generate_topp([0], [5], [6], 3, stop=[V - 1], samplers=[arm(L.Sampler, kind, True)])
        assert toks[0].tolist() == good_out and fin.tolist() == [BUDGET], what

    good("first")
    topp, other, mult = L.Sampler(V, 0.8, 0.9, 1), L.Sampler(V - 1, 0.8, 0.9, 1), L.Sampler(V, 0.8, 1.0, 1)
    unordered = L.Sampler(V, 0.8, 0.9, 2)
    vec = unordered.candidates()[0]; vec["prob"][7] = 0.5
    unordered.set_candidates(vec)
    before = topp.candidates()[0].tobytes()
    name = "lmrs_batch_generate_topp: "
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
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=2, samplers=[topp, topp]), "row 1: the top-p sampler of row 0 appears twice"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=2, samplers=[None, other]), "row 1: the sampler was made for another vocabulary size"),
        (dict(slots=[0, 1], tokens=[1, 2], pos=[6, 0], max_new=2, samplers=[topp, unordered]), "row 1: the top-p sampler's candidate vector is not in descending order"),
    ]
    for kw, msg in cases:
        with pytest.raises(L.LmrsError) as e:
            b.generate_topp(**kw)
        assert str(e.value).startswith(name + msg), (msg, str(e.value))
        assert topp.candidates()[0].tobytes() == before, f"after {msg!r}: a refused call changed a sampler"
        good(f"after {msg!r}")
    # a NULL required array, and n_stop without stop_tokens: straight at the C entry point
    u32 = lambda *v: np.array(v, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    a, out = u32(0), np.zeros(4, np.uint32)
    full = [b._h, 1, p(a), p(u32(5)), p(u32(6)), p(u32(2)), None, None, None, 1, p(out), None, p(out), p(out), None, None]
    for k in (2, 3, 4, 5, 10, 12, 13):
        args = list(full); args[k] = None
        assert lib.lmrs_batch_generate_topp(*args) != 0 and lib.lmrs_last_error().decode().startswith(name + "NULL array"), k
    args = list(full); args[6] = p(u32(1))
    assert lib.lmrs_batch_generate_topp(*args) != 0 and lib.lmrs_last_error().decode().startswith(name + "n_stop given without stop_tokens")
    good("after the NULL arguments")
    # lmrs_batch_generate with a top-p sampler: still refused, with its old message
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_generate: row 1: a top-p sampler \(top_p = 0\.9.*cannot run in the device loop: its candidate vector lives in the host sampler"):
        b.generate([0, 1], [1, 2], [6, 0], 2, samplers=[mult, topp])
    good("after lmrs_batch_generate's refusal")
    b.close()
