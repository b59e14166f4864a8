"""Allowed-token masks on batch slots (lmrs_batch_set_masks / _clear_masks / _mask_info, include/lmrs_hip.h): while a slot has a mask, every output
row of it - logits, argmax, top-k, sampled token - comes from the row's logits with the disallowed entries -inf.  The reference is one CPU oracle PER
SEQUENCE; its logits row is masked in numpy (-inf at the cleared bits) before Sampler::sample (the oracle's), sample_argmax (lmrs_ref_argmax) or the
top-k definition (tests/test_topk.py's rank_row / topk_rule).  Every comparison is exact: logits bit for bit, tokens and indices by value; the top-k
log-probabilities by test_topk's own rule."""
import ctypes
import dataclasses

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from test_batch import Seq as TokenSeq, prefilled
from test_batch_embed import token_rows
from test_batch_sample import KINDS, SORT_MIN, Seq as SampledSeq, n0_of
from test_topk import rank_row, topk_rule
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
NINF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


# ---------------------------------------------------------------------------------------------- the masks

def ban(V, toks):
    m = np.ones(V, np.bool_); m[np.asarray(toks, np.int64)] = False
    return m


def allow(V, toks):
    m = np.zeros(V, np.bool_); m[np.asarray(toks, np.int64)] = True
    return m


def mask_of_kind(kind, V, row, i=0):
    """kind: "ban" - a few tokens, the unmasked argmax of `row` (the oracle's) and its runner-up among them, so the mask provably changes the answer;
    "allow3"; "single" (the token is forced); the edge patterns "only31" / "only32" / "only0" / "last"; "alt" - every word 0x55555555, so each group of
    four columns is mixed; None: no mask"""
    if kind is None:
        return None
    if kind == "ban":
        order = rank_row(row)
        return ban(V, [int(order[0]), int(order[1]), (5 + 37 * i) % V, (1000 + i) % V, V - 1 - i])
    if kind == "allow3":
        return allow(V, [(7 + 3 * i) % V, (1234 + 5 * i) % V, (V - 2 - i) % V])
    if kind == "single":
        return allow(V, [(777 + 11 * i) % V])
    if kind == "alt":
        m = np.zeros(V, np.bool_); m[0::2] = True
        return m
    return allow(V, [{"only31": 31, "only32": 32, "only0": 0, "last": V - 1}[kind]])


ALL_KINDS = ["ban", "allow3", "single", "only31", "only32", "only0", "last", "alt"]


def masked(row, mask):
    """the oracle's row as the sinks see it under `mask`"""
    row = np.asarray(row, np.float32)
    return row.copy() if mask is None else np.where(mask, row, NINF).astype(np.float32)


def set_masks(b, seqs, masks):
    """masks[i] (bool [V] or None) for seqs[i]'s slot: the masked ones in one call, the others cleared"""
    on = [i for i, m in enumerate(masks) if m is not None]
    off = [seqs[i].slot for i, m in enumerate(masks) if m is None]
    if on:
        b.set_masks([seqs[i].slot for i in on], np.stack([masks[i] for i in on]))
    b.clear_masks(off)
    for i, s in enumerate(seqs):
        assert b.mask_info(s.slot) == (None if masks[i] is None else int(masks[i].sum()))


def check_row(lg, am, want, mask, what, changed=False):
    exp = masked(want, mask)
    assert_bit_equal(lg, exp, f"{what}: logits")
    if mask is not None:
        assert np.array_equal(np.isneginf(lg), ~mask), f"{what}: -inf is not exactly at the cleared bits"
    assert int(am) == ref_argmax(exp), f"{what}: argmax {am} vs {ref_argmax(exp)}"
    if changed:
        assert int(am) != ref_argmax(want), f"{what}: the ban-list did not change the argmax"


# ---------------------------------------------------------------------------------------------- 1. forward

DEPTHS16 = [0, 1, 7, 63, 64, 65, 127, 128, 129, 200, 2, 31, 32, 33, 96, 5]
FORWARD_KINDS = ALL_KINDS + ["ban", "allow3", None, None, "alt", None, "single", None]


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_forward_rows_under_masks(L, cfg, q):
    """16 rows at the depths the attention forms change at, masked and unmasked rows in one pass (mini-gemma: the soft cap in front of the mask); a
    second batch on the same model that never had a mask gives the unmasked rows' bits"""
    img = S.build_image(cfg, q, seed=401)
    m, b, seqs = prefilled(L, img, cfg, DEPTHS16, 402)
    plain = L.Batch(m, 16)
    for i, n in enumerate(DEPTHS16):
        if n:
            plain.prefill(i, S.prompt_tokens(cfg, n, 402 + i), 0)
    V = seqs[0].orc.args.vocab_size
    toks = [(13 * i + 3) % V for i in range(16)]
    for step, order in enumerate((list(range(16)), list(range(15, -1, -1))[:11])):
        rows = [seqs[i] for i in order]
        pos = [s.n for s in rows]
        want = [s.feed([toks[s.slot]]) for s in rows]
        kinds = [FORWARD_KINDS[(s.slot + 3 * step) % 16] for s in rows]
        masks = [mask_of_kind(k, V, w, s.slot) for k, w, s in zip(kinds, want, rows)]
        set_masks(b, rows, masks)
        slots = [s.slot for s in rows]
        am, lg = b.forward(slots, [toks[s] for s in slots], pos, logits=True)
        am0, lg0 = plain.forward(slots, [toks[s] for s in slots], pos, logits=True)
        for i, s in enumerate(rows):
            what = f"{cfg} q{q} step {step} row {i} (slot {s.slot}, pos {pos[i]}, {kinds[i]})"
            check_row(lg[i], am[i], want[i], masks[i], what, changed=kinds[i] == "ban")
            assert_bit_equal(lg0[i], want[i], f"{what}: the batch without masks")
            if masks[i] is None:
                assert_bit_equal(lg[i], lg0[i], f"{what}: an unmasked row beside masked ones")
                assert int(am[i]) == int(am0[i]), what
            toks[s.slot] = int(am[i])
    b.close(); plain.close()


# ---------------------------------------------------------------------------------------------- 2. forward_runs

def runs_call(b, entries, kinds, k, what):
    """one forward_runs over entries = [(seq, tokens, n_out)], logits on, under masks of `kinds` (one per entry; a ban-list holds the oracle's unmasked
    argmax of the run's last row), judged against the oracles"""
    V = entries[0][0].orc.args.vocab_size
    runs = [(s.slot, s.n, toks, n_out) for s, toks, n_out in entries]
    wants = [[s.feed([t]) for t in toks] for s, toks, _ in entries]
    masks = [mask_of_kind(kd, V, w[-1], e[0].slot) for kd, w, e in zip(kinds, wants, entries)]
    set_masks(b, [e[0] for e in entries], masks)
    got = b.forward_runs(runs, k=k, logits=True)
    am, lg = got[0], got[1]
    o = 0
    for (s, toks, n_out), want, mask, kd in zip(entries, wants, masks, kinds):
        for j in range(len(toks) - n_out, len(toks)):
            where = f"{what}: slot {s.slot} ({kd}) output row {o}"
            check_row(lg[o], am[o], want[j], mask, where, changed=kd == "ban" and j == len(toks) - 1)
            if k:
                ti, tl = got[2], got[3]
                exp = masked(want[j], mask)
                assert ti[o].tolist() == rank_row(exp)[:k].tolist(), f"{where}: top-{k} indices"
                if mask is not None:
                    assert mask[ti[o]].all(), f"{where}: a disallowed token among the top {k}"
                    if int(mask.sum()) == k:
                        assert set(ti[o].tolist()) == set(np.flatnonzero(mask).tolist()), f"{where}: the index set is not the allow-list"
                with np.errstate(all="ignore"):
                    topk_rule(tl[o:o + 1], ti[o:o + 1], exp[None, :], where)
            o += 1
    assert o == am.size


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_forward_runs_under_masks(L, cfg, q):
    """prompts of 1, 5 and 17 tokens beside two decode rows in one pass; n_out = 3 on a masked run; k = 3 under a 3-token allow-list, k = 20 under a ban-list"""
    img = S.build_image(cfg, q, seed=403)
    m, b, seqs = prefilled(L, img, cfg, [0, 0, 0, 9, 70], 404)
    V = seqs[0].orc.args.vocab_size
    prompt = lambda i, n: S.prompt_tokens(cfg, n, 900 + i).tolist()
    lens = [1, 5, 17, 1, 1]
    # the forced and the edge masks, no top-k (k would exceed n_allowed)
    runs_call(b, [(s, prompt(s.slot, lens[s.slot]), (1, 2, 3, 1, 1)[s.slot]) for s in seqs], ["single", "only31", "only32", "only0", "last"], 0, f"{cfg} q{q} forced")
    # k = 3: the allow-list of 3 on the 17-token run with three outputs and on a decode row
    runs_call(b, [(s, prompt(10 + s.slot, lens[(s.slot + 1) % 3] if s.slot < 3 else 1), (1, 3, 1, 1, 1)[s.slot]) for s in seqs][::-1],
              ["ban", "allow3", "alt", "allow3", None][::-1], 3, f"{cfg} q{q} k = 3")
    # k = 20 on ban-list rows (and the alternating mask, and a row without one)
    runs_call(b, [(s, prompt(20 + s.slot, lens[(s.slot + 2) % 3] if s.slot < 3 else 1), (2, 1, 1, 1, 1)[s.slot]) for s in seqs], ["ban", "alt", "ban", None, "ban"], 20, f"{cfg} q{q} k = 20")
    b.close()


# ---------------------------------------------------------------------------------------------- 3. the sampled passes

WIDE_KINDS = ["ban", "allow3", "single", "only31", "only32", "only0", "last", "alt", None, "ban", None]        # 11: every pairing with the six sampler kinds


def sampled_call(b, rows, last, masks, wide, what):
    """one forward_runs_sample (wide) or forward_sample over `rows`, each fed its own last token -> the n0 of the top-p rows, by slot"""
    if wide:
        got = b.forward_runs_sample([(s.slot, s.n, [last[s.slot]], s.dev) for s in rows])
    else:
        got = b.forward_sample([s.slot for s in rows], [last[s.slot] for s in rows], [s.n for s in rows], [s.dev for s in rows])
    want, n0 = [], {}
    for s in rows:
        lg = masked(s.feed([last[s.slot]]), masks[s.slot])
        want.append(s.ref.sample(lg))                                                 # (lg: the probabilities now)
        if s.kind[0] != 0.0 and 0.0 < s.kind[1] < 1.0:
            n0[s.slot] = n0_of(lg, s.kind[1])
    assert got.tolist() == want, f"{what}: tokens {got.tolist()} vs the oracle's {want}"
    for s, t in zip(rows, got.tolist()):
        last[s.slot] = t
    return n0


@gpu
def test_sampled_passes_under_masks(L):
    """forward_runs_sample on a wide batch at 64, 48 and 17 runs and forward_sample at 16 rows, the six sampler kinds and eleven mask kinds cycling over the
    slots, every row fed its own token, two rounds.  (The vocabulary of 4096 is the sort threshold itself: an unmasked (3.0, 0.999) row is sorted on the
    device, one under a 3-token allow-list is finished on the host; a masked row that stays flat needs the larger vocabulary of the next test.)"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=405)
    m = L.Transformer(img); b = L.Batch(m, 64, wide=True)
    seqs = []
    for i in range(64):
        s = SampledSeq(L, img, i, KINDS[i % 6], 4000 + i)
        if i % 3:
            toks = S.prompt_tokens(cfg, i % 3, 50 + i)
            b.prefill(i, toks, 0); s.feed(toks)
        seqs.append(s)
    V = 4096
    last = {i: (13 * i + 3) % V for i in range(64)}
    probe = O.Oracle(img).forward(3, 0).copy()
    masks = {i: mask_of_kind(WIDE_KINDS[i % 11], V, probe, i) for i in range(64)}
    set_masks(b, seqs, [masks[i] for i in range(64)])
    flat_masked, flat_plain = set(), set()
    for k in range(2):
        for rows, wide in ((seqs, True), (seqs[8:56], True), (seqs[:17], True), (seqs[40:56][::-1], False)):
            n0 = sampled_call(b, rows, last, masks, wide, f"round {k}, {len(rows)} {'runs' if wide else 'rows'}")
            for slot, n in n0.items():
                if seqs[slot].kind == (3.0, 0.999):
                    (flat_plain if masks[slot] is None else flat_masked).add((WIDE_KINDS[slot % 11], n >= SORT_MIN))
    assert flat_plain == {(None, True)}, flat_plain                                   # the device sort ran (slot 41)
    assert ("allow3", False) in flat_masked and all(not dev for _, dev in flat_masked), flat_masked
    b.close()


@gpu
def test_both_candidate_routes_under_masks(L):
    """vocabulary 40 000: a ban-list leaves a (3.0, 0.999) row flat - at least SORT_MIN candidates, sorted on the device - and a 3-token allow-list takes
    another such row below it, finished on the host; in forward_sample and in forward_runs_sample"""
    cfg = "mini-llama-v40k"
    img = S.build_image(cfg, S.Q8_0, seed=406)
    V = 40000
    kinds = [(3.0, 0.999), (3.0, 0.999), (3.0, 0.999), (0.7, 0.9), (0.0, 0.9), (0.8, 1.0)]
    m = L.Transformer(img); b = L.Batch(m, 6, wide=True)
    seqs = [SampledSeq(L, img, i, kinds[i], 4100 + i) for i in range(6)]
    probe = O.Oracle(img).forward(3, 0).copy()
    mk = ["ban", "allow3", None, "alt", "ban", "single"]
    masks = {i: mask_of_kind(mk[i], V, probe, i) for i in range(6)}
    set_masks(b, seqs, [masks[i] for i in range(6)])
    last = {i: (13 * i + 3) % V for i in range(6)}
    seen = {0: set(), 1: set(), 2: set()}
    for k, wide in enumerate((False, True, True, False)):
        n0 = sampled_call(b, seqs if k % 2 == 0 else seqs[::-1], last, masks, wide, f"v40k call {k}")
        for i in seen:
            seen[i].add(n0[i] >= SORT_MIN)
    assert seen == {0: {True}, 1: {False}, 2: {True}}, seen
    b.close()


# ---------------------------------------------------------------------------------------------- 4. generate_greedy

@gpu
@pytest.mark.parametrize("n,n_new", [(8, 12), (17, 4)])
def test_generate_greedy_under_ban_masks(L, n, n_new):
    """each row's ban-list is what its unmasked run produced: every step against the oracle loop under the same mask (17 rows: the long table's loop)"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=407)
    depths = [(0, 1, 7, 63, 64, 65, 2, 30)[i % 8] for i in range(n)]
    m = L.Transformer(img); b = L.Batch(m, n, wide=n > 16)
    seqs = []
    for i, d in enumerate(depths):
        s = TokenSeq(img, i)
        if d:
            toks = S.prompt_tokens(cfg, d, 408 + i)
            b.prefill(i, toks, 0); s.feed(toks)
        seqs.append(s)
    V = 4096
    slots = list(range(n)); toks = [(13 * i + 3) % V for i in range(n)]
    free = b.generate_greedy(slots, toks, depths, n_new)
    masks = [ban(V, free[i]) for i in range(n)]
    b.set_masks(slots, np.stack(masks))
    got = b.generate_greedy(slots, toks, depths, n_new)
    for i, s in enumerate(seqs):
        t = toks[i]
        for j in range(n_new):
            t = ref_argmax(masked(s.orc.forward(int(t), depths[i] + j), masks[i]))
            assert int(got[i, j]) == t, f"row {i} step {j}: {got[i, j]} vs the oracle's {t}"
        assert not set(got[i].tolist()) & set(free[i].tolist()), f"row {i}: a banned token was produced"
        assert got[i, 0] != free[i, 0]
    b.clear_masks()
    assert np.array_equal(b.generate_greedy(slots, toks, depths, n_new), free), "the unmasked run after clear_masks"
    b.close()


# ---------------------------------------------------------------------------------------------- 5. state

@gpu
def test_mask_state(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=409)
    m, b, seqs = prefilled(L, img, cfg, [3, 0, 9, 1], 410)
    V = 4096
    row = O.Oracle(img).forward(5, 0).copy()
    assert [b.mask_info(i) for i in range(4)] == [None] * 4

    def step(masks, what):
        pos = [s.n for s in seqs]
        toks = [(17 * s.slot + pos[s.slot]) % V for s in seqs]
        am, lg = b.forward([0, 1, 2, 3], toks, pos, logits=True)
        for i, s in enumerate(seqs):
            check_row(lg[i], am[i], s.feed([toks[i]]), masks[i], f"{what}: slot {i}")

    # a mask on a slot that is not in the call changes nothing
    b.set_masks([3], mask_of_kind("single", V, row)[None, :])
    assert b.mask_info(3) == 1
    am, lg = b.forward([0, 2], [11, 12], [seqs[0].n, seqs[2].n], logits=True)
    for i, s in enumerate((seqs[0], seqs[2])):
        check_row(lg[i], am[i], s.feed([11 + i]), None, f"slot {s.slot} beside a masked slot that is not in the call")
    # packed words are taken as they are; bits at and above vocab_size would be ignored (4096 has none: the word count is checked on the host side)
    alt, a3 = mask_of_kind("alt", V, row), mask_of_kind("allow3", V, row)
    b.set_masks([0, 2], L.pack_mask(np.stack([alt, a3])))
    assert [b.mask_info(i) for i in range(4)] == [V // 2, None, 3, 1]
    step([alt, None, a3, mask_of_kind("single", V, row)], "three masks")
    # set_masks twice replaces the mask
    b1 = mask_of_kind("ban", V, row, 1)
    b.set_masks([2], b1[None, :])
    assert b.mask_info(2) == int(b1.sum()) >= V - 5
    step([alt, None, b1, mask_of_kind("single", V, row)], "slot 2 replaced")
    # fork leaves the destination's mask (and the source's) as it was: slot 1 gets slot 0's rows, not its mask; slot 3 keeps its own over slot 2's rows
    b.fork(0, 1, seqs[0].n); b.fork(2, 3, seqs[2].n)
    assert [b.mask_info(i) for i in range(4)] == [V // 2, None, int(b1.sum()), 1]
    pos = [seqs[0].n, seqs[2].n]
    am, lg = b.forward([1, 3], [21, 22], pos, logits=True)
    for i, (src, mask) in enumerate(((seqs[0], None), (seqs[2], mask_of_kind("single", V, row)))):
        want = src.orc.forward(21 + i, pos[i]).copy()                                 # (the source's oracle one row ahead: the next feed overwrites the row)
        check_row(lg[i], am[i], want, mask, f"fork destination {(1, 3)[i]}")
    # clear_masks per slot, then for all
    b.clear_masks([0])
    assert [b.mask_info(i) for i in range(4)] == [None, None, int(b1.sum()), 1]
    am, lg = b.forward([0, 2], [31, 32], pos, logits=True)
    for i, (s, mask) in enumerate(((seqs[0], None), (seqs[2], b1))):
        check_row(lg[i], am[i], s.feed([31 + i]), mask, f"slot {s.slot} after clear_masks([0])")
    b.clear_masks()
    assert [b.mask_info(i) for i in range(4)] == [None] * 4
    am, lg = b.forward([0, 2], [41, 42], [seqs[0].n, seqs[2].n], logits=True)
    for i, s in enumerate((seqs[0], seqs[2])):
        check_row(lg[i], am[i], s.feed([41 + i]), None, f"slot {s.slot} after clear_masks()")
    b.close()


# ---------------------------------------------------------------------------------------------- 6. paged

@gpu
def test_a_paged_batch_gives_the_wide_batch_under_the_same_masks(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=411)
    m = L.Transformer(img)
    wide, paged = L.Batch(m, 20, wide=True), L.Batch(m, 20, page_len=64, n_pages=48)
    V = 4096
    depths = [(0, 1, 63, 64, 65, 100)[i % 6] for i in range(20)]
    row = O.Oracle(img).forward(5, 0).copy()
    masks = [mask_of_kind((ALL_KINDS + [None, None])[i % 10], V, row, i) for i in range(20)]
    on = [i for i in range(20) if masks[i] is not None]
    samplers = {id(x): [L.Sampler(V, *KINDS[i % 6], 4200 + i) for i in range(20)] for x in (wide, paged)}

    def fill(slots):
        for x in (wide, paged):
            for i in slots:
                if depths[i]:
                    x.prefill(i, S.prompt_tokens(cfg, depths[i], 412 + i), 0)

    def both(what, slots):
        outs = []
        for x in (wide, paged):
            pos = [depths[i] for i in slots]
            am, lg = x.forward(slots, [(7 * i + 1) % V for i in slots], pos, logits=True)                     # 20 rows: the long table
            r_am, r_lg, ti, tl = x.forward_runs([(i, depths[i] + 1, [5 + i, 6 + i, 7 + i], 2) for i in slots if masks[i] is None or masks[i].sum() >= 3], k=3, logits=True)
            nxt = x.forward_runs_sample([(i, depths[i] + 4, [9 + i], samplers[id(x)][i]) for i in slots])
            gg = x.generate_greedy(slots[:16], [3 + i for i in slots[:16]], [depths[i] + 5 for i in slots[:16]], 3)
            outs.append((am, lg, r_am, r_lg, ti, tl, nxt, gg))
        for name, a, p in zip(("argmax", "logits", "runs argmax", "runs logits", "top-k indices", "top-k log-probabilities", "sampled", "greedy"), *outs):
            assert_bit_equal(p, a, f"{what}: {name} of the paged batch against the wide batch")
        lg = outs[1][1]
        for r, i in enumerate(slots):
            if masks[i] is not None:
                assert np.array_equal(np.isneginf(lg[r]), ~masks[i]), f"{what}: slot {i}: -inf is not exactly at the cleared bits"
            else:
                assert np.isfinite(lg[r]).all()

    for x in (wide, paged):
        x.set_masks(on, np.stack([masks[i] for i in on]))
    fill(range(20))
    both("first", list(range(20)))
    # a release empties slots of the paged batch; filled again they give the wide batch's rows, under the masks they kept
    for i in (2, 4, 11):
        paged.release(i, 0)
        assert paged.mask_info(i) == (None if masks[i] is None else int(masks[i].sum()))
    fill((2, 4, 11))
    both("after release", list(range(19, -1, -1)))
    wide.close(); paged.close()


# ---------------------------------------------------------------------------------------------- 7. an embedding run with outputs

@gpu
def test_an_embedding_run_with_outputs_under_a_mask(L):
    cfg = "mini-phi"
    img = S.build_image(cfg, S.Q8_0, seed=413)
    m, b, seqs = prefilled(L, img, cfg, [4, 0], 414)
    V = 4096
    toks = S.prompt_tokens(cfg, 6, 415).tolist()
    rows = token_rows(seqs[0].orc, toks)                                              # the rows Transformer::forward would build: the oracle is fed the tokens
    want = [seqs[0].feed([t]) for t in toks][-2:] + [seqs[1].feed([9])]
    masks = [mask_of_kind("ban", V, want[1], 0), mask_of_kind("allow3", V, want[2], 1)]
    b.set_masks([0, 1], np.stack(masks))
    am, lg, ti, tl = b.forward_runs([(0, 4, rows, 2), (1, 0, [9], 1)], k=3, logits=True)
    for o, mask in enumerate((masks[0], masks[0], masks[1])):
        check_row(lg[o], am[o], want[o], mask, f"output row {o}", changed=o == 1)
        assert ti[o].tolist() == rank_row(masked(want[o], mask))[:3].tolist(), f"output row {o}: top-3 indices"
    # ... and sampled: the embedding run's last row under the ban-list
    dev, ref = L.Sampler(V, 0.8, 1.0, 7), O.Sampler(V, 0.8, 1.0, 7)
    more = S.prompt_tokens(cfg, 3, 416).tolist()
    nxt = b.forward_runs_sample([(0, seqs[0].n, token_rows(seqs[0].orc, more), dev)])
    assert int(nxt[0]) == ref.sample(masked(seqs[0].feed(more), masks[0]))
    b.close()


# ---------------------------------------------------------------------------------------------- 8. refusals

@gpu
def test_refusals_come_before_device_work_and_leave_everything_usable(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=417)
    m, b, seqs = prefilled(L, img, cfg, [2, 0, 1], 418)
    lib = L.lib()
    V, W = 4096, 128
    row = O.Oracle(img).forward(5, 0).copy()
    a3 = mask_of_kind("allow3", V, row)
    b.set_masks([1], a3[None, :])
    masks = [None, a3, None]

    def valid(what):
        pos = [s.n for s in seqs]
        am, lg = b.forward([0, 1, 2], [1, 2, 3], pos, logits=True)
        for i, s in enumerate(seqs):
            check_row(lg[i], am[i], s.feed([1 + i]), masks[i], f"{what}: slot {i}")
        assert [b.mask_info(i) for i in range(3)] == [None, 3, None], what

    u32 = lambda *v: np.array(v, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    ones = np.full((17, W), 0xFFFFFFFF, np.uint32)
    none_allowed = ones[:2].copy(); none_allowed[1] = 0
    valid("first")
    cases = [
        (lambda: lib.lmrs_batch_set_masks(None, 1, p(u32(0)), p(ones)), "lmrs_batch_set_masks: NULL argument"),
        (lambda: lib.lmrs_batch_set_masks(b._h, 1, None, p(ones)), "lmrs_batch_set_masks: NULL array"),
        (lambda: lib.lmrs_batch_set_masks(b._h, 1, p(u32(0)), None), "lmrs_batch_set_masks: NULL array"),
        (lambda: lib.lmrs_batch_set_masks(b._h, 17, p(np.arange(17, dtype=np.uint32)), p(ones)), "lmrs_batch_set_masks: n = 17 exceeds the batch's width of 16"),
        (lambda: lib.lmrs_batch_set_masks(b._h, 2, p(u32(0, 3)), p(ones)), "lmrs_batch_set_masks: mask 1: slot 3 of 3"),
        (lambda: lib.lmrs_batch_set_masks(b._h, 2, p(u32(2, 2)), p(ones)), "lmrs_batch_set_masks: slot 2 appears twice"),
        (lambda: lib.lmrs_batch_set_masks(b._h, 2, p(u32(0, 2)), p(none_allowed)), "lmrs_batch_set_masks: mask 1: slot 2 would have no allowed token below vocab_size"),
        (lambda: lib.lmrs_batch_clear_masks(None, 0, None), "lmrs_batch_clear_masks: NULL argument"),
        (lambda: lib.lmrs_batch_clear_masks(b._h, 1, None), "lmrs_batch_clear_masks: NULL array"),
        (lambda: lib.lmrs_batch_clear_masks(b._h, 17, p(np.arange(17, dtype=np.uint32))), "lmrs_batch_clear_masks: n = 17 exceeds the batch's width of 16"),
        (lambda: lib.lmrs_batch_clear_masks(b._h, 1, p(u32(3))), "lmrs_batch_clear_masks: mask 0: slot 3 of 3"),
        (lambda: lib.lmrs_batch_clear_masks(b._h, 2, p(u32(1, 1))), "lmrs_batch_clear_masks: slot 1 appears twice"),
        (lambda: lib.lmrs_batch_mask_info(None, 0, ctypes.byref(ctypes.c_uint32())), "lmrs_batch_mask_info: NULL argument"),
        (lambda: lib.lmrs_batch_mask_info(b._h, 0, None), "lmrs_batch_mask_info: NULL argument"),
        (lambda: lib.lmrs_batch_mask_info(b._h, 3, ctypes.byref(ctypes.c_uint32())), "lmrs_batch_mask_info: slot 3 of 3"),
    ]
    for fn, msg in cases:
        assert fn() != 0, msg
        assert lib.lmrs_last_error().decode().startswith(msg), (msg, lib.lmrs_last_error().decode())
        valid(f"after {msg!r}")
    # the top-k of a row cannot be longer than its allow-list: slot 1 allows 3 tokens
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_forward_runs: run 1: slot 1: k = 4 exceeds the 3 tokens its mask allows \(n_allowed\)"):
        b.forward_runs([(0, seqs[0].n, [5], 1), (1, seqs[1].n, [6, 7], 1)], k=4)
    valid("after k > n_allowed")
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_forward_runs_embed: run 0: slot 1: k = 4 exceeds the 3 tokens"):
        b.forward_runs([(1, seqs[1].n, token_rows(seqs[1].orc, [6]), 1)], k=4)
    valid("after k > n_allowed with an embedding run")
    # ... a masked run without outputs is no obstacle, and k = n_allowed is served
    pos = [seqs[0].n, seqs[1].n]
    am = b.forward_runs([(0, pos[0], [5], 1), (1, pos[1], [6, 7], 0)], k=4)[0]
    assert int(am[0]) == ref_argmax(seqs[0].feed([5])); seqs[1].feed([6, 7])
    valid("after a masked run without outputs")
    # the Python wrapper's own shape checks
    with pytest.raises(L.LmrsError, match="bool masks must be"):
        b.set_masks([0], np.ones((1, V - 1), np.bool_))
    with pytest.raises(L.LmrsError, match="packed masks must be"):
        b.set_masks([0], np.ones((1, W + 1), np.uint32))
    valid("last")
    b.close()


@gpu
def test_a_vocabulary_with_an_unwritten_tail_has_no_masks(L):
    """vocabulary 4098 (Q8_0): the classifier writes 4096 of the 4098 logits - a batch exists (4096 rows are a multiple of 16), the sampled calls refuse
    it and so does set_masks; the batch goes on unmasked"""
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-v4098", vocab_size=4098)
    img = S.build_image(cfg, S.Q8_0, seed=419)
    m, b, seqs = prefilled(L, img, cfg, [2, 0], 420)
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_set_masks: the classifier leaves the last vocab_size % 4 logits unwritten"):
        b.set_masks([0], np.ones((1, 4098), np.bool_))
    assert b.mask_info(0) is None
    am, lg = b.forward([0, 1], [5, 6], [2, 0], logits=True)
    for i, s in enumerate(seqs):
        check_row(lg[i], am[i], s.feed([5 + i]), None, f"slot {i} after the refusal")
    b.close()
