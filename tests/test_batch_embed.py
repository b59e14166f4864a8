"""lmrs_batch_prefill_embeddings, lmrs_batch_forward_runs_embed, lmrs_batch_forward_runs_embed_sample (include/lmrs_hip.h): embedding rows - image
features - in a batch slot and in the ragged passes.  The reference is one CPU oracle PER SEQUENCE (tests/test_batch.py's Seq) fed the same rows through
Oracle.fill_kv_cache (transformer.rs:672-684) and the same tokens through its sequential forward; every comparison - residual rows, argmax, logits,
top-k, K/V rows, sampled tokens - is bit for bit (tests/parity_rules.py).  No tolerances."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax, run_positions
from test_batch import CFGS, Seq as TokenSeq, check_slot_rows, snapshot
from test_batch_runs import FORMS, STARTS, toks_for
from test_topk import rank_row
from tools import synth_lmrs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


class Seq(TokenSeq):
    """tests/test_batch.py's Seq with embedding rows: fill() is ONE fill_kv_cache call, fill_rows() one call per row (each at its own position)"""

    def fill(self, rows):
        e = np.ascontiguousarray(rows, np.float32).copy()
        assert self.orc.fill_kv_cache(e.reshape(-1), self.n) == self.n + e.shape[0]
        self.n += e.shape[0]
        return e                                               # the reference's mutated argument

    def fill_rows(self, rows):
        for r in np.ascontiguousarray(rows, np.float32):
            self.fill(r[None, :])


def random_rows(n, dim, seed):
    """n embedding rows: normal * 0.5, then (where there is room) one row all zero, one with magnitudes spread over 1e-3 .. 1e3, one holding a -0.0"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, dim)).astype(np.float32) * np.float32(0.5)
    if n >= 3:
        e[n // 3] = 0.0
    if n >= 2:
        e[n // 2] = (rng.choice([-1.0, 1.0], dim) * 10.0 ** rng.uniform(-3, 3, dim)).astype(np.float32)
    e[n - 1, dim // 2] = np.float32(-0.0)
    return np.ascontiguousarray(e)


def token_rows(orc, toks):
    """get_embeddings(toks) as Transformer::forward feeds them to the layers: Gemma-2 scales by sqrt(dim), one f32 multiply (transformer.rs:326-332)"""
    e = orc.get_embeddings(np.asarray(toks, np.uint32)).reshape(len(toks), orc.args.dim).copy()
    if orc.args.model_type == 0:
        e = e * np.float32(np.sqrt(np.float32(orc.args.dim)))
    return np.ascontiguousarray(e, np.float32)


def prefilled(L, img, cfg, lengths, seed, n_slots=None, wide=False):
    m = L.Transformer(img)
    b = L.Batch(m, n_slots or len(lengths), wide=wide)
    seqs = []
    for i, n in enumerate(lengths):
        s = Seq(img, i)
        if n:
            toks = S.prompt_tokens(cfg, n, seed + i)
            assert b.prefill(i, toks, 0) == n
            s.feed(toks)
        seqs.append(s)
    return m, b, seqs


def embed_pass(b, work, what, k=0, kv="all"):
    """One forward_runs over work = [(Seq, rows, n_out, how), ...] at each sequence's end, logits on.  how = "tokens": rows is a token list; "same": rows is
    a token list fed as the embedding rows Transformer::forward would build from it, the oracle is fed the tokens; "rows": rows is a float32 array the
    oracle takes through fill_kv_cache one row at a time (no outputs can be judged: n_out must be 0).  -> (argmax, logits, the oracle's logits of the
    output rows, top-k results or None)"""
    runs = []
    for s, rows, n_out, how in work:
        assert how in ("tokens", "same", "rows") and (how != "rows" or n_out == 0)
        runs.append((s.slot, s.n, list(rows) if how == "tokens" else (token_rows(s.orc, rows) if how == "same" else rows), n_out))
    got = b.forward_runs(runs, k=k, logits=True)
    am, lg = got[0], got[1]
    assert am.shape == (sum(w[2] for w in work),) and lg.shape[0] == am.size
    o, wants = 0, []
    for s, rows, n_out, how in work:
        start, n = s.n, len(rows)
        if how == "rows":
            s.fill_rows(rows)
        else:
            want = [s.feed([t]) for t in rows]
            for j in range(n - n_out, n):
                where = f"{what}: slot {s.slot} pos {start + j} (output row {o}, {how})"
                assert int(am[o]) == ref_argmax(want[j]), f"{where}: argmax"
                assert_bit_equal(lg[o], want[j], f"{where}: logits")
                wants.append(want[j]); o += 1
        check_slot_rows(b, s, range(start, start + n) if kv == "all" else run_positions(start, n), f"{what} ({how})")
    return am, lg, wants, (got[2:] if k else None)


def decode_pass(b, seqs, what):
    """one decode row on every sequence through the token call: pins what the earlier rows left through attention"""
    V = seqs[0].orc.args.vocab_size
    pos = [s.n for s in seqs]
    toks = [(31 * s.slot + 7) % V for s in seqs]
    am, lg = b.forward([s.slot for s in seqs], toks, pos, logits=True)
    for i, s in enumerate(seqs):
        want = s.feed([toks[i]])
        assert int(am[i]) == ref_argmax(want), f"{what}: slot {s.slot}: argmax"
        assert_bit_equal(lg[i], want, f"{what}: slot {s.slot} pos {pos[i]}: logits of the decode row")


# ---------------------------------------------------------------------------------------------- 1. prefill_embeddings against one fill_kv_cache

PREFILL = [("mini-llama", S.Q8_0, 70, 5), ("mini-llama", S.Q4_0, 70, 5), ("mini-phi", S.Q8_0, 63, 2), ("mini-gemma", S.Q8_0, 50, 3), ("mini-gemma", S.Q4_0, 17, 0)]
PREFILL += [("mini-llama3b", S.Q8_0, n, 4) for n in (1, 2, 15, 16, 17, 47, 48)]           # both sides of the skinny / direct / ring switches
PREFILL += [("mini-phi-long", S.Q8_0, 530, 3)]                                            # a 512-row chunk and an 18-row one


@gpu
@pytest.mark.parametrize("cfg,q,n,start", PREFILL)
def test_prefill_embeddings_is_one_fill_kv_cache(L, cfg, q, n, start):
    img = S.build_image(cfg, q, seed=401)
    m = L.Transformer(img); b = L.Batch(m, 3)
    s = Seq(img, 1)
    if start:
        toks = S.prompt_tokens(cfg, start, 402)
        b.prefill(1, toks, 0); s.feed(toks)
    rows = random_rows(n, m.args.dim, 403 + n)
    keep = rows.copy()
    end, res = b.prefill_embeddings(1, rows, start, residual=True)
    assert end == start + n
    assert_bit_equal(rows, keep, "the caller's rows are never written")
    want = s.fill(rows)
    what = f"{cfg} q{q} n {n} at {start}"
    assert_bit_equal(res, want, f"{what}: residual against the oracle's mutated embeddings")
    check_slot_rows(b, s, run_positions(start, n), what)
    for k in range(2):
        pos, tok = s.n, 11 + k
        am, lg = b.forward([1], [tok], [pos], logits=True)
        assert_bit_equal(lg[0], s.feed([tok]), f"{what}: forward step {k} on the slot")
    # the same rows into another slot without the download: the same K/V rows
    if start:
        b.prefill(2, toks, 0)
    assert b.prefill_embeddings(2, rows, start) == start + n
    for layer in range(m.args.n_layers):
        for p in run_positions(start, n):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(2, w, layer, p), s.orc.kv_row(w, layer, p), f"{what}: residual=False, {'kv'[w]} layer {layer} pos {p}")


# ---------------------------------------------------------------------------------------------- 2. mixed ragged pass, R = 16

@gpu
@pytest.mark.parametrize("cfg,q", CFGS)
def test_mixed_runs_of_tokens_and_embeddings(L, cfg, q):
    """tests/test_batch_runs.py's skinny pass (slots at 65, 0, 128, 61, 252; runs of 1, 4, 1, 7, 3) with the 4-row run random embedding rows without outputs
    and the 7-row run the embedding rows of its tokens with all 7 outputs"""
    img = S.build_image(cfg, q, seed=411)
    m, b, seqs = prefilled(L, img, cfg, [65, 0, 128, 61, 252], 412)
    dim = m.args.dim
    same = toks_for(cfg, 7, 423)
    work = [(seqs[0], toks_for(cfg, 1, 420), 1, "tokens"), (seqs[1], random_rows(4, dim, 421), 0, "rows"), (seqs[2], toks_for(cfg, 1, 422), 1, "tokens"),
            (seqs[3], same, 7, "same"), (seqs[4], toks_for(cfg, 3, 424), 3, "tokens")]
    am, lg, wants, (ti, tl) = embed_pass(b, work, f"{cfg} q{q}", k=5)
    assert [s.n for s in seqs] == [66, 4, 129, 68, 255] and ti.shape == (12, 5)
    own = L.Transformer(img)                                 # the token-equal run's top-k: the same sequence on a context of its own
    _, _, _, ti1, tl1, _ = own.score_topk(list(S.prompt_tokens(cfg, 61, 412 + 3)) + same, 5, 0)
    for j in range(7):
        o = 2 + j                                              # outputs: run 0's one row, run 2's one row, then the 7
        assert ti[o].tolist() == rank_row(wants[o])[:5].tolist() and ti[o].tolist() == ti1[61 + j].tolist(), f"{cfg} q{q}: top-5 indices of row {j}"
        assert_bit_equal(tl[o], tl1[61 + j], f"{cfg} q{q}: top-5 log-probabilities of row {j}")
    decode_pass(b, seqs[:4], f"{cfg} q{q}: decode rows behind the mixed pass")


# ---------------------------------------------------------------------------------------------- 3. every GEMM form

@gpu
@pytest.mark.parametrize("R", [17, 47, 48, 65, 130])
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_every_gemm_form(L, cfg, q, R):
    lens = FORMS[R]
    img = S.build_image(cfg, q, seed=431)
    m, b, seqs = prefilled(L, img, cfg, STARTS[:len(lens)], 432)
    n_out = [(n, 0, 1, n, 1)[i] for i, n in enumerate(lens)]
    work = []
    for i, (s, n, no) in enumerate(zip(seqs, lens, n_out)):
        if i % 2 == 0:
            work.append((s, toks_for(cfg, n, 440 + R + i), no, "tokens"))
        elif no:
            work.append((s, toks_for(cfg, n, 440 + R + i), no, "same"))
        else:
            work.append((s, random_rows(n, m.args.dim, 440 + R + i), 0, "rows"))
    embed_pass(b, work, f"{cfg} q{q} R {R}", kv="ends")
    decode_pass(b, seqs, f"{cfg} q{q} R {R}: decode rows behind it")


@gpu
def test_forty_single_rows_on_a_wide_batch(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=433)
    m, b, seqs = prefilled(L, img, cfg, [i % 5 for i in range(40)], 434, wide=True)
    work = []
    for i, s in enumerate(seqs):
        if i % 2 == 0:
            work.append((s, [(17 * i + 3) % 4096], 1, "tokens"))
        elif i % 4 == 1:
            work.append((s, [(19 * i + 1) % 4096], 1, "same"))
        else:
            work.append((s, random_rows(1, m.args.dim, 450 + i), 0, "rows"))
    embed_pass(b, work, "40 single rows")
    decode_pass(b, seqs, "40 single rows: the step behind them")


# ---------------------------------------------------------------------------------------------- 4. run_kind all zero is the token twin

def raw_runs(runs):
    s, p, n, x = (np.array([r[i] if i != 2 else len(r[2]) for r in runs], np.uint32) for i in (0, 1, 2, 3))
    t = np.array([t for r in runs for t in r[2]], np.uint32)
    return s, p, n, x, t


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_all_token_runs_equal_the_token_call(L, cfg, q):
    img = S.build_image(cfg, q, seed=441)
    m = L.Transformer(img)
    b1, b2 = L.Batch(m, 4), L.Batch(m, 4)
    lib, V = L.lib(), m.args.vocab_size
    for b in (b1, b2):
        b.prefill(0, S.prompt_tokens(cfg, 65, 442), 0); b.prefill(2, S.prompt_tokens(cfg, 9, 443), 0)
    runs = [(0, 65, toks_for(cfg, 3, 444), 3), (1, 0, toks_for(cfg, 20, 445), 0), (2, 9, toks_for(cfg, 1, 446), 1), (3, 0, toks_for(cfg, 6, 447), 2)]
    am1, lg1, ti1, tl1 = b1.forward_runs(runs, k=5, logits=True)
    s, p, n, no, t = raw_runs(runs)
    kind = np.zeros(4, np.uint32)
    am2, lg2, ti2, tl2 = np.zeros(6, np.uint32), np.zeros((6, V), np.float32), np.zeros((6, 5), np.uint32), np.zeros((6, 5), np.float32)
    rc = lib.lmrs_batch_forward_runs_embed(b2._h, 4, s.ctypes.data, p.ctypes.data, n.ctypes.data, no.ctypes.data, kind.ctypes.data, t.ctypes.data, None,
                                           am2.ctypes.data, lg2.ctypes.data, 5, ti2.ctypes.data, tl2.ctypes.data)
    assert rc == 0, lib.lmrs_last_error().decode()
    assert am1.tolist() == am2.tolist() and ti1.tolist() == ti2.tolist()
    assert_bit_equal(lg1, lg2, "logits"); assert_bit_equal(tl1, tl2, "top-k log-probabilities")
    for slot, start, toks, _ in runs:
        for layer in range(m.args.n_layers):
            for pos in range(start, start + len(toks)):
                for w in (0, 1):
                    assert_bit_equal(b1.kv_row(slot, w, layer, pos), b2.kv_row(slot, w, layer, pos), f"slot {slot} {'kv'[w]} layer {layer} pos {pos}")
    # the sampled twin: one argmax, one sample_mult and one top-p sampler, twin samplers on either side, two calls (the top-p vector is carried over)
    kinds = [(0.0, 0.9), (0.8, 1.0), (0.7, 0.9)]
    sa = [L.Sampler(V, *kd, 4400 + i) for i, kd in enumerate(kinds)]
    sb = [L.Sampler(V, *kd, 4400 + i) for i, kd in enumerate(kinds)]
    at = {0: 68, 1: 20, 2: 10}
    for step in range(2):
        sruns = [(i, at[i], toks_for(cfg, 2 + i, 448 + 3 * step + i)) for i in range(3)]
        want = b1.forward_runs_sample([r + (sa[i],) for i, r in enumerate(sruns)])
        s, p, n, _, t = raw_runs([r + (0,) for r in sruns])
        hs = (ctypes.c_void_p * 3)(*[x._h for x in sb])
        nxt = np.zeros(3, np.uint32)
        rc = lib.lmrs_batch_forward_runs_embed_sample(b2._h, 3, s.ctypes.data, p.ctypes.data, n.ctypes.data, kind.ctypes.data, t.ctypes.data, None,
                                                      ctypes.cast(hs, ctypes.c_void_p), nxt.ctypes.data)
        assert rc == 0, lib.lmrs_last_error().decode()
        assert nxt.tolist() == want.tolist(), f"sampled step {step}"
        for i in range(3):
            at[i] += 2 + i


# ---------------------------------------------------------------------------------------------- 5. sampled

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_sampled_embedding_runs(L, cfg, q):
    """the rule of tests/test_batch_runs_sample.py: the oracle's Sampler::sample on the oracle's logits, a persistent sampler per sequence on either side"""
    from test_batch_sample import Seq as SampledSeq
    img = S.build_image(cfg, q, seed=451)
    m = L.Transformer(img); b = L.Batch(m, 3)
    kinds = [(0.7, 0.9), (0.0, 0.9), (0.8, 1.0)]
    seqs = [SampledSeq(L, img, i, kinds[i], 4500 + i) for i in range(3)]
    for s, n in zip(seqs, (5, 0, 66)):
        if n:
            toks = S.prompt_tokens(cfg, n, 452 + s.slot); b.prefill(s.slot, toks, 0); s.feed(toks)
    for step in range(2):
        same = toks_for(cfg, 6, 453 + step)
        rows = random_rows(5, m.args.dim, 455 + step)
        dec = toks_for(cfg, 1, 457 + step)
        s0, s1, s2 = seqs
        got = b.forward_runs_sample([(0, s0.n, token_rows(s0.orc, same), s0.dev), (1, s1.n, rows, None), (2, s2.n, dec, s2.dev)])
        p1 = s1.n
        for r in rows:
            e = np.ascontiguousarray(r[None, :]).copy()
            s1.orc.fill_kv_cache(e.reshape(-1), s1.n); s1.n += 1
        want = [s0.ref.sample(s0.feed(same)), 0, s2.ref.sample(s2.feed(dec))]
        assert got.tolist() == want, f"{cfg} q{q} step {step}: {got.tolist()} vs {want}"
        for s, rng in ((s0, range(s0.n - 6, s0.n)), (s1, range(p1, s1.n)), (s2, [s2.n - 1])):
            for layer in range(m.args.n_layers):
                for p in rng:
                    for w in (0, 1):
                        assert_bit_equal(b.kv_row(s.slot, w, layer, p), s.orc.kv_row(w, layer, p), f"{cfg} q{q} step {step}: slot {s.slot} {'kv'[w]} layer {layer} pos {p}")


# ---------------------------------------------------------------------------------------------- 6. the two window rules

@gpu
def test_the_two_window_rules():
    """mini-gemma with 4352 positions (tests/test_batch.py's recipe), ONE oracle and ONE slot at 4100.  Three random rows at 4100: (a) as an embedding run
    of the ragged call every row tests the 4096-key window against its OWN position - the oracle's fill_kv_cache row by row; (b) through
    prefill_embeddings every row tests it against 4100 - ONE fill_kv_cache(n = 3).  Rows 4101 and 4102 mask different keys in layer 0 under the two
    rules, which their last-layer K/V rows show; (b) rewrites the rows of (a), as stale draft rows are rewritten."""
    import lmrs_amd as L
    cfg = dataclasses.replace(S.CONFIGS["mini-gemma"], name="mini-gemma-window", max_pos=4352)
    img = S.build_image(cfg, S.Q8_0, 29)
    m, b, seqs = prefilled(L, img, cfg, [4100], 29)
    s = seqs[0]
    last = m.args.n_layers - 1
    rows = random_rows(3, m.args.dim, 461)
    assert b.forward_runs([(0, 4100, rows, 0)]).size == 0
    s.fill_rows(rows)
    a = {}
    for p in (4101, 4102):
        for w in (0, 1):
            a[p, w] = b.kv_row(0, w, last, p).copy()
            assert_bit_equal(a[p, w], s.orc.kv_row(w, last, p), f"(a) the window per row: {'kv'[w]} row of the last layer at {p}")
    s.n = 4100
    assert b.prefill_embeddings(0, rows, 4100) == 4103
    s.fill(rows)
    differ = False
    for p in (4101, 4102):
        for w in (0, 1):
            got = b.kv_row(0, w, last, p)
            assert_bit_equal(got, s.orc.kv_row(w, last, p), f"(b) the window on the first position: {'kv'[w]} row of the last layer at {p}")
            differ = differ or (got.view(np.uint32) != a[p, w].view(np.uint32)).any()
    assert differ, "the two rules gave the same rows: the test shows nothing"


# ---------------------------------------------------------------------------------------------- 7. isolation

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q8_0)])
def test_isolation_and_interleaving(L, cfg, q):
    img = S.build_image(cfg, q, seed=471)
    m, b, seqs = prefilled(L, img, cfg, [12, 0, 66, 30], 472)
    own = Seq(img, None)                                       # the context's own sequence: an oracle that never sees the batch
    nl, dim = own.orc.args.n_layers, m.args.dim
    idle = seqs[3]

    def check_own(what):
        for layer in range(nl):
            for p in range(own.n):
                for w in (0, 1):
                    assert_bit_equal(m.kv_row(w, layer, p), own.orc.kv_row(w, layer, p), f"{what}: the context's {'kv'[w]} row layer {layer} pos {p}")

    assert_bit_equal(m.forward(5, 0), own.feed([5]), "forward before any embedding call")
    before = snapshot(b, idle.slot, range(idle.n + 8), nl)
    rows = random_rows(20, dim, 473)
    assert b.prefill_embeddings(1, rows, 0) == 20
    seqs[1].fill(rows)
    assert_bit_equal(m.forward(6, 1), own.feed([6]), "forward between embedding calls")
    check_own("after prefill_embeddings")
    embed_pass(b, [(seqs[0], toks_for(cfg, 2, 474), 1, "tokens"), (seqs[1], random_rows(9, dim, 475), 0, "rows"), (seqs[2], toks_for(cfg, 3, 476), 3, "same")], "pass 0")
    prompt = S.prompt_tokens(cfg, 10, 477)
    got = m.generate_greedy(prompt, 6, own.n)
    assert got.tolist() == own.orc.generate_greedy(prompt, 6, own.n).tolist(), "generate_greedy between embedding calls"
    own.n += 10 + 5
    assert b.prefill_embeddings(0, random_rows(1, dim, 478), seqs[0].n) == seqs[0].n + 1
    seqs[0].fill(random_rows(1, dim, 478))
    embed_pass(b, [(seqs[1], toks_for(cfg, 1, 479), 1, "same"), (seqs[2], random_rows(2, dim, 480), 0, "rows")], "pass 1")
    for x, y in zip(before, snapshot(b, idle.slot, range(idle.n + 8), nl)):
        assert_bit_equal(x, y, "a slot that no call names keeps its rows")
    check_own("after everything")
    assert_bit_equal(m.forward(3, own.n), own.feed([3]), "forward after everything")
    decode_pass(b, seqs, "decode rows after everything")


# ---------------------------------------------------------------------------------------------- 8. refusals

@gpu
def test_refusals_come_before_device_work(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=481)
    m, b, seqs = prefilled(L, img, cfg, [6, 0, 0], 482)
    T, dim = m.args.seq_len, m.args.dim
    lib = L.lib()
    n_good = [0]

    def good():
        k = n_good[0]
        embed_pass(b, [(seqs[0], [50 + k % 7], 1, "tokens"), (seqs[1], [60, 61], 2, "same") if k % 2 else (seqs[1], random_rows(2, dim, 483 + k), 0, "rows")],
                   f"the valid call after refusal {k}")
        n_good[0] += 1

    e2 = random_rows(2, dim, 484)
    name = "lmrs_batch_forward_runs_embed: "
    cases = [
        ([(0, 6, [1], 1), (1, T - 1, e2, 0)], name + "run 1: start_pos \\+ run_len exceeds seq_len"),
        ([(0, 6, [1, 2], 1), (1, 0, random_rows(300, dim, 485), 0), (2, 0, random_rows(211, dim, 486), 0)], name + "the runs hold more than 512 rows"),
        ([(0, 6, [1], 1), (0, 7, e2, 0)], name + "slot 0 appears in more than one run"),
    ]
    for runs, msg in cases:
        with pytest.raises(L.LmrsError, match=msg):
            b.forward_runs(runs)
        good()
    with pytest.raises(L.LmrsError, match="lmrs_batch_forward_runs_embed_sample: slot 0 appears in more than one run"):
        b.forward_runs_sample([(0, 6, [1], None), (0, 7, e2, None)])
    good()
    u = lambda *v: np.array(v, np.uint32)
    slot, start, ln, no = u(0, 1), u(seqs[0].n, seqs[1].n), u(1, 2), u(1, 0)
    tok, am, nxt = u(1), u(0, 0, 0), u(0, 0)
    P = lambda a: a.ctypes.data

    def call(kind, tokens=P(tok), emb=P(e2), bh=None):
        return lib.lmrs_batch_forward_runs_embed(b._h if bh is None else bh, 2, P(slot), P(start), P(ln), P(no), P(kind), tokens, emb, P(am), None, 0, None, None)

    hs = (ctypes.c_void_p * 2)(None, None)

    def call_s(kind, tokens=P(tok), emb=P(e2), bh=None):
        return lib.lmrs_batch_forward_runs_embed_sample(b._h if bh is None else bh, 2, P(slot), P(start), P(ln), P(kind), tokens, emb, ctypes.cast(hs, ctypes.c_void_p), P(nxt))

    for fn, nm in ((call, "lmrs_batch_forward_runs_embed: "), (call_s, "lmrs_batch_forward_runs_embed_sample: ")):
        for kw, msg in (({"kind": u(0, 2)}, "run 1: run_kind = 2"), ({"kind": u(0, 1), "emb": None}, "embeddings is NULL with an embedding run present"),
                        ({"kind": u(0, 1), "tokens": None}, "tokens is NULL with a token run present"), ({"kind": u(0, 1), "bh": ctypes.c_void_p()}, "NULL argument")):
            kind = kw["kind"]                                  # (kept alive over the call)
            assert fn(**kw) != 0
            err = lib.lmrs_last_error().decode()
            assert err.startswith(nm) and msg in err, (kw, err)
            good()
    for args, msg in (((0, np.empty((0, dim), np.float32), 0), "n == 0"), ((3, e2, 0), "slot 3 of 3"), ((0, e2, T - 1), "exceeds seq_len")):
        with pytest.raises(L.LmrsError, match="lmrs_batch_prefill_embeddings: .*" + msg):
            b.prefill_embeddings(*args)
        good()
    assert b.prefill_embeddings(2, e2, T - 2) == T            # ... and the last position is allowed
    assert lib.lmrs_batch_prefill_embeddings(None, 0, P(e2), 2, 0, None) != 0
    err = lib.lmrs_last_error().decode()
    assert err.startswith("lmrs_batch_prefill_embeddings: ") and "NULL" in err
    assert lib.lmrs_batch_prefill_embeddings(b._h, 0, None, 2, 0, None) != 0 and "NULL" in lib.lmrs_last_error().decode()
    good()
    # non-finite rows are not an error (the reference does not check them): the call runs, and the other slots' next call is the oracle's
    bad = random_rows(2, dim, 487); bad[0, 3] = np.inf; bad[1, 5] = np.nan
    assert b.prefill_embeddings(2, bad, 0) == 2
    good()


# ---------------------------------------------------------------------------------------------- 9. end to end, 10. the example program

def multimodal_file(text_cfg, vis_layers, seed, q=S.Q8_0):
    """a text model, a CLIP tower of vis_layers layers and a projector in one file, as the exporter lays them out (the recipe of tests/test_gpu_parity.py)"""
    from tools import synth_vision as V
    text = S.build_image(text_cfg, q, seed=seed, multimodal=1)
    vcfg = V.VisionCfg(n_layers=vis_layers)
    return np.concatenate([text, V.build_vision_section(vcfg, seed=seed + 1, q_type=q), V.build_processor_section(seed=seed + 2, q_type=q)]), vcfg


NUM_CROPS, W_CROP, H_CROP = 2, 1, 1                            # one 336 x 336 crop and the global view: 4 + 313 + 3 = 320 embeddings


def two_images(L, data, vcfg, cfg):
    """per image of two (different pixel_values seeds): (Seq after ONE fill_kv_cache(320), pixel values, the 320 embedding rows - prefix | the
    library's image features, checked against the oracle's | suffix -, 5 text tokens, the oracle's 9 greedy tokens behind them)"""
    from tools import synth_vision as V
    m = L.Transformer(data)
    off = m.bytes_consumed
    vis = L.VisionTransformer(data[off:]); proc = L.PHI3VProcessor(data[off + vis.bytes_consumed:])
    vis_o = O.VisionOracle(data[off:]); proc_o = O.ProcessorOracle(data[off + vis_o.bytes_consumed:])
    V_ = m.args.vocab_size
    bos_image = [1, 32010 % V_, 29871 % V_, 13]; bos_text = [1, 29871 % V_, 13]          # chat.rs:110-112 (ids folded into a mini vocabulary)
    seqs = []
    for i, seed in enumerate((33, 57)):
        pv = V.pixel_values(vcfg, NUM_CROPS, seed=seed)
        s = Seq(data, i)
        feats = proc.forward(vis.forward(pv, NUM_CROPS), 576 * 1024, 336 // 14 // 2, W_CROP, H_CROP)
        feats_o = proc_o.forward(vis_o.forward(pv, NUM_CROPS), 576 * 1024, 336 // 14 // 2, W_CROP, H_CROP)
        assert_bit_equal(np.asarray(feats).reshape(-1), np.asarray(feats_o).reshape(-1), f"image {i}: features")
        emb = np.concatenate([s.orc.get_embeddings(bos_image), np.asarray(feats, np.float32).reshape(-1), s.orc.get_embeddings(bos_text)])
        emb = np.ascontiguousarray(emb, np.float32).reshape(-1, m.args.dim)
        assert emb.shape[0] == 320
        s.fill(emb)
        text = toks_for(cfg, 5, 60 + i)
        seqs.append((s, pv, emb, text, s.orc.generate_greedy(text, 9, 320).tolist()))
    return m, seqs


@gpu
def test_two_images_end_to_end(L):
    data, vcfg = multimodal_file("mini-phi-long", 3, 31, S.Q8_0)
    m, seqs = two_images(L, data, vcfg, "mini-phi-long")
    b = L.Batch(m, 2)
    for s, pv, emb, text, want in seqs:
        assert b.prefill_embeddings(s.slot, emb, 0) == 320
        check_slot_rows(b, s, [3, 160, 319], f"image {s.slot}: rows of the image span")
    first = b.forward_runs([(s.slot, 320, text, 1) for s, _, _, text, _ in seqs])
    rest = b.generate_greedy([0, 1], first, [325, 325], 8)
    for i, (s, _, _, _, want) in enumerate(seqs):
        assert [int(first[i])] + rest[i].tolist() == want, f"image {i}: greedy ids"
    assert seqs[0][4] != seqs[1][4], "the two images give the same ids: the test shows nothing"


@gpu
def test_batch_image_program_prints_what_image_prefill_prints(L, tmp_path):
    """hostcpp/batch_image.cpp and hostcpp/image_prefill.cpp built with g++ against the library and run.  Both feed the reference's literal prefix /
    suffix ids (chat.rs:110-112), which mini-phi-long's vocabulary of 4096 does not hold: the file here is mini-phi-long's geometry with the real
    vocabulary size (the recipe of tests/test_gpu_parity.py's image_prefill test, with 1024 positions)."""
    cfg = dataclasses.replace(S.CONFIGS["mini-phi-long"], name="mini-phi-long-v32064", vocab_size=32064)
    data, vcfg = multimodal_file(cfg, 3, 31, S.Q8_0)
    m, seqs = two_images(L, data, vcfg, cfg)
    del m
    data.tofile(tmp_path / "model.lmrs")
    exe = {}
    for prog in ("image_prefill", "batch_image"):
        exe[prog] = str(tmp_path / prog)
        subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "lm.rs_amd", "hostcpp", prog + ".cpp"), "-I", os.path.join(ROOT, "include"),
                        "-L", os.path.join(ROOT, "lm.rs_amd"), "-llmrs_hip", f"-Wl,-rpath,{os.path.join(ROOT, 'lm.rs_amd')}", "-o", exe[prog]], check=True)
    alone, args = [], []
    for s, pv, emb, text, want in seqs:
        f = tmp_path / f"patches{s.slot}.f32"
        np.ascontiguousarray(pv, np.float32).tofile(f)
        geo = [str(f), str(NUM_CROPS), str(W_CROP), str(H_CROP)]
        r = subprocess.run([exe["image_prefill"], str(tmp_path / "model.lmrs")] + geo + ["9"] + [str(t) for t in text], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        ids = r.stdout.strip().split("\n")[-1].split()
        assert [int(t) for t in ids] == want, f"image_prefill on image {s.slot} alone"
        alone.append(ids)
        args += geo + [",".join(str(t) for t in text)]
    r = subprocess.run([exe["batch_image"], str(tmp_path / "model.lmrs"), "9"] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [l.split() for l in r.stdout.strip().split("\n")] == alone
