"""Positions 2104 .. 8191 on every attention path, run with `-m gpu` on an MI355X against the CPU oracle, bit for bit (parity_rules.assert_bit_equal: no
tolerance anywhere).  The library keeps 8192 positions per sequence; the split form's 32-chunk bucket covers half of them.  tests/deep_rules.py holds the
one-layer geometries, the reasoned position sets and the ONE oracle run per geometry that every test here shares; every context, slot and run replays that
run's tokens at their own positions.

What only takes effect at this depth: LDS sized from seq_len (two value tiles + 8192 weights), grids larger than the resident slots (32 heads x 32 chunks in
the qkv + scores launch), the lazily captured graph of each bucket, 64-bit offsets into the score scratch and the caches, Gemma-2's window arithmetic with
whole value and score chunks behind the window, and serial chains of up to 8192 adds that must keep the reference's order.

Oracle cost, one layer, sequential steps - each reference() prints its wall time.  As measured when this module was written, on 8 CPU threads / on the
16 threads beside an MI355X: mini-llama 8192 steps 32.5 s / 6.7 s, mini-gemma 8192 steps 46.2 s / 20.8 s, mini-llama3b 4416 steps 22.9 s / 5.5 s,
mini-phi 2320 steps 13.7 s / 2.6 s: 115 s / 36 s together, against 3 x the window recipe's 4100 two-layer Gemma steps (about as many layer passes as
mini-gemma's run here, so about 3 x 46 s / 3 x 21 s).  The whole module beside the GPU: 47 tests in 47 s, 36 s of it these four runs (charged to the
four tests that call reference() first); every test is below 0.15 s otherwise."""
import numpy as np
import pytest

import deep_rules as D
from deep_rules import reference
from parity_rules import assert_bit_equal, ref_argmax
from penalty_rules import params, penalised

pytestmark = pytest.mark.gpu

SWITCHES = ("LMRS_ATT_SPLIT_POS", "LMRS_ATT_SPLIT_MERGED", "LMRS_ATT_SPLIT_SCORE_WGS")
# the forms of a decode step: five launches a layer (scores in the qkv launch), six (what sharded and f32 contexts take), no split at any depth (the plain
# attention kernel over up to 8192 keys), and few score workgroups walking every (head, chunk) item
FORMS = {"default": {}, "six": {"LMRS_ATT_SPLIT_MERGED": 0}, "nosplit": {"LMRS_ATT_SPLIT_POS": 0},
         "wgs3": {"LMRS_ATT_SPLIT_SCORE_WGS": 3}, "wgs5": {"LMRS_ATT_SPLIT_SCORE_WGS": 5}}
STEP_CASES = [(n, f) for n in D.NAMES for f in ("default", "six", "nosplit")] + [(n, f) for n in ("mini-llama", "mini-gemma") for f in ("wgs3", "wgs5")]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def context(L, monkeypatch, ref, form="default"):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, str(v))
    m = L.Transformer(ref.img)
    assert m.args.seq_len == D.SEQ_LEN and m.args.n_layers == 1
    return m


def filled(L, monkeypatch, ref, form="default"):
    """a fresh context whose cache holds toks[:depth - 1], by one prefill_tokens call (the batched pass: block attention, 512 rows a chunk)"""
    m = context(L, monkeypatch, ref, form)
    n = ref.depth - 1
    assert m.tokens_path(n)
    assert m.prefill_tokens(ref.toks[:n], 0) == n
    return m


def check_rows(kv_row, ref, positions, what):
    for p in positions:
        assert_bit_equal(kv_row(0, 0, p), ref.K[p], f"{what}: key row at {p}")
        assert_bit_equal(kv_row(1, 0, p), ref.V[p], f"{what}: value row at {p}")


def check_step(m, ref, p, what):
    """forward(toks[p], p): the logits, and the K/V row the step wrote (the same values the row held: one layer)"""
    assert_bit_equal(m.forward(int(ref.toks[p]), p), ref.logits[p], f"{what}: logits at {p}")
    check_rows(m.kv_row, ref, [p], what)


def check_launches(m, form, p):
    nl, n = m.args.n_layers, m.step_info(p)[0]
    if p < 384:
        return
    if form == "six":
        assert n == 6 * nl + 1, f"position {p}: {n} launches, the six-launch split form has {6 * nl + 1}"
    elif form == "nosplit":
        if p < 1024:                                        # (the unsplit merged qkv + attention launch; from 1024 on the two separate kernels)
            assert n == 4 * nl + 1, f"position {p}: {n} launches, the split form is in use with LMRS_ATT_SPLIT_POS=0"
    else:
        assert n == 5 * nl + 1, f"position {p}: {n} launches, the merged qkv + scores launch is not in use"


# ---------------------------------------------------------------------------------------------- a. the cache at depth

@pytest.mark.parametrize("name", D.NAMES)
def test_the_cache_at_depth(L, monkeypatch, name):
    """prefill_tokens(toks[:depth - 1]) on a fresh context: K/V rows at about 20 positions over every bucket.  Every other test builds its cache this way;
    a failure here is a prefill fault, not an attention fault of a decode step."""
    ref = reference(name)
    m = filled(L, monkeypatch, ref)
    check_rows(m.kv_row, ref, D.cache_positions(name), f"{name}: prefill_tokens of {ref.depth - 1}")


# ---------------------------------------------------------------------------------------------- b. decode steps at depth

@pytest.mark.parametrize("name,form", STEP_CASES)
def test_decode_steps_at_depth(L, monkeypatch, name, form):
    """forward(toks[p], p) at the geometry's position set, in a shuffled fixed order: the bucket edges, the 32-chunk bucket's chunk edges and its end,
    interior positions, Gemma's window edges - in the five-launch, six-launch and unsplit forms, and with 3 and 5 score workgroups."""
    ref = reference(name)
    m = filled(L, monkeypatch, ref, form)
    ps = D.step_positions(name)
    order = [ps[i] for i in np.random.default_rng(7).permutation(len(ps))]
    for p in order:
        check_launches(m, form, p)
        check_step(m, ref, p, f"{name}, {form}")


# ---------------------------------------------------------------------------------------------- c. dense crossings

@pytest.mark.parametrize("name", D.NAMES)
def test_dense_crossings(L, monkeypatch, name):
    """Consecutive steps over the bucket edges and up to the clamp, on one context, in order: the graph of each bucket is captured inside the run and the
    new key moves into a fresh chunk.  Gemma: also across the positions where a whole value chunk and a whole score chunk fall behind the window."""
    ref = reference(name)
    m = filled(L, monkeypatch, ref)
    for r in sorted(D.dense_ranges(name), key=lambda r: r[0]):
        for p in r:
            check_launches(m, "default", p)
            check_step(m, ref, p, f"{name}, steps {r[0]} .. {r[-1]}")


# ---------------------------------------------------------------------------------------------- d. generate_greedy, and the clamp's refusals

@pytest.mark.parametrize("name", D.NAMES)
def test_generate_greedy_across_an_edge_and_up_to_the_end(L, monkeypatch, name):
    """generate_greedy of 12 steps across a bucket edge, and the run whose last written position is the geometry's last (8191 at the clamp), against the
    oracle's chain of forward + lmrs_ref_argmax.  The rows are put back by re-forwarding toks; then the refusals at 8192, and a deep step after them."""
    ref = reference(name)
    m = filled(L, monkeypatch, ref)
    toks = ref.toks
    for s in D.greedy_starts(name):
        out = m.generate_greedy([int(toks[s])], D.N_GREEDY, s)
        assert out.tolist() == ref.chains[s], f"{name}: greedy tokens from {s}"
        for p in range(s + 1, s + D.N_GREEDY):
            check_step(m, ref, p, f"{name}: restoring the rows behind the greedy run from {s}")
    deep = ref.depth - 1
    with pytest.raises(L.LmrsError, match="pos out of range"):
        m.forward(int(toks[0]), D.SEQ_LEN)
    with pytest.raises(L.LmrsError, match="exceeds seq_len"):
        m.prefill_tokens(toks[:10], D.SEQ_LEN - 2)
    with pytest.raises(L.LmrsError, match="exceeds seq_len"):
        m.generate_greedy([int(toks[0])], D.N_GREEDY + 1, D.SEQ_LEN - D.N_GREEDY)
    check_step(m, ref, deep, f"{name}: after the refusals")


# ---------------------------------------------------------------------------------------------- e. the separate kernels at depth

@pytest.mark.parametrize("name", D.NAMES)
def test_fill_kv_cache_at_depth(L, monkeypatch, name):
    """fill_kv_cache of ONE embedding row - the layers-only graph of the separate kernels: the plain attention kernel at any depth - at the last position and
    at a chunk edge, and of 40 rows near the end (block attention with the fill call's own window meaning on Gemma): the residual rows and the K/V rows
    against orc.fill_kv_cache.  The rows are another token run's, so a call that left the cache alone would not pass; toks' rows are put back."""
    ref = reference(name)
    m = filled(L, monkeypatch, ref)
    dim = m.args.dim
    emb = m.get_embeddings(ref.fill_toks).reshape(D.FILL_ROWS, dim)
    assert_bit_equal(emb, ref.fill_emb, f"{name}: embedding rows")
    for p in D.fill_one_positions(name):
        e = emb[0].copy()
        res, k, v = ref.fills["one", p]
        assert m.fill_kv_cache(e, p) == p + 1
        assert_bit_equal(e, res, f"{name}: residual row of a one-row fill_kv_cache at {p}")
        assert_bit_equal(m.kv_row(0, 0, p), k, f"{name}: key row of a one-row fill_kv_cache at {p}")
        assert_bit_equal(m.kv_row(1, 0, p), v, f"{name}: value row of a one-row fill_kv_cache at {p}")
        check_step(m, ref, p, f"{name}: restoring row {p}")
    p0 = D.fill_run_start(name)
    res, kv = ref.fills["run", p0]
    e = emb.copy().reshape(-1)
    assert m.fill_kv_cache(e, p0) == p0 + D.FILL_ROWS
    assert_bit_equal(e.reshape(D.FILL_ROWS, dim), res, f"{name}: residual rows of fill_kv_cache of {D.FILL_ROWS} rows at {p0}")
    for p, (k, v) in kv.items():
        assert_bit_equal(m.kv_row(0, 0, p), k, f"{name}: key row {p} of the {D.FILL_ROWS}-row fill_kv_cache")
        assert_bit_equal(m.kv_row(1, 0, p), v, f"{name}: value row {p} of the {D.FILL_ROWS}-row fill_kv_cache")
    assert m.prefill_tokens(ref.toks[p0:p0 + D.FILL_ROWS], p0) == p0 + D.FILL_ROWS
    check_rows(m.kv_row, ref, [p0, p0 + D.FILL_ROWS - 1], f"{name}: rows put back")
    check_step(m, ref, ref.depth - 1, f"{name}: after the rows were put back")


# ---------------------------------------------------------------------------------------------- f. batched rows at depth on the context

@pytest.mark.parametrize("name", D.NAMES)
def test_forward_tokens_at_depth(L, monkeypatch, name):
    """forward_tokens near the end: 192 rows of block attention over about 8k keys, and 20 rows whose in-block queries lie on both sides of Gemma's window
    (the 128- and 96-wide geometries: the last 64 positions of their depth).  The logits of every row."""
    ref = reference(name)
    m = filled(L, monkeypatch, ref)
    for s, n in D.tokens_runs(name):
        got = m.forward_tokens(ref.toks[s:s + n], s)
        want = D.rows(ref, range(s, s + n))
        for i in range(n):
            assert_bit_equal(got[i], want[i], f"{name}: forward_tokens of {n} rows at {s}: row {i} (position {s + i})")
        check_rows(m.kv_row, ref, [s, s + n // 2, s + n - 1], f"{name}: forward_tokens of {n} rows at {s}")


# ---------------------------------------------------------------------------------------------- g. batches at depth

def pages_of(n, page_len):
    return -(-n // page_len)


def make_batch(L, m, kind):
    if kind == "16":
        return L.Batch(m, 4)
    if kind == "wide":
        return L.Batch(m, 20, wide=True)
    # a pool just large enough: one slot to the clamp, the three shallow slots as far as they get (two steps, a run row, four greedy steps), and a spare
    # page for a copy
    n_pages = pages_of(D.SEQ_LEN, kind) + sum(pages_of(p + 3 + D.BATCH_GREEDY, kind) for p in D.BATCH_SHALLOW) + 1
    return L.Batch(m, 4, page_len=kind, n_pages=n_pages)


@pytest.mark.parametrize("kind", ["16", "wide", 64, 1024])
@pytest.mark.parametrize("name", ["mini-llama", "mini-gemma"])
def test_batches_at_depth(L, monkeypatch, name, kind):
    """Slot 0 at 8000 (a fork of the context's cache) beside slots at 3, 255 and 400: two forward calls in either row order, a ragged pass with a 7-row run
    on the deep slot, four greedy steps of the device loop, a prompt chunk at 8009 .. 8190 (block attention; over the page table on paged batches), the
    step at 8191 and the refusal at 8192 - on a 16-row batch, a wide one and pages of 64 and 1024 positions."""
    ref = reference(name)
    toks = ref.toks
    what = f"{name}, batch {kind}"
    m = filled(L, monkeypatch, ref)
    b = make_batch(L, m, kind)
    b.fork(L.BATCH_CTX, 0, D.BATCH_DEEP)
    for s, n in zip((1, 2, 3), D.BATCH_SHALLOW):
        assert b.prefill(s, toks[:n], 0) == n
    first, second, runs, greedy = D.batch_positions()
    slot_row = lambda s: (lambda w, l, p: b.kv_row(s, w, l, p))

    def step(order, pos):
        am, lg = b.forward(order, [int(toks[pos[s]]) for s in order], [pos[s] for s in order], logits=True)
        for r, s in enumerate(order):
            assert_bit_equal(lg[r], ref.logits[pos[s]], f"{what}: rows {order}: logits of slot {s} at {pos[s]}")
            assert int(am[r]) == ref_argmax(ref.logits[pos[s]]), f"{what}: rows {order}: argmax of slot {s} at {pos[s]}"
            check_rows(slot_row(s), ref, [pos[s]], f"{what}: slot {s}")

    step([0, 1, 2, 3], first)
    step([3, 2, 1, 0], second)
    rr = [(0, runs[0], toks[runs[0]:runs[0] + D.BATCH_RUN], D.BATCH_RUN)] + [(s, runs[s], [int(toks[runs[s]])], 1) for s in (1, 2, 3)]
    at = list(range(runs[0], runs[0] + D.BATCH_RUN)) + [runs[s] for s in (1, 2, 3)]
    am, lg = b.forward_runs(rr, logits=True)
    for i, p in enumerate(at):
        assert_bit_equal(lg[i], ref.logits[p], f"{what}: forward_runs output {i} (position {p})")
        assert int(am[i]) == ref_argmax(ref.logits[p]), f"{what}: forward_runs argmax {i} (position {p})"
    out = b.generate_greedy([0, 1, 2, 3], [int(toks[g]) for g in greedy], list(greedy), D.BATCH_GREEDY)
    for s, g in enumerate(greedy):
        assert out[s].tolist() == ref.chains[g], f"{what}: greedy tokens of slot {s} from {g}"
    # slot 0 stands at 8009 with three rows of its own tokens behind it: the prompt chunk puts toks' rows back and runs on to 8190
    p, last = greedy[0], D.SEQ_LEN - 1
    assert b.prefill_form(last - p, p) == (1, 1), f"{what}: {last - p} rows at {p} take block attention"
    assert b.prefill(0, toks[p:last], p) == last
    am, lg = b.forward([0], [int(toks[last])], [last], logits=True)
    assert_bit_equal(lg[0], ref.logits[last], f"{what}: logits at {last}")
    assert int(am[0]) == ref_argmax(ref.logits[last])
    with pytest.raises(L.LmrsError, match="exceeds seq_len"):
        b.forward([0], [int(toks[0])], [D.SEQ_LEN])
    with pytest.raises(L.LmrsError, match="exceeds seq_len"):
        b.forward([1, 0], [int(toks[0])] * 2, [10, D.SEQ_LEN])
    check_rows(slot_row(0), ref, D.BATCH_KV, f"{what}: slot 0")
    if kind not in ("16", "wide"):
        assert b.slot_pages(0) == (pages_of(D.SEQ_LEN, kind), 0), f"{what}: slot 0 holds every page of 8192 positions alone"
    b.close()


# ---------------------------------------------------------------------------------------------- h. penalties over a full record

def test_penalties_over_a_full_record(L, monkeypatch):
    """penalty_rows_kernel sorts cap = the next power of two >= pos + 1 keys in LDS: slot 0 at 8191 (cap 8192, every key live), slot 1 at 4097 (cap 8192,
    about half live), slot 2 at 4095 (cap 4096).  The records are draws from a 300-token alphabet (set_history), the caches forks of the context's; one pass
    of repetition, presence and frequency penalties, out_from deep in the record on one row, against penalty_rules.penalised over the oracle's logits."""
    ref = reference("mini-llama")
    toks, V = ref.toks, ref.cfg.vocab_size
    m = filled(L, monkeypatch, ref)
    b = L.Batch(m, 3)
    pars = [params("all"), params("freq", out_from=2048), params("all", out_from=0)]
    b.set_penalties([0, 1, 2], *([p[k] for p in pars] for k in ("repetition", "presence", "frequency", "out_from")))
    alpha = np.random.default_rng(572).choice(V, 300, replace=False).astype(np.uint32)
    hist = []
    for s, p in enumerate(D.PENALTY_AT):
        b.fork(L.BATCH_CTX, s, p)
        h = alpha[np.random.default_rng(573 + s).integers(0, alpha.size, p)]
        b.set_history(s, h, 0)
        hist.append(h.tolist() + [int(toks[p])])                # the step records its own token at p
    am, lg = b.forward([0, 1, 2], [int(toks[p]) for p in D.PENALTY_AT], list(D.PENALTY_AT), logits=True)
    for s, (p, par) in enumerate(zip(D.PENALTY_AT, pars)):
        pen = penalised(ref.logits[p], hist[s], p, par)
        assert (pen.view(np.uint32) != ref.logits[p].view(np.uint32)).sum() >= 200, "the penalty should touch most of the alphabet"
        assert_bit_equal(lg[s], pen, f"slot {s} at {p}: penalised logits")
        assert int(am[s]) == ref_argmax(pen), f"slot {s} at {p}: argmax"
        assert b.history(s, 1, p).tolist() == [int(toks[p])]
    b.close()


# ---------------------------------------------------------------------------------------------- teeth: on the oracle alone

def test_teeth_llama_deep_keys_are_read():
    """A test that found deep keys ignored would be vacuous otherwise: another token at key 0 moves the logits at 8191, at key 6000 those at 6144."""
    ref = reference("mini-llama")
    assert D.moved_by(ref, 0, 8191) > 0, "oracle: key 0 does not move the logits at 8191"
    assert D.moved_by(ref, 6000, 6144) > 0, "oracle: key 6000 does not move the logits at 6144"


def test_teeth_gemma_window_edges():
    """The window's first live key, exactly: at 8190 key 4094 is live, at 8191 it is not and 4095 is; at 4352 the whole first 256-key score chunk is
    behind the window - key 255 moves nothing, key 256 does."""
    ref = reference("mini-gemma")
    assert D.moved_by(ref, 4094, 8190) > 0, "oracle: key 4094 does not move the logits at 8190"
    assert D.moved_by(ref, 4094, 8191) == 0, "oracle: key 4094 moves the logits at 8191 - it lies behind the window"
    assert D.moved_by(ref, 4095, 8191) > 0, "oracle: key 4095 does not move the logits at 8191"
    assert D.moved_by(ref, 255, 4352) == 0, "oracle: key 255 moves the logits at 4352 - it lies behind the window"
    assert D.moved_by(ref, 256, 4352) > 0, "oracle: key 256 does not move the logits at 4352"
