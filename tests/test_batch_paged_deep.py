"""Paged K/V (lmrs_batch_create_paged, lm.rs_amd/csrc/lmrs_paged.inc) where tests/test_batch_paged.py does not reach: rows beyond 256 keys - the second
and later score passes of paged_attn_kernel, more than four 64-row V chunks -, pages of 256, 512 and 1024 positions, prefills of more than one 512-row
chunk, Gemma-2's 4096-key window on pages, and pages that lie above 2^32 bytes, 2^31 floats and 2^32 floats of a pool.  The wide batch runs beside the
paged forms wherever the reference is shared, which takes attention_table_kernel / attention_runs_kernel beyond 256 keys for head sizes 128 and 256 too.
Every comparison is bit for bit, against the CPU oracle or - group E - against a wide batch that the oracle already pins.  No tolerances.

One oracle run per model (reference(), as tests/test_gpu_split_merged.py does it) serves groups A, B and D."""
import collections
import dataclasses
import functools

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from test_batch import Seq, check_slot_rows, snapshot, step
from test_batch_embed import Seq as EmbedSeq, random_rows, run_positions
from tools import synth_lmrs as S

pytestmark = pytest.mark.gpu

N = 1024
SEED = 701
LONG = {name + "-1k": dataclasses.replace(S.CONFIGS[name], name=name + "-1k", max_pos=N) for name in ("mini-llama", "mini-llama3b", "mini-gemma")}
# head sizes 64, 128, Gemma's 256, Phi's 96; and a Q4_0 file
CFGS = [("mini-llama-1k", S.Q8_0), ("mini-llama3b-1k", S.Q8_0), ("mini-gemma-1k", S.Q8_0), ("mini-phi-long", S.Q8_0), ("mini-llama-1k", S.Q4_0)]
FORMS = ["wide", 64, 256, 1024]
# T = pos + 1 crosses a 256-key score pass at 256, 512 and 768 (at 256 one lane of the new pass is live, 255 are clamped); 319 / 320 is a 64-row V chunk
# edge behind the first pass; the edges of 256- and 512-position pages are among them; three steps from 1021 end at the last position
D = [0, 3, 255, 256, 257, 319, 320, 511, 512, 513, 767, 768, 769, 1000, 1019, 1021]
STEPS = 3
STARTS = [250, 505, 760, 1010]                              # the greedy branches' first positions
N_NEW = 12

Ref = collections.namedtuple("Ref", "cfg img toks logits K V branch")


def config(name):
    return LONG.get(name) or S.CONFIGS[name]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


@functools.lru_cache(maxsize=None)
def reference(cfg, q):
    """The oracle over positions 0 .. 1023 of one seeded token run: the image, the tokens, logits [N, vocab], K and V rows [layers, N, kv_dim], read-only;
    and, recorded on the same oracle object after that capture, the greedy branches the device loop is judged by: from each d of STARTS - taken in
    DESCENDING order - toks[d] fed at d, then the argmax (ref_argmax) at d + 1, and so on for 12 steps.  A branch overwrites only oracle rows above its own
    d and the starts lie more than 12 apart, so a shallower branch never reads a row that a deeper one rewrote: each branch is what a fresh oracle fed
    toks[:d + 1] would continue with."""
    c = config(cfg)
    img = S.build_image(c, q, seed=SEED)
    toks = S.prompt_tokens(c, N, SEED)
    orc = O.Oracle(img)
    logits = np.stack([orc.forward(int(toks[p]), p).copy() for p in range(N)])
    kv = [np.stack([np.stack([orc.kv_row(w, l, p) for p in range(N)]) for l in range(c.n_layers)]) for w in (0, 1)]
    branch = {}
    for d in sorted(STARTS, reverse=True):
        t, out = int(toks[d]), []
        for k in range(N_NEW):
            t = ref_argmax(orc.forward(t, d + k)); out.append(t)
        branch[d] = out
    for a in (toks, logits, kv[0], kv[1]):
        a.setflags(write=False)
    return Ref(c, img, toks, logits, kv[0], kv[1], branch)


def pages_of(n, page_len):
    return -(-n // page_len)


def make_batch(L, m, form, n_slots, n_pages=None):
    """a wide batch, or a paged one of page_len = form whose pool could hold every slot at full depth"""
    if form == "wide":
        return L.Batch(m, n_slots, wide=True)
    return L.Batch(m, n_slots, page_len=form, n_pages=n_pages or n_slots * pages_of(m.args.seq_len, form))


def zero_row(m):
    return np.zeros(m.args.n_kv_heads * m.args.head_size, np.float32)


def check_ref_rows(b, ref, slot, positions, what):
    """K and V rows of every layer of `slot` at `positions`, against the shared reference"""
    for layer in range(ref.K.shape[0]):
        for p in positions:
            assert_bit_equal(b.kv_row(slot, 0, layer, p), ref.K[layer, p], f"{what}: slot {slot} k layer {layer} pos {p}")
            assert_bit_equal(b.kv_row(slot, 1, layer, p), ref.V[layer, p], f"{what}: slot {slot} v layer {layer} pos {p}")


def ref_steps(b, ref, slots, depths, what):
    """STEPS passes over `slots` (one call each), row i feeding toks[depths[i] + k] at depths[i] + k; a row stops once that would pass the last position.
    Logits, argmax and the written K/V row against the reference."""
    for k in range(STEPS):
        live = [(s, d + k) for s, d in zip(slots, depths) if d + k < N]
        am, lg = b.forward([s for s, _ in live], [int(ref.toks[p]) for _, p in live], [p for _, p in live], logits=True)
        for i, (s, p) in enumerate(live):
            assert_bit_equal(lg[i], ref.logits[p], f"{what} step {k}: row {i} (slot {s}, pos {p}): logits")
            assert int(am[i]) == ref_argmax(ref.logits[p]), f"{what} step {k}: row {i} (slot {s}, pos {p}): argmax"
            check_ref_rows(b, ref, s, [p], f"{what} step {k}")


# ---------------------------------------------------------------------------------------------- A. rows at every pass edge, per form

def prefilled(L, ref, form, n_slots):
    """slot i holds toks[:D[i]], one prefill call each (two chunks on a paged batch above 512)"""
    m = L.Transformer(ref.img)
    b = make_batch(L, m, form, n_slots)
    for i, d in enumerate(D):
        if d:
            assert b.prefill(i, ref.toks[:d], 0) == d
    return m, b


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cfg,q", CFGS)
def test_prefilled_rows_at_every_pass_edge(L, cfg, q, form):
    ref = reference(cfg, q)
    what = f"{cfg} q{q} {form}"
    m, b = prefilled(L, ref, form, 16)
    if form != "wide":
        for i, d in enumerate(D):
            assert b.slot_pages(i) == (pages_of(d, form), 0), f"{what}: slot {i} after a prefill of {d}"
        n_pages = b.pages()[1]
        assert b.pages() == (form, n_pages, n_pages - sum(pages_of(d, form) for d in D))
    for i, d in enumerate(D):
        at = {0, d // 2, d - 1} | ({511, 512} if d > 512 else set()) if d else set()
        check_ref_rows(b, ref, i, sorted(at), f"{what}: prefill of {d}")
    ref_steps(b, ref, list(range(16)), D, f"{what}: the 16-row table")
    if form != "wide":
        assert b.pages()[2] == n_pages - sum(pages_of(min(d + STEPS, N), form) for d in D)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cfg,q", CFGS)
def test_prefilled_rows_in_a_20_row_pass(L, cfg, q, form):
    """the same rows through the long table: four more slots are forks of the slots at 257, 513, 769 and 1000"""
    ref = reference(cfg, q)
    what = f"{cfg} q{q} {form}"
    m, b = prefilled(L, ref, form, 20)
    extra = [257, 513, 769, 1000]
    for j, d in enumerate(extra):
        b.fork(D.index(d), 16 + j, d)
        if form != "wide":
            for s in (D.index(d), 16 + j):
                assert b.slot_pages(s) == (pages_of(d, form), d // form), f"{what}: slot {s} after the fork at {d}"
    ref_steps(b, ref, list(range(20)), D + extra, f"{what}: the long table")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cfg,q", CFGS)
def test_forked_rows_at_every_pass_edge(L, cfg, q, form):
    """one slot holds toks[:1021]; the other 15 are forks of it at the depths of D (depth 0: an empty slot)"""
    ref = reference(cfg, q)
    what = f"{cfg} q{q} {form}"
    m = L.Transformer(ref.img)
    b = make_batch(L, m, form, 16)
    src = D.index(1021)
    assert b.prefill(src, ref.toks[:1021], 0) == 1021
    for i, d in enumerate(D):
        if i != src and d:
            b.fork(src, i, d)
    if form != "wide":
        # a fork shares the whole pages below d and copies the rows of the partial one into a page of its own; the source's last page (it holds 1021
        # positions, never a multiple of page_len) is shared with nobody
        for i, d in enumerate(D):
            want = (pages_of(1021, form), max(x // form for x in D if x != 1021)) if i == src else (pages_of(d, form), d // form)
            assert b.slot_pages(i) == want, f"{what}: slot {i} forked at {d}"
        n_pages = b.pages()[1]
        assert b.pages()[2] == n_pages - pages_of(1021, form) - sum(1 for d in D if d != 1021 and d % form)
    for i, d in enumerate(D):
        check_ref_rows(b, ref, i, sorted({0, d // 2, d - 1}) if d else [], f"{what}: fork at {d}")
    ref_steps(b, ref, list(range(16)), D, f"{what}: forked rows")
    if form != "wide":
        for i, d in enumerate(D):
            held, shared = b.slot_pages(i)
            assert held == pages_of(min(d + STEPS, N), form), f"{what}: slot {i} after the steps"
            if i != src:
                assert shared == d // form, f"{what}: slot {i}: a step never writes into a page below its fork point"
    check_ref_rows(b, ref, src, [0, 255, 256, 1020], f"{what}: the source after its forks were stepped")


# ---------------------------------------------------------------------------------------------- B. the device loop across deep page edges

KV_CHECKED = {("mini-llama-1k", S.Q8_0), ("mini-llama3b-1k", S.Q8_0), ("mini-gemma-1k", S.Q8_0), ("mini-phi-long", S.Q8_0)}    # one per head size
EDGE = {505: 512, 760: 768}


@functools.lru_cache(maxsize=None)
def branch_rows(cfg, q):
    """K and V rows [layers, 12, kv_dim] that the branches from 505 and from 760 leave at d .. d + 11, from ONE Seq oracle (not the reference's): fed
    toks[:506] and the branch, then - from 506 again, overwriting the branch's rows - toks[506:761] and that branch.  About 800 forwards."""
    ref = reference(cfg, q)
    s = Seq(ref.img, 0)
    out = {}
    for d in (505, 760):
        s.feed(ref.toks[s.n:d])
        t, got = int(ref.toks[d]), []
        for _ in range(N_NEW):
            t = ref_argmax(s.feed([t])); got.append(t)
        assert got == ref.branch[d], f"{cfg} q{q}: the branch from {d} on a second oracle"
        out[d] = [np.stack([np.stack([s.orc.kv_row(w, l, p) for p in range(d, d + N_NEW)]) for l in range(ref.cfg.n_layers)]) for w in (0, 1)]
        s.n = d + 1                                           # (the oracle's rows up to d are toks[:d + 1]'s: the next feed goes on from there)
    return out


@pytest.mark.parametrize("n_rows", [4, 20])
@pytest.mark.parametrize("form", ["wide", 64, 256])
@pytest.mark.parametrize("cfg,q", CFGS)
def test_device_loop_across_deep_page_edges(L, cfg, q, form, n_rows):
    """generate_greedy of 12 steps from 250, 505, 760 and 1010: across the 256-key passes' edges at 256, 512 and 768 (page edges of both lengths) and up to
    position 1021.  20 rows: five slots a depth, four of them forks - equal rows.  (mini-gemma's greedy continuation is one token repeated: its rows check
    the loop's page crossings and positions, not varied inputs - groups A, D and E carry its arithmetic.)"""
    ref = reference(cfg, q)
    what = f"{cfg} q{q} {form} n {n_rows}"
    per = n_rows // 4
    m = L.Transformer(ref.img)
    b = make_batch(L, m, form, n_rows)
    for j, d in enumerate(STARTS):
        assert b.prefill(j * per, ref.toks[:d], 0) == d
        for f in range(1, per):
            b.fork(j * per, j * per + f, d)
    slots = list(range(n_rows))
    depth = [STARTS[s // per] for s in slots]
    out = b.generate_greedy(slots, [int(ref.toks[d]) for d in depth], depth, N_NEW)
    assert out.shape == (n_rows, N_NEW)
    for i, d in enumerate(depth):
        assert out[i].tolist() == ref.branch[d], f"{what}: row {i} (slot {slots[i]} from {d})"
    if form != "wide":
        for s, d in zip(slots, depth):
            assert b.slot_pages(s)[0] == pages_of(d + N_NEW, form), f"{what}: slot {s} after the loop"
    if (cfg, q) in KV_CHECKED:
        rows = branch_rows(cfg, q)
        for d, edge in EDGE.items():
            base = STARTS.index(d) * per
            for s in sorted({base, base + per - 1}):
                for layer in range(ref.cfg.n_layers):
                    for p in (d, edge - 1, edge, d + N_NEW - 1):
                        for w in (0, 1):
                            assert_bit_equal(b.kv_row(s, w, layer, p), rows[d][w][layer, p - d], f"{what}: slot {s} {'kv'[w]} layer {layer} pos {p} left by the loop")


# ---------------------------------------------------------------------------------------------- C. embedding rows in two chunks on pages

@pytest.mark.parametrize("page_len", [64, 512])
def test_embedding_rows_in_two_chunks_on_pages(L, page_len):
    """tests/test_batch_embed.py::test_prefill_embeddings_is_one_fill_kv_cache's 530-row case on a paged batch: a 512-row chunk and an 18-row one whose
    rows attend over the first chunk's pages"""
    cfg, q, n, start = "mini-phi-long", S.Q8_0, 530, 3
    img = S.build_image(cfg, q, seed=711)
    m = L.Transformer(img)
    b = L.Batch(m, 3, page_len=page_len, n_pages=2 * pages_of(start + n + 2, page_len))
    s = EmbedSeq(img, 1)
    toks = S.prompt_tokens(cfg, start, 712)
    b.prefill(1, toks, 0); s.feed(toks)
    rows = random_rows(n, m.args.dim, 713)
    keep = rows.copy()
    end, res = b.prefill_embeddings(1, rows, start, residual=True)
    assert end == start + n and b.slot_pages(1) == (pages_of(start + n, page_len), 0)
    assert_bit_equal(rows, keep, "the caller's rows are never written")
    want = s.fill(rows)
    what = f"{cfg} q{q} n {n} at {start}, page_len {page_len}"
    assert_bit_equal(res, want, f"{what}: residual against the oracle's mutated embeddings")
    check_slot_rows(b, s, sorted(set(run_positions(start, n)) | {start + 511, start + 512}), what)
    for k in range(2):
        pos, tok = s.n, 11 + k
        am, lg = b.forward([1], [tok], [pos], logits=True)
        assert_bit_equal(lg[0], s.feed([tok]), f"{what}: forward step {k} on the slot")
    # the same rows into another slot without the download: the same K/V rows
    b.prefill(2, toks, 0)
    assert b.prefill_embeddings(2, rows, start) == start + n
    for layer in range(m.args.n_layers):
        for p in run_positions(start, n):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(2, w, layer, p), s.orc.kv_row(w, layer, p), f"{what}: residual=False, {'kv'[w]} layer {layer} pos {p}")


# ---------------------------------------------------------------------------------------------- D. copy on write, release, the context fork: 256-position pages

@pytest.mark.parametrize("cfg,q", [("mini-llama-1k", S.Q8_0), ("mini-gemma-1k", S.Q4_0)])
def test_unshare_release_and_context_fork_on_256_position_pages(L, cfg, q):
    ref = reference(cfg, q)
    PL, n_pages = 256, 12
    nl = ref.cfg.n_layers
    m = L.Transformer(ref.img)
    b = L.Batch(m, 4, page_len=PL, n_pages=n_pages)
    # --- fork and un-share
    assert b.prefill(0, ref.toks[:700], 0) == 700
    b.fork(0, 1, 700); b.fork(0, 2, 700)
    for s in range(3):
        assert b.slot_pages(s) == (3, 2), f"{cfg} q{q}: slot {s} after the forks"
    assert b.pages() == (PL, n_pages, n_pages - 5)
    at = [0, 255, 256, 299, 300, 309, 310, 511, 512, 699]
    before = {s: snapshot(b, s, at, nl) for s in (0, 2)}
    other = S.prompt_tokens(ref.cfg, 10, SEED + 1)
    assert b.prefill(1, other, 300) == 310                   # into the shared page 1: a whole-page copy first
    for s in (0, 2):
        for x, y in zip(before[s], snapshot(b, s, at, nl)):
            assert_bit_equal(x, y, f"{cfg} q{q}: slot {s} moved by slot 1's write into a shared page")
        check_ref_rows(b, ref, s, at, f"{cfg} q{q}: slot {s} beside slot 1's write")
    s1 = Seq(ref.img, 1)
    s1.feed(ref.toks[:300]); s1.feed(other)
    check_slot_rows(b, s1, range(300, 310), f"{cfg} q{q}: slot 1's own rows")
    check_ref_rows(b, ref, 1, [0, 255, 256, 299, 310, 511, 512, 699], f"{cfg} q{q}: the rows the page copy kept")
    # slot 1 shares page 0 only; slots 0 and 2 still share pages 0 and 1 with each other
    assert b.slot_pages(1) == (3, 1) and b.slot_pages(0) == (3, 2) and b.slot_pages(2) == (3, 2) and b.pages()[2] == n_pages - 6
    step(b, [s1], [int(ref.toks[310])], f"{cfg} q{q}: slot 1 at 310, behind its write")
    # --- release
    keep = [0, 299, 300, 511]
    kept = snapshot(b, 2, keep, nl)
    b.release(2, 300)
    assert b.slot_pages(2) == (2, 2) and b.pages()[2] == n_pages - 5, "release(slot, 300) keeps two pages of 256 positions"
    for x, y in zip(kept, snapshot(b, 2, keep, nl)):
        assert_bit_equal(x, y, f"{cfg} q{q}: a kept position moved by the release")
    for layer in range(nl):
        for p in (512, 699):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(2, w, layer, p), zero_row(m), f"{cfg} q{q}: released position {p}")
    assert b.prefill(2, ref.toks[512:600], 512) == 600
    assert b.slot_pages(2) == (3, 2)
    check_ref_rows(b, ref, 2, range(512, 600), f"{cfg} q{q}: rows 512 .. 599 written again")
    am, lg = b.forward([2], [int(ref.toks[600])], [600], logits=True)
    assert_bit_equal(lg[0], ref.logits[600], f"{cfg} q{q}: the step at 600 after release and prefill")
    assert int(am[0]) == ref_argmax(ref.logits[600])
    # --- fork from the context's own (contiguous) cache
    assert m.prefill_tokens(ref.toks[:700], 0) == 700
    free = b.pages()[2]
    b.fork(L.BATCH_CTX, 3, 700)
    assert b.slot_pages(3) == (3, 0) and b.pages()[2] == free - 3
    for layer in range(nl):
        for p in (0, 255, 256, 511, 512, 699):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(3, w, layer, p), m.kv_row(w, layer, p), f"{cfg} q{q}: fork from the context, {'kv'[w]} layer {layer} pos {p}")
        for w in (0, 1):
            assert_bit_equal(b.kv_row(3, w, layer, 700), zero_row(m), f"{cfg} q{q}: behind the forked rows")
    check_ref_rows(b, ref, 3, [0, 255, 256, 511, 512, 699], f"{cfg} q{q}: fork from the context")
    am, lg = b.forward([3], [int(ref.toks[700])], [700], logits=True)
    assert_bit_equal(lg[0], ref.logits[700], f"{cfg} q{q}: the step at 700 on the context's fork")
    assert int(am[0]) == ref_argmax(ref.logits[700])
    check_ref_rows(b, ref, 3, [700], f"{cfg} q{q}: the row that step wrote")


# ---------------------------------------------------------------------------------------------- E. Gemma's window on pages, differential

def window_calls(b, cfg, V):
    """one call sequence on a batch of 20 slots, slot 0 beyond Gemma-2's 4096-key window -> the uint32 view of everything it returns"""
    u = lambda x: np.ascontiguousarray(x).view(np.uint32).copy()
    lengths = [4100] + [i % 4 for i in range(19)]
    for i, n in enumerate(lengths):
        if n:
            assert b.prefill(i, S.prompt_tokens(cfg, n, 29 + i), 0) == n                 # slot 0: nine chunks on pages
    out, slots = [], list(range(20))
    for k in range(2):
        out += [u(x) for x in b.forward(slots, [(50 + k + i) % V for i in slots], [n + k for n in lengths], logits=True)]
    out += [u(x) for x in b.forward(slots[::-1], [(90 + i) % V for i in slots], [n + 2 for n in lengths[::-1]], logits=True)]
    out.append(u(b.generate_greedy([0, 1, 2, 3], [7, 8, 9, 10], [lengths[i] + 3 for i in range(4)], 4)))
    nl = b.model.args.n_layers
    for layer in range(nl):
        out += [u(b.kv_row(0, w, layer, p)) for p in [0, 3, 4, 4095, 4096, 4099] + list(range(4100, 4107)) for w in (0, 1)]
        for s in (1, 2, 3, 19):
            out += [u(b.kv_row(s, w, layer, p)) for p in range(lengths[s], lengths[s] + 7) for w in (0, 1)]
    return out


def test_gemma_window_on_pages_against_the_wide_batch(L):
    """Differential: tests/test_batch_wide.py::test_gemma_window_per_row_in_a_wide_pass pins the wide batch against the oracle on this image at exactly
    these positions, so the paged batches are held to the wide batch's bits and no second oracle run of 4100 forwards is needed.  The paged kernel has
    its own copy of the window logic (wpos, gemma_cap_window): slot 0's queries mask keys 0 .. pos - 4097, the 19 shallow rows mask none."""
    cfg = dataclasses.replace(S.CONFIGS["mini-gemma"], name="mini-gemma-window", max_pos=4352)
    img = S.build_image(cfg, S.Q8_0, 29)
    m = L.Transformer(img)
    wide = L.Batch(m, 20, wide=True)
    want = window_calls(wide, cfg, m.args.vocab_size)
    wide.close()
    for page_len in (64, 1024):
        b = L.Batch(m, 20, page_len=page_len, n_pages=pages_of(4352, page_len) + 19 + 4)
        got = window_calls(b, cfg, m.args.vocab_size)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and (g == w).all(), f"page_len {page_len}: output {i} of the window calls differs from the wide batch"
        assert b.slot_pages(0) == (pages_of(4107, page_len), 0)
        b.close()


# ---------------------------------------------------------------------------------------------- F. pages above 2^32 bytes, 2^31 floats, 2^32 floats

def test_pages_high_in_a_pool_of_17_gb(L):
    """mini-phi's geometry with 8192 positions, pages of 1024 positions (48 MiB each), a pool of 352 pages.  The pool hands out pages 1, 2, 3, .. while
    nothing is released (lmrs_pages.cpp), so n_pages - n_free is the highest page claimed: single-row steps on burner slots at positions k * 1024 claim a
    page each, until the next page claimed lies wholly above 2^30 floats (2^32 bytes), 2^31 floats, 2^32 floats; then a fresh probe slot takes its first
    call there.  One Seq oracle of 73 forwards serves the three probes.  Short of memory the create call fails with the library's message."""
    cfg = dataclasses.replace(S.CONFIGS["mini-phi"], name="mini-phi-8k", max_pos=8192)
    img = S.build_image(cfg, S.Q8_0, seed=721)
    m = L.Transformer(img)
    PL, n_slots, n_pages = 1024, 64, 352
    a = m.args
    nl, per_slot = a.n_layers, a.seq_len // PL
    stride = 2 * nl * PL * a.n_kv_heads * a.head_size        # floats a page
    targets = [-(-(1 << e) // stride) for e in (30, 31, 32)]  # the first page that starts at or above 2^e floats; the probe's page lies one higher
    assert targets[-1] + 2 <= n_pages and targets[0] > 2 and all(y - x > 2 for x, y in zip(targets, targets[1:]))
    toks = S.prompt_tokens(cfg, 73, 722)
    s = Seq(img, 0)
    s.feed(toks[:70])
    want_kv = {p: [[s.orc.kv_row(w, l, p).copy() for w in (0, 1)] for l in range(nl)] for p in (0, 35, 69)}
    want_lg = [s.feed([t]) for t in toks[70:]]
    for k in range(3):
        want_kv[70 + k] = [[s.orc.kv_row(w, l, 70 + k).copy() for w in (0, 1)] for l in range(nl)]
    b = L.Batch(m, n_slots, page_len=PL, n_pages=n_pages)
    claimed = lambda: n_pages - b.pages()[2]
    burners = list(range(6, n_slots))
    spots = [(slot, k) for k in range(per_slot) for slot in burners]     # every (slot, k) names a page nobody claimed; a call takes each slot once
    assert len(spots) >= targets[-1]

    def burn_to(target):
        while claimed() < target:
            n = min(len(burners), target - claimed())
            take, spots[:] = spots[:n], spots[n:]
            assert len({slot for slot, _ in take}) == n
            b.forward([slot for slot, _ in take], [1] * n, [k * PL for _, k in take])
        assert claimed() == target

    def check_rows(slot, positions, what):
        for p in positions:
            for l in range(nl):
                for w in (0, 1):
                    assert_bit_equal(b.kv_row(slot, w, l, p), want_kv[p][l][w], f"{what}: slot {slot} {'kv'[w]} layer {l} pos {p}")

    for i, target in enumerate(targets):
        probe, twin = 2 * i, 2 * i + 1
        burn_to(target)
        what = f"page {target + 1}, at {(target + 1) * stride} floats"
        assert (target + 1) * stride >= 1 << (30 + i)
        assert b.prefill(probe, toks[:70], 0) == 70
        assert claimed() == target + 1 and b.slot_pages(probe) == (1, 0)
        check_rows(probe, [0, 35, 69], f"{what}: prefill")
        for l in range(nl):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(probe, w, l, 100), zero_row(m), f"{what}: the claimed page was cleared")
        for k in range(3):
            am, lg = b.forward([probe], [int(toks[70 + k])], [70 + k], logits=True)
            assert_bit_equal(lg[0], want_lg[k], f"{what}: step {k}")
            assert int(am[0]) == ref_argmax(want_lg[k])
            check_rows(probe, [70 + k], f"{what}: step {k}")
        b.fork(probe, twin, 70)                              # the partial page's rows into the next page up
        assert claimed() == target + 2 and b.slot_pages(twin) == (1, 0) and b.slot_pages(probe) == (1, 0)
        check_rows(twin, [0, 35, 69], f"{what}: the fork's copied rows")
        am, lg = b.forward([twin], [int(toks[70])], [70], logits=True)
        assert_bit_equal(lg[0], want_lg[0], f"{what}: the step on the fork")
        check_rows(twin, [70], f"{what}: the step on the fork")
        check_rows(probe, [0, 69, 70, 72], f"{what}: the probe after its fork was stepped")
