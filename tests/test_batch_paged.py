"""Paged K/V for batches (lmrs_batch_create_paged, include/lmrs_hip.h): the slots draw pages from one pool, fork shares pages, a write un-shares them,
release gives them back.  Paging changes addresses only, so the references are the existing ones: one CPU oracle PER SEQUENCE (the Seq pattern of
tests/test_batch.py) and, for whole call sequences, a lmrs_batch_create_wide batch fed the same calls.  Every comparison is bit for bit.  The mini
fixtures' 256 positions with page_len = 64 give four pages a slot, so every page edge is reached in a few tokens."""
import numpy as np
import pytest

from parity_rules import assert_bit_equal, ref_argmax
from test_batch import CFGS, Seq, check_slot_rows, snapshot, step
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
PL = 64


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def pages_of(n):
    return -(-n // PL)


def zeros_like_row(m):
    return np.zeros(m.args.n_kv_heads * m.args.head_size, np.float32)


# ---------------------------------------------------------------------------------------------- 1. rows on scattered pages, every edge

# both sides of every page edge of the fixtures' 256 positions, the ends, and a few shallow rows
DEPTHS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 252, 2, 32, 96]


@gpu
@pytest.mark.parametrize("cfg,q", CFGS)
def test_rows_on_scattered_pages(L, cfg, q):
    """16 slots prefilled in two chunks each, round robin, so that the slots' pages interleave in the pool - after a few pages were claimed and
    released, so that the free list is not ascending either; then three steps of all 16 rows with logits"""
    img = S.build_image(cfg, q, seed=501)
    m = L.Transformer(img)
    b = L.Batch(m, 16, page_len=PL, n_pages=64)
    assert b.pages() == (PL, 64, 64) and b.width == 64
    b.prefill(15, S.prompt_tokens(cfg, 200, 1), 0)
    b.prefill(3, S.prompt_tokens(cfg, 70, 2), 0)
    b.release(15, 64)
    b.release(3)
    b.release(15)
    assert b.pages() == (PL, 64, 64)
    seqs = [Seq(img, i) for i in range(16)]
    toks = [S.prompt_tokens(cfg, n, 510 + i) if n else [] for i, n in enumerate(DEPTHS)]
    for first in (True, False):
        for i, n in enumerate(DEPTHS):
            a = n // 2
            part = toks[i][:a] if first else toks[i][a:]
            if len(part):
                assert b.prefill(i, part, 0 if first else a) == (a if first else n)
    held = 0
    for s, n in zip(seqs, DEPTHS):
        s.feed(toks[s.slot])
        assert b.slot_pages(s.slot) == (pages_of(n), 0), f"slot {s.slot} after a prefill of {n}"
        held += pages_of(n)
        check_slot_rows(b, s, sorted({0, n // 2, n - 1}) if n else [], f"{cfg} q{q}: paged prefill of {n}")
    assert b.pages() == (PL, 64, 64 - held)
    V = seqs[0].orc.args.vocab_size
    for k in range(3):
        step(b, seqs, [(13 * i + 5 * k + 3) % V for i in range(16)], f"{cfg} q{q} paged step {k}")
    assert b.pages()[2] == 64 - sum(pages_of(n + 3) for n in DEPTHS)


# ---------------------------------------------------------------------------------------------- 2. fork shares, writes un-share

@gpu
@pytest.mark.parametrize("cfg,q", CFGS)
def test_fork_shares_and_writes_unshare(L, cfg, q):
    img = S.build_image(cfg, q, seed=521)
    m = L.Transformer(img)
    b = L.Batch(m, 9, page_len=PL, n_pages=40)
    prefix = S.prompt_tokens(cfg, 190, 522)
    b.prefill(0, prefix, 0)
    for d in range(1, 8):
        b.fork(0, d, 190)
    assert b.pages() == (PL, 40, 40 - (3 + 7)), "a fork of 190 positions shares two pages and copies the rows of the third"
    for s in range(8):
        assert b.slot_pages(s) == (3, 2), f"slot {s}"
    seqs = [Seq(img, i) for i in range(8)]
    for s in seqs:
        s.feed(prefix)
    check_slot_rows(b, seqs[5], [0, 64, 127, 128, 189], f"{cfg} q{q}: the forked prefix")
    V = seqs[0].orc.args.vocab_size
    for k in range(3):                                       # positions 190, 191 and - in a page of its own - 192
        step(b, seqs, [(31 * i + 7 * k + 1) % V for i in range(8)], f"{cfg} q{q} forked step {k}")
    for s in range(8):
        assert b.slot_pages(s) == (4, 2), f"slot {s} after crossing position 192"
    if (cfg, q) in (("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)):
        # slot 1 rewrites positions 10 .. 19 of the shared first page: it gets a copy, everybody else keeps the page
        nl, at = seqs[0].orc.args.n_layers, [0, 9, 10, 19, 20, 63, 64, 189, 192]
        before = {s: snapshot(b, s, at, nl) for s in (0, 2)}
        other = S.prompt_tokens(cfg, 10, 523)
        assert b.prefill(1, other, 10) == 20
        for j, t in enumerate(other):
            seqs[1].orc.forward(int(t), 10 + j)
        for s in (0, 2):
            for x, y in zip(before[s], snapshot(b, s, at, nl)):
                assert_bit_equal(x, y, f"{cfg} q{q}: slot {s} moved by slot 1's write into a shared page")
        check_slot_rows(b, seqs[1], at + [12, 15], f"{cfg} q{q}: slot 1 after its write")
        assert b.slot_pages(1) == (4, 1) and b.slot_pages(0) == (4, 2) and b.slot_pages(2) == (4, 2)
    # from the context's own (contiguous) cache: the rows are copied into pages of the slot's own
    own = S.prompt_tokens(cfg, 70, 524)
    m.prefill_tokens(own, 0)
    free = b.pages()[2]
    b.fork(L.BATCH_CTX, 8, 70)
    assert b.slot_pages(8) == (2, 0) and b.pages()[2] == free - 2
    for layer in range(seqs[0].orc.args.n_layers):
        for p in (0, 35, 63, 64, 69):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(8, w, layer, p), m.kv_row(w, layer, p), f"{cfg} q{q}: fork from the context, {'kv'[w]} layer {layer} pos {p}")
        for w in (0, 1):
            assert_bit_equal(b.kv_row(8, w, layer, 70), zeros_like_row(m), f"{cfg} q{q}: behind the forked rows")


# ---------------------------------------------------------------------------------------------- 3. exhaustion and release

@gpu
def test_exhaustion_and_release(L):
    """A pool of 5 pages.  (A call that wants 6 pages can never succeed in it - un-sharing keeps what it copies - so the call that succeeds there after
    the release is a second refused one, which wants 2 pages with none free; the 6-page call itself is refused and then, after a release, served in
    a pool of 8 pages of which 4 were held.)"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=531)
    m = L.Transformer(img)
    b = L.Batch(m, 4, page_len=PL, n_pages=5)
    seqs = [Seq(img, i) for i in range(4)]
    nl = seqs[0].orc.args.n_layers
    t0 = S.prompt_tokens(cfg, 70, 532)
    b.prefill(0, t0, 0)
    seqs[0].feed(t0)
    t1, t2 = S.prompt_tokens(cfg, 130, 533), S.prompt_tokens(cfg, 65, 534)
    state = lambda: (b.pages(), [b.slot_pages(s) for s in range(4)])
    before, rows0 = state(), snapshot(b, 0, [0, 35, 63, 64, 69], nl)
    assert before[0] == (PL, 5, 3)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward_runs: 6 pages wanted, 3 free"):
        b.forward_runs([(1, 0, t1, 1), (2, 0, t2, 1), (3, 0, [7], 1)])
    assert state() == before
    for x, y in zip(rows0, snapshot(b, 0, [0, 35, 63, 64, 69], nl)):
        assert_bit_equal(x, y, "slot 0 moved by a refused call")
    for s in (1, 2, 3):
        assert_bit_equal(b.kv_row(s, 0, 0, 0), zeros_like_row(m), f"slot {s} written by a refused call")
    # the next smaller call: three pages, three free
    am = b.forward_runs([(1, 0, t1, 1)])
    want1 = ref_argmax(seqs[1].feed(t1))
    assert int(am[0]) == want1
    check_slot_rows(b, seqs[1], [0, 64, 129], "the smaller call")
    assert b.pages() == (PL, 5, 0)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward_runs: 2 pages wanted, 0 free"):
        b.forward_runs([(2, 0, t2, 1)])
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward: 1 pages wanted, 0 free"):
        b.forward([3], [7], [0])
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_fork: 1 pages wanted, 0 free"):
        b.fork(1, 3, 10)
    b.release(0)
    assert b.pages() == (PL, 5, 2) and b.slot_pages(0) == (0, 0)
    for p in (0, 35, 69):
        for w in (0, 1):
            assert_bit_equal(b.kv_row(0, w, 1, p), zeros_like_row(m), f"released position {p}")
    am = b.forward_runs([(2, 0, t2, 1)])                      # the refused call, into slot 0's former pages
    want2 = ref_argmax(seqs[2].feed(t2))
    assert int(am[0]) == want2
    check_slot_rows(b, seqs[2], [0, 63, 64], "the refused call after the release")
    for p in (65, 70, 100, 127):                             # claimed with position 64, not written: a reclaimed page was cleared
        for layer in range(nl):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(2, w, layer, p), zeros_like_row(m), f"position {p} of a reclaimed page")
    check_slot_rows(b, seqs[1], [0, 64, 129], "slot 1 after its neighbours came and went")
    # a partial release keeps the pages of the positions it keeps
    b.release(1, 65)
    assert b.slot_pages(1) == (2, 0) and b.pages()[2] == 1
    check_slot_rows(b, seqs[1], [0, 64, 127], "the kept positions")
    assert_bit_equal(b.kv_row(1, 0, 0, 128), zeros_like_row(m), "a released position")
    # argument errors, each with a message of its own
    plain = L.Batch(m, 2)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_release: not a paged batch"):
        plain.release(0)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_pages: not a paged batch"):
        plain.pages()
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_slot_pages: not a paged batch"):
        plain.slot_pages(0)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_release: slot 4 of 4"):
        b.release(4)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_slot_pages: slot 9 of 4"):
        b.slot_pages(9)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_release: n_pos = 257 exceeds seq_len"):
        b.release(1, 257)
    assert b.pages() == (PL, 5, 1)
    b.close()
    # the 6-page call in a pool it can fit: refused while slot 0 holds 4 of the 8 pages, served once slot 0 has let go of them
    b = L.Batch(m, 4, page_len=PL, n_pages=8)
    b.prefill(0, S.prompt_tokens(cfg, 200, 535), 0)
    six = [(1, 0, t1, 1), (2, 0, t2, 1), (3, 0, [7], 1)]
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward_runs: 6 pages wanted, 4 free"):
        b.forward_runs(six)
    assert b.pages() == (PL, 8, 4)
    b.release(0)
    am = b.forward_runs(six)
    assert am.tolist() == [want1, want2, ref_argmax(seqs[3].feed([7]))] and b.pages() == (PL, 8, 2)
    for s, at in ((1, [0, 64, 129]), (2, [0, 63, 64]), (3, [0])):
        check_slot_rows(b, seqs[s], at, "the 6-page call after the release")
    assert_bit_equal(b.kv_row(3, 1, 0, 1), zeros_like_row(m), "a reclaimed page behind the one row written")


# ---------------------------------------------------------------------------------------------- 4. differential against the wide batch

def scripted(L, m, b, cfg, phi):
    """one call sequence on a batch of 60 slots -> the uint32 view of everything it returns"""
    V, out = m.args.vocab_size, []
    u = lambda x: np.ascontiguousarray(x).view(np.uint32).copy()
    # 40 rows decode greedily from position 60 (nothing was written below it: zeros on both sides) across the edge at 64
    out.append(u(b.generate_greedy(list(range(40)), [(37 * i + 11) % V for i in range(40)], [60] * 40, 10)))
    # 12 rows - the 16-row table and its advance on the device - across the edges at 64 and at 128
    out.append(u(b.generate_greedy(list(range(48, 60)), [(41 * i + 3) % V for i in range(12)], [58] * 12, 10)))
    out.append(u(b.generate_greedy(list(range(48, 60)), [(43 * i + 5) % V for i in range(12)], [122] * 12, 10)))
    # runs that straddle edges, a verified draft with every row's output, decode rows beside them
    runs = [(40, 50, S.prompt_tokens(cfg, 30, 541), 1), (41, 120, S.prompt_tokens(cfg, 16, 542), 16), (0, 70, [5], 1), (7, 70, [6], 1), (42, 0, [9], 1)]
    out += [u(x) for x in b.forward_runs(runs, k=8, logits=True)]
    kinds = [(0.0, 0.9), (0.8, 1.0), (0.02, 0.9), (3.0, 0.999)]       # argmax, sample_mult, peaked and flat top-p
    samplers = [L.Sampler(V, *kinds[i % 4], 5500 + i) for i in range(8)]
    for k in range(2):
        sr = [(i, 71 + k, [(3 * i + k) % V], samplers[i]) for i in range(6)] + [(43, 60, S.prompt_tokens(cfg, 9, 543 + k), samplers[6]), (44 + k, 0, [1, 2, 3], None)]
        out.append(u(b.forward_runs_sample(sr)))
    out.append(u(np.array([s.info() for s in samplers], np.float32)))
    out.append(u(b.forward_sample([1, 2, 3, 46], [4, 5, 6, 7], [73, 73, 73, 0], samplers[:4])))
    out.append(u(b.forward(list(range(20)), [(5 * i + 2) % V for i in range(20)], [74] * 4 + [70] * 16, logits=True)[1]))
    if phi:
        e = m.get_embeddings(S.prompt_tokens(cfg, 80, 545)).reshape(80, -1)
        out += [u(x) for x in b.forward_runs([(47, 30, e[:40], 2), (0, 75, [8], 1)], logits=True)]
        n, res = b.prefill_embeddings(46, e, 100, residual=True)
        assert n == 180
        out.append(u(res))
        assert b.prefill_embeddings(45, e[:1], 63) == 64
    b.fork(40, 45, 70)
    for slot, at in ((0, [0, 59, 60, 63, 64, 69, 70, 75]), (41, [119, 120, 127, 128, 135]), (40, [50, 63, 64, 79]), (43, [60, 68, 69]), (45, [0, 63, 64, 69, 70]),
                     (46, [0, 99, 100, 127, 128, 179, 180]), (47, [30, 63, 64, 69]), (50, [58, 63, 64, 67, 68, 122, 127, 128, 131, 132])):
        for layer in range(m.args.n_layers):
            out += [u(b.kv_row(slot, w, layer, p)) for p in at for w in (0, 1)]
    return out


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_the_same_calls_on_a_wide_batch(L, cfg, q):
    img = S.build_image(cfg, q, seed=551)
    m = L.Transformer(img)
    wide = L.Batch(m, 60, wide=True)
    want = scripted(L, m, wide, cfg, cfg == "mini-phi")
    wide.close()
    for page_len in (64, 128):
        b = L.Batch(m, 60, page_len=page_len, n_pages=160)
        got = scripted(L, m, b, cfg, cfg == "mini-phi")
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and (g == w).all(), f"{cfg} q{q} page_len {page_len}: output {i} of the scripted calls differs from the wide batch"
        b.close()


# ---------------------------------------------------------------------------------------------- 5. the create refusals

@gpu
def test_create_refusals(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=561)
    m = L.Transformer(img)
    for bad in (0, 1, 32, 63, 65, 96, 192, 2048):
        with pytest.raises(L.LmrsError, match=rf"lmrs_batch_create_paged: page_len = {bad} is none of"):
            L.Batch(m, 4, page_len=bad, n_pages=8)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_create_paged: n_pages is 0"):
        L.Batch(m, 4, page_len=64, n_pages=0)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_create_paged: n_slots = 65 is outside 1 \.\. 64"):
        L.Batch(m, 65, page_len=64, n_pages=8)
    with pytest.raises(L.LmrsError, match=r"page_len and n_pages must be given together"):
        L.Batch(m, 4, page_len=64)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_create_paged: unquantised \(f32\) files have no batched pass"):
        L.Batch(L.Transformer(S.build_image("mini-llama", S.Q_NONE, seed=561)), 4, page_len=64, n_pages=8)
    for page_len in (64, 128, 256, 512, 1024):              # every allowed length, longer than the fixture's 256 positions included
        b = L.Batch(m, 2, page_len=page_len, n_pages=3)
        assert b.pages() == (page_len, 3, 3)
        am = b.forward([1], [5], [200])
        assert b.slot_pages(1) == (1, 0) and am.shape == (1,)
        b.close()
