"""The batched stack on the corners of the geometry lattice it admits (tools/synth_lmrs.py::lattice_corners; prefill_batched_ok in lmrs_api.hip), run with
`-m gpu` on an MI355X against the CPU oracle, bit for bit (tests/parity_rules.py).  Every batched entry point is gated by that one predicate and the
kernel of every GEMM is chosen per launch from (n, o, tokens, format): tests/test_lattice_host.py proves on the host that these corners, at the token
counts below (imported from there), reach every instantiation the lattice can.  Admission is asserted, never assumed: a corner that falls back to the
token-by-token path, or whose batch is refused, fails.  One image per (corner, format), cached and read-only; every reference is one oracle run."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, check_after, check_scores, oracle_rows, ref_argmax, run_positions
from test_batch import Seq, check_slot_rows, prefilled, step
from test_batch_runs import run_pass, toks_for
from test_lattice_host import CORNERS, FILL_TOKENS, SCORE_TOKENS
from test_topk import check_topk
from test_verify import _gemm_operands, _gemm_reference
from tools import synth_lmrs as S

pytestmark = pytest.mark.gpu

FORMATS = (S.Q8_0, S.Q4_0)
CASES = [(name, q) for name in CORNERS for q in FORMATS]
PREFIX = 8                                                     # cached rows in front of every other fill of a corner
# (corner, format, tokens, first position): the counts the host test certified, by turns on an empty cache and behind PREFIX rows
FILLS = [(name, q, t, PREFIX * (i % 2)) for name, q in CASES for i, t in enumerate(FILL_TOKENS[name])]
VERIFY_NS = (2, 9, 16)
PAGED = ("w1024-h1024", "w1024-att3072", "gemma-att1024")      # head sizes 64, 96 and 256


def ids(cases):
    return [f"{c[0]}-{'q4' if c[1] == S.Q4_0 else 'q8'}" + "".join(f"-{x}" for x in c[2:]) for c in cases]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


@functools.lru_cache(maxsize=None)
def image(name, q):
    img = S.build_image(CORNERS[name], q, seed=401)
    img.setflags(write=False)
    return img


def fill_reference(name, q, n_tok, pos0):
    """The oracle's side of one fill: pos0 single-token steps (their logits kept), fill_kv_cache of n_tok rows, the K/V rows it left, two decode steps"""
    c = CORNERS[name]
    orc = O.Oracle(image(name, q))
    pre = S.prompt_tokens(c, pos0, 402)
    steps = [orc.forward(int(t), p).copy() for p, t in enumerate(pre)]
    b = orc.get_embeddings(S.prompt_tokens(c, n_tok, 403))
    assert orc.fill_kv_cache(b, pos0) == pos0 + n_tok and np.isfinite(b).all()
    kv = {(w, l, p): orc.kv_row(w, l, p).copy() for w in (0, 1) for l in range(c.n_layers) for p in run_positions(pos0, n_tok)}
    after, t = [], 7
    for pos in range(pos0 + n_tok, pos0 + n_tok + 2):
        lo = orc.forward(t, pos).copy()
        after.append((t, pos, lo)); t = ref_argmax(lo)
    b.setflags(write=False)
    return pre, steps, b, kv, after


def token_reference(name, q):
    """The oracle's sequential forward over one token run as long as the corner's longest scoring call -> (tokens, logits rows), read-only"""
    c = CORNERS[name]
    toks = S.prompt_tokens(c, max(SCORE_TOKENS[name]), 404)
    rows = oracle_rows(O.Oracle(image(name, q)), toks, 0)
    rows.setflags(write=False)
    return toks, rows


# ---------------------------------------------------------------------------------------------- 1. fill_kv_cache

@pytest.mark.parametrize("name,q,n_tok,pos0", FILLS, ids=ids(FILLS))
def test_fill_kv_cache_on_a_corner(L, name, q, n_tok, pos0):
    """Single-token steps from an empty cache (the decode step's GEMV classes at the corner's widths), then one fill_kv_cache of n_tok rows behind
    them: the whole residual stream, the K and V rows of every layer at the first, middle and last position, two decode steps on that cache.  The
    batched pass ran: only it records lmrs_last_fill_ms."""
    c = CORNERS[name]
    pre, steps, b, kv, after = fill_reference(name, q, n_tok, pos0)
    m = L.Transformer(image(name, q))
    what = f"{name} q{q}, {n_tok} tokens at {pos0}"
    for p, t in enumerate(pre):
        assert_bit_equal(m.forward(int(t), p), steps[p], f"{what}: single-token step at {p}")
    a = m.get_embeddings(S.prompt_tokens(c, n_tok, 403))
    assert m.fill_kv_cache(a, pos0) == pos0 + n_tok
    assert m.last_fill_ms() > 0, f"{what}: fill_kv_cache fell back to the token-by-token path"
    assert_bit_equal(a.reshape(-1), b.reshape(-1), f"{what}: residual stream after the batched layers")
    for (w, l, p), row in kv.items():
        assert_bit_equal(m.kv_row(w, l, p), row, f"{what}: {'kv'[w]} row layer {l} pos {p}")
    for t, pos, lo in after:
        assert_bit_equal(m.forward(t, pos), lo, f"{what}: decode at {pos} on the prefilled cache")
    m.close()


# ---------------------------------------------------------------------------------------------- 2. token runs

@pytest.mark.parametrize("name,q", CASES, ids=ids(CASES))
def test_token_runs_on_a_corner(L, name, q):
    """verify_tokens at 2, 9 and 16 tokens (the skinny GEMM), score_tokens and score_tokens_topk at the corner's scoring lengths (the classifier
    launch; score chunks at vocabularies of 272 and 4112), prefill_tokens - each as ONE batched pass (lmrs_tokens_path), against the oracle's
    sequential forward."""
    toks, rows = token_reference(name, q)
    img = image(name, q)
    m = L.Transformer(img); orc = O.Oracle(img)
    what = f"{name} q{q}"
    for n in VERIFY_NS:
        am, acc = m.verify_tokens(toks[:n], 0)
        want = [ref_argmax(r) for r in rows[:n]]
        assert am.tolist() == want, f"{what}: verify_tokens of {n}"
        assert acc == next((i for i in range(n - 1) if int(toks[i + 1]) != want[i]), n - 1)
    for t in range(max(VERIFY_NS)):
        orc.forward(int(toks[t]), t)
    check_after(m, orc, max(VERIFY_NS), 0, f"{what}: verify_tokens of {max(VERIFY_NS)}")
    for n in SCORE_TOKENS[name]:
        assert m.tokens_path(n), f"{what}: a run of {n} tokens is not one batched pass"
        check_scores(m.score(toks[:n], 0), rows[:n], toks[:n], f"{what}: score of {n}")
    n = min(SCORE_TOKENS[name], key=lambda t: abs(t - 60))
    k = 8
    got = m.score_topk(toks[:n], k, 0)
    check_topk(L, img, got, rows[:n], toks[:n], 0, k, f"{what}: score_topk of {n}")
    m2 = L.Transformer(img)
    assert m2.prefill_tokens(toks[:n - 1], 0) == n - 1
    assert_bit_equal(m2.forward(int(toks[n - 1]), n - 1), rows[n - 1], f"{what}: forward after prefill_tokens")
    for x in (m, m2):
        x.close()


# ---------------------------------------------------------------------------------------------- 3. batches

DEPTHS4 = [70, 0, 5, 33]                                       # one slot at position 0, one past a wave's 64 keys


@pytest.mark.parametrize("name,q", CASES, ids=ids(CASES))
def test_contiguous_batch_on_a_corner(L, name, q):
    """lmrs_batch_create accepts the corner; four slots at different depths: logits and argmax of every row against the slot's own oracle and the
    K/V rows the pass left, over three steps; then one forward_runs call with ragged runs (a 9-token run from position 0 among them)."""
    c = CORNERS[name]
    m, b, seqs = prefilled(L, image(name, q), c, DEPTHS4, 410)
    for s in seqs:
        check_slot_rows(b, s, sorted({0, s.n // 2, s.n - 1}) if s.n else [], f"{name} q{q}: prefill of {s.n}")
    V = c.vocab_size
    for k in range(3):
        step(b, seqs, [(13 * i + 5 * k + 3) % V for i in range(4)], f"{name} q{q} step {k}")
    work = [(s, toks_for(c, n, 420 + i), no) for i, (s, n, no) in enumerate(zip(seqs, [3, 9, 1, 6], [3, 1, 1, 0]))]
    run_pass(b, work, f"{name} q{q}: ragged runs", kv="ends")
    b.close(); m.close()


DEPTHS6 = [70, 1, 5, 33, 130, 64]


@pytest.mark.parametrize("name,q", CASES, ids=ids(CASES))
def test_wide_batch_on_a_corner(L, name, q):
    """A wide batch: a pass of 20 rows (the stream GEMM) and one of 52 (the ring kernels, q | k | v stored as one block) - logits of every row and
    the K/V row it left.  Six slots stand at depths of their own, each with its own oracle; the other rows of a pass are slots at position 0, a
    different token each, judged one after the other by ONE more oracle (an oracle per slot would cost more than the rest of the test)."""
    c = CORNERS[name]
    img = image(name, q)
    m = L.Transformer(img); b = L.Batch(m, 64, wide=True)
    assert b.width == 64
    deep = []
    for i, n in enumerate(DEPTHS6):
        s = Seq(img, i)
        toks = S.prompt_tokens(c, n, 430 + i)
        assert b.prefill(i, toks, 0) == n
        s.feed(toks); deep.append(s)
    shared = O.Oracle(img)

    def at_zero(slots):
        out = []
        for slot in slots:
            s = Seq.__new__(Seq)
            s.slot, s.orc, s.n = slot, shared, 0
            out.append(s)
        return out

    V = c.vocab_size
    step(b, deep + at_zero(range(6, 20)), [(7 * i + 2) % V for i in range(20)], f"{name} q{q}: 20 rows")
    step(b, at_zero(range(14, 37)) + deep + at_zero(range(37, 60)), [(11 * i + 1) % V for i in range(52)], f"{name} q{q}: 52 rows")
    b.close(); m.close()


def _scripted(L, m, b, c):
    """the calls of the two tests above on any batch of 24 slots -> every output, as uint32"""
    u = lambda a: np.ascontiguousarray(a).view(np.uint32).copy()
    V = c.vocab_size
    out = []
    for slot, n in enumerate([70, 0, 5, 33, 130]):
        if n:
            b.prefill(slot, S.prompt_tokens(c, n, 440 + slot), 0)
    pos = [70, 0, 5, 33, 130] + [0] * 15
    out += [u(x) for x in b.forward(list(range(20)), [(7 * i + 2) % V for i in range(20)], pos, logits=True)]
    runs = [(0, 71, toks_for(c, 3, 450), 3), (1, 1, toks_for(c, 9, 451), 1), (20, 0, toks_for(c, 70, 452), 2), (4, 131, [5], 1)]
    out += [u(x) for x in b.forward_runs(runs, k=4, logits=True)]
    for slot, at in ((0, [0, 63, 64, 70, 73]), (1, [0, 9]), (4, [0, 64, 127, 128, 131]), (20, [0, 63, 64, 69])):
        for layer in range(c.n_layers):
            out += [u(b.kv_row(slot, w, layer, p)) for p in at for w in (0, 1)]
    return out


@pytest.mark.parametrize("name,q", [(n, q) for n in PAGED for q in FORMATS], ids=ids([(n, q) for n in PAGED for q in FORMATS]))
def test_paged_batch_equals_the_wide_batch_on_a_corner(L, name, q):
    """tests/test_batch_paged.py::test_the_same_calls_on_a_wide_batch on three corners of different head size: the same calls on a paged batch of
    64-position pages give the wide batch's bits (which the test above holds against the oracle)."""
    c = CORNERS[name]
    m = L.Transformer(image(name, q))
    wide = L.Batch(m, 24, wide=True)
    want = _scripted(L, m, wide, c)
    wide.close()
    b = L.Batch(m, 24, page_len=64, n_pages=40)
    got = _scripted(L, m, b, c)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and (g == w).all(), f"{name} q{q}: output {i} of the scripted calls differs from the wide batch"
    b.close(); m.close()


def test_sampled_pass_on_the_smallest_vocabulary(L):
    """Sampling is vocabulary-side: one sampled pass on the corner whose 272 logits are less than one sort block - argmax, sample_mult and top-p rows
    - gives lmrs_forward_sample's tokens"""
    name, q = "w1024-h1024", S.Q8_0
    c = CORNERS[name]
    assert c.vocab_size == 272
    img = image(name, q)
    m = L.Transformer(img); b = L.Batch(m, 4)
    kinds = [(0.0, 0.9), (0.8, 1.0), (0.9, 0.9), (3.0, 1.0)]
    got = b.forward_sample([0, 1, 2, 3], [3, 4, 5, 6], [0] * 4, [L.Sampler(272, *kinds[i], 460 + i) for i in range(4)])
    own = L.Transformer(img)
    assert got.tolist() == [own.forward_sample(3 + i, 0, L.Sampler(272, *kinds[i], 460 + i)) for i in range(4)]
    assert int(got[0]) == ref_argmax(O.Oracle(img).forward(3, 0)), "the argmax row against the oracle"


# ---------------------------------------------------------------------------------------------- 4. the GEMMs alone

# (n, o) of the corners' launches that tests/test_verify.py and tests/test_batch_wide.py do not use: k_proj of one 64-wide kv head (o = 64), qkv of
# 16 x 64 / 1 at widths 1024, 8192 and 9216, qkv with the part-filled last tile of 32 x 96 / 1, wo of the 4096-wide corners
GEMM_SHAPES = [(1024, 64), (9216, 64), (1024, 1152), (8192, 1152), (9216, 1152), (1024, 3264), (4096, 4096)]


@pytest.mark.parametrize("q4", [False, True], ids=["q8", "q4"])
@pytest.mark.parametrize("n,o", GEMM_SHAPES)
def test_skinny_and_stream_gemms_at_the_corners_shapes(L, n, o, q4):
    rng = np.random.default_rng(3000 + n + o + int(q4))
    full = _gemm_operands(rng, n, o, 47, q4)
    ref = _gemm_reference(full[0], full[1], full[2], full[3], n, o, 47, q4)          # row t depends on token t alone
    for n_tok in (2, 9, 16):
        got = L.debug_gemm_skinny(full[0][:n_tok].copy(), full[1][:n_tok].copy(), full[2], full[3], n, o, n_tok, q4)
        assert_bit_equal(got, ref[:n_tok], f"skinny n {n} o {o} n_tok {n_tok} q4 {q4}")
    for n_tok in (20, 47):
        got = L.debug_gemm_wide(full[0][:n_tok].copy(), full[1][:n_tok].copy(), full[2], full[3], n, o, n_tok, q4)
        assert_bit_equal(got, ref[:n_tok], f"stream n {n} o {o} n_tok {n_tok} q4 {q4}")
