"""The split attention form with its scores inside the qkv launch (launch_qkv_scores: five launches per layer instead of six), run with
`-m gpu` on an MI355X against the CPU oracle, on `uint32` views: the (head, 256-key chunk) score items poll q - and, in the chunk that
receives the new key, the raw key - from the {value, tag} granules the GEMV workgroups of the same launch publish.  The split position
is lowered to 4 at create, so mini models reach the form at once; one oracle run per model is shared by the tests that need it."""
import dataclasses
import functools

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, bits
from tools import synth_lmrs as S

pytestmark = pytest.mark.gpu

SPLIT_POS = 4
# the 128-wide and the 256-wide (Gemma-2) mini with a context that holds three 256-key chunks, and the 128-wide one past the 2048 positions from which
# the launch no longer fits the resident slots
LONG = {"mini-llama3b-long": dataclasses.replace(S.CONFIGS["mini-llama3b"], name="mini-llama3b-long", max_pos=1024),
        "mini-gemma-long": dataclasses.replace(S.CONFIGS["mini-gemma"], name="mini-gemma-long", max_pos=1024),
        "mini-llama3b-deep": dataclasses.replace(S.CONFIGS["mini-llama3b"], name="mini-llama3b-deep", max_pos=2304)}


def config(name):
    return LONG.get(name) or S.CONFIGS[name]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


@functools.lru_cache(maxsize=None)
def reference(cfg, q, n):
    """The oracle over positions 0 .. n-1 of one seeded token run: (image, tokens, logits [n, vocab], K rows and V rows [layers, n, kv_dim]), read-only."""
    img = S.build_image(config(cfg), q, seed=61)
    toks = S.prompt_tokens(config(cfg), n, 61)
    orc = O.Oracle(img)
    logits = np.stack([orc.forward(int(toks[p]), p).copy() for p in range(n)])
    nl = config(cfg).n_layers
    kv =[np.stack([np.stack([orc.kv_row(w, l, p) for p in range(n)]) for l in range(nl)]) for w in (0, 1)]
    for a in (logits, kv[0], kv[1]):
        a.setflags(write=False)
    return img, toks, logits, kv[0], kv[1]


def run_positions(m, toks, positions):
    return np.stack([m.forward(int(toks[p]), p).copy() for p in positions])


def first_diff(a, b):
    d = np.flatnonzero((bits(a) != bits(b)).reshape(len(a), -1).any(axis=1))
    return int(d[0]) if d.size else None


def assert_steps_equal(got, want, positions, what):
    d = first_diff(got, want)
    assert d is None, f"{what}: logits differ first at position {positions[d]}"


def assert_caches_equal(m, K, V, lo, hi, what):
    for l in range(K.shape[0]):
        for p in range(lo, hi):
            assert_bit_equal(m.kv_row(0, l, p), K[l, p], f"{what}: key row, layer {l} position {p}")
            assert_bit_equal(m.kv_row(1, l, p), V[l, p], f"{what}: value row, layer {l} position {p}")


def merged_context(L, monkeypatch, img, **env):
    monkeypatch.setenv("LMRS_ATT_SPLIT_POS", str(SPLIT_POS))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    m = L.Transformer(img)
    nl = m.args.n_layers
    assert m.step_info(SPLIT_POS)[0] == 5 * nl + 1, f"the merged qkv + scores launch is not in use ({m.step_info(SPLIT_POS)[0]} launches per step)"
    return m


def test_chunk_boundaries(L, monkeypatch):
    """Mini Llama (64-wide heads, 2048 positions), positions 0 .. 530: the logits of every step and the K / V rows of positions 4 .. 530 - across the
    256- and 512-key chunk boundaries, with the new key's chunk moving from the first to the third."""
    n = 531
    img, toks, logits, K, V = reference("mini-llama-long", S.Q8_0, n)
    m = merged_context(L, monkeypatch, img)
    assert_steps_equal(run_positions(m, toks, range(n)), logits, list(range(n)), "mini-llama-long")
    assert_caches_equal(m, K, V, SPLIT_POS, n, "mini-llama-long")


@pytest.mark.parametrize("cfg,q,n", [("mini-llama3b-long", S.Q8_0, 531), ("mini-gemma-long", S.Q8_0, 531), ("mini-llama-long", S.Q4_0, 531),
                                     ("mini-phi-long", S.Q8_0, 300)])
def test_other_shapes(L, monkeypatch, cfg, q, n):
    """test_chunk_boundaries on the other classes: 128-wide heads, Gemma-2 (256-wide heads: the new key's later batches come back from memory, also in a
    chunk other than the first; soft-cap and window; the folded norm + add prologue) and a Q4_0 file, each over positions 0 .. 530 - chunks 1 and 2 poll q
    alone, the new key moves from chunk to chunk - and Phi's 96-wide heads past the first boundary."""
    img, toks, logits, K, V = reference(cfg, q, n)
    m = merged_context(L, monkeypatch, img)
    assert_steps_equal(run_positions(m, toks, range(n)), logits, list(range(n)), cfg)
    assert_caches_equal(m, K, V, SPLIT_POS, n, cfg)


def test_old_and_new_forms_agree(L, monkeypatch):
    """Two contexts of one image, the second with LMRS_ATT_SPLIT_MERGED=0 (plain qkv, score launch, value launch): bit-equal logits at every step and
    bit-equal caches."""
    n = 531
    img, toks, logits, K, V = reference("mini-llama-long", S.Q8_0, n)
    new = merged_context(L, monkeypatch, img)
    monkeypatch.setenv("LMRS_ATT_SPLIT_MERGED", "0")
    old = L.Transformer(img)
    assert old.step_info(SPLIT_POS)[0] == 6 * old.args.n_layers + 1
    a = run_positions(new, toks, range(n)); b = run_positions(old, toks, range(n))
    assert_steps_equal(a, b, list(range(n)), "six launches against five")
    assert_steps_equal(b, logits, list(range(n)), "six launches against the oracle")
    for l in range(K.shape[0]):
        for p in range(n):
            for w in (0, 1):
                assert_bit_equal(new.kv_row(w, l, p), old.kv_row(w, l, p), f"cache {w}, layer {l} position {p}")


def test_tags_never_repeat(L, monkeypatch):
    """Positions re-run out of order (the granules of a layer still hold an earlier step's values: only the tag tells them apart), across the switches
    between the forms: the wave form below the split position, the merged split form above it, and the separate kernels of a one-token fill_kv_cache -
    which bump the same step counter - in between."""
    n = 531
    img, toks, logits, K, V = reference("mini-llama-long", S.Q8_0, n)
    m = merged_context(L, monkeypatch, img)
    run_positions(m, toks, range(n))
    emb = m.get_embeddings(toks)
    dim = m.args.dim
    order = [5, 300, 2, 4, 256, 255, 3, 511, 512, 6, 0, 520, 257, 530]
    for i, p in enumerate(order):
        if i % 3 == 1:                                         # a layers-only step of the separate kernels at a position of its own
            e = emb[(p + 7) * dim: (p + 8) * dim].copy() if p + 8 <= n else emb[:dim].copy()
            fp = p + 7 if p + 8 <= n else 0
            assert m.fill_kv_cache(e, fp) == fp + 1
        assert_bit_equal(m.forward(int(toks[p]), p), logits[p], f"logits at re-run position {p}")
    assert_caches_equal(m, K, V, SPLIT_POS, n, "after the re-runs")


@pytest.mark.parametrize("cfg,q,n,wgs", [("mini-llama-long", S.Q8_0, 531, 3), ("mini-gemma-long", S.Q8_0, 531, 5)])
def test_capped_grid(L, monkeypatch, cfg, q, n, wgs):
    """LMRS_ATT_SPLIT_SCORE_WGS limits the score workgroups of the launch: each walks several (head, chunk) items (32 heads x 3 chunks over 3 workgroups;
    8 heads x 3 chunks over 5), reusing its LDS vectors.  Bit-equal steps and caches; a bounded poll that gave up would fail the call (the error word)."""
    img, toks, logits, K, V = reference(cfg, q, n)
    m = merged_context(L, monkeypatch, img, LMRS_ATT_SPLIT_SCORE_WGS=wgs)
    assert_steps_equal(run_positions(m, toks, range(n)), logits, list(range(n)), f"{cfg}, {wgs} score workgroups")
    assert_caches_equal(m, K, V, SPLIT_POS, n, f"{cfg}, {wgs} score workgroups")


def test_launch_larger_than_the_resident_slots(L, monkeypatch):
    """Positions 2100 .. 2103 of the 128-wide mini: the graph's bucket holds 16 chunks, so 24 x 16 score workgroups and the GEMV workgroups no longer fit
    the slots resident at once and launch_qkv_scores caps both parts (the score part at its floor, the GEMV part at the rest; the 24 x 9 items that
    exist are walked by fewer workgroups).  The cache below is filled by fill_kv_cache; logits and the new cache rows against the oracle."""
    first, n = 2100, 4
    img, toks, logits, K, V = reference("mini-llama3b-deep", S.Q8_0, first + n)
    m = merged_context(L, monkeypatch, img)
    assert m.step_info(first)[0] == 5 * m.args.n_layers + 1
    assert m.fill_kv_cache(m.get_embeddings(toks[:first]), 0) == first
    positions = list(range(first, first + n))
    assert_steps_equal(run_positions(m, toks, positions), logits[first:], positions, "mini-llama3b-deep")
    assert_caches_equal(m, K, V, first - 2, first + n, "mini-llama3b-deep")
