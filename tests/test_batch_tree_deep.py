"""Token trees (lmrs_batch_forward_tree / lmrs_batch_accept_path, lm.rs_amd/csrc/lmrs_tree.inc) where tests/test_batch_tree.py does not reach: two-layer
models of 1024 positions, one per head size (64, 96, 128, Gemma's 256); trees behind more than 256 keys - the second and later score passes of
tree_attn_kernel -, trees of depth 64 (a full anc[64], two gathered V chunks, a tree that is exactly one 64-row chunk), pages of 256 and 1024 positions
in TreeSlot, the scatter, v_load's contiguous branch and tree_commit_kernel, 512 rows in one call, and accept_path over long paths and page edges.

The reference is ONE oracle per model (reference()): fed the 1024 positions of one token run, then - on the same oracle object - the trees of PLAN in
DESCENDING order of base.  A tree at base B rewrites only oracle rows at or above B and reads rows below B and rows it has itself just written, so
every tree sees what a fresh oracle fed toks[:B] would hold.  Directly behind a tree's feed_tree its accepted path is fed again from B, then one
further token: the rows and logits accept_path and the step behind it are judged by.  Every comparison is bit for bit; no tolerances.

Oracle cost: 2015 forwards a model (1024 + 991 for the trees, their paths and the steps; test_the_reference_stays_within_its_forward_budget holds it
below 3000); reference() prints its wall time.  As measured when this module was written, on 8 CPU threads / on the 16 threads beside an MI355X:
mini-llama-1k 7.7 s / 1.6 s, mini-phi-long 15.4 s / 2.7 s, mini-llama3b-1k 12.6 s / 2.5 s, mini-gemma-1k 11.2 s / 3.1 s - 47 s / 10 s together, charged
to the four cases that call reference() first.  A case beside the GPU takes 1.6 - 3.3 s, mini-phi-long's 8.4 - 9.7 s: about 3400 kv_row reads a case, and a
key row of its 32 kv heads is 32 strided copies (lmrs_batch_debug_kv)"""
import collections
import functools
import time
import types

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from test_batch_paged_deep import config, pages_of
from test_batch_tree import feed_tree, node_tokens, path_of
from test_topk import rank_row, topk_rule
from tools import synth_lmrs as S

gpu = pytest.mark.gpu

N = 1024
SEED = 801
MODELS = ["mini-llama-1k", "mini-phi-long", "mini-llama3b-1k", "mini-gemma-1k"]          # head sizes 64, 96, 128, 256
FORMS = ["contiguous", "wide", 64, 256, 1024]
MAX_FORWARDS = 3000
NEXT_TOKEN = 17                                                                           # the token of the step behind every accepted path


def random_tree(n, seed):
    rng = np.random.default_rng(seed)
    return [None if c < 0 else int(c) for c in (rng.integers(-1, j) if j else -1 for j in range(n))]


SHAPES = {"chain64": [None] + list(range(63)), "comb64": [None if j == 0 else j - 2 + j % 2 for j in range(64)],
          "binary63": [None] + [(j - 1) // 2 for j in range(1, 63)], "star64": [None] * 64,
          "bush64": [None] + list(range(39)) + [5] * 24,                                  # a chain of 40, then 24 leaves under node 5
          "random64": random_tree(64, 9), "one": [None]}


def depth_of(parents, j):
    """0 for a root: the node is fed at base + depth, over T = base + depth + 1 keys"""
    return len(path_of(parents, j)) - 1


def deepest_path(parents):
    d = [depth_of(parents, j) for j in range(len(parents))]
    return path_of(parents, d.index(max(d)))


# (base, shape): nine trees in ONE forward_tree call, 512 rows (kRunRowsMax), slot i holds tree i
PLAN = ((960, "chain64"),    # the last node at position 1023: T = 1024 = seq_len, 64 nodes on one path
        (760, "random64"),   # T crosses 768 inside the tree, storage 760 .. 823 the 768 page edge; ancestor lists that jump
        (640, "chain64"),    # base a multiple of 64: the tree is exactly one gathered V chunk, full for the deepest node
        (505, "comb64"),     # T 506 .. 538 crosses the 512 score-pass edge, storage 505 .. 568 the 512 page edge
        (449, "chain64"),    # base = 64 k + 1: two gathered chunks (63 tree keys + 1); the deepest T = 513, one live lane in the third score pass
        (250, "binary63"),   # T reaches 256; storage 250 .. 312 crosses the 256 edge
        (191, "star64"),     # T = 192 for every node: 64 siblings at one logical position over 64 storage rows
        (0, "bush64"),       # no prefix; deep chain rows and late shallow rows in one tree
        (3, "one"))          # brings the call to 512 rows
PATHS = {"chain64": list(range(64)), "comb64": list(range(0, 64, 2)), "random64": deepest_path(SHAPES["random64"]),
         "binary63": [0, 2, 6, 14, 30, 62], "star64": [63], "bush64": [0, 1, 2, 3, 4, 5, 63], "one": [0]}


def tree_tokens(i, V):
    return node_tokens(len(SHAPES[PLAN[i][1]]), SEED + i, V)


def walk(orc, V):
    """PLAN on an oracle that holds the 1024-position run -> per tree of PLAN (feed_tree's per-node rows, the K/V rows [(layer, which)][len + 1] the
    accepted path and the step behind it leave at base .., that step's logits or None where no position is left)"""
    nl, out = orc.args.n_layers, {}
    for i in sorted(range(len(PLAN)), key=lambda i: -PLAN[i][0]):
        base, shape = PLAN[i]
        toks, path = tree_tokens(i, V), PATHS[shape]
        nodes = feed_tree(types.SimpleNamespace(orc=orc, n=base), SHAPES[shape], toks)
        for d, j in enumerate(path):
            orc.forward(int(toks[j]), base + d)
        end = base + len(path)
        nxt = orc.forward(NEXT_TOKEN, end).copy() if end < N else None
        rows = {(l, w): [orc.kv_row(w, l, p).copy() for p in range(base, min(end + 1, N))] for l in range(nl) for w in (0, 1)}
        out[i] = (nodes, rows, nxt)
    return [out[i] for i in range(len(PLAN))]


class CountingOracle:
    """what walk() asks of an oracle, counted"""

    def __init__(self, n_layers=2):
        self.args, self.forwards = types.SimpleNamespace(n_layers=n_layers), 0

    def forward(self, token, pos):
        assert 0 <= pos < N
        self.forwards += 1
        return np.zeros(1, np.float32)

    def kv_row(self, which, layer, pos):
        return np.zeros(1, np.float32)


Ref = collections.namedtuple("Ref", "cfg img toks K V trees seconds")


@functools.lru_cache(maxsize=None)
def reference(name):
    """One oracle over positions 0 .. 1023 of one seeded token run, its K and V rows [layers, N, kv_dim]; then walk() on the same oracle.  Read-only."""
    c = config(name)
    img = S.build_image(c, S.Q8_0, seed=SEED)
    toks = S.prompt_tokens(c, N, SEED)
    orc = O.Oracle(img)
    t0 = time.time()
    for p in range(N):
        orc.forward(int(toks[p]), p)
    kv = [np.stack([np.stack([orc.kv_row(w, l, p) for p in range(N)]) for l in range(c.n_layers)]) for w in (0, 1)]
    trees = walk(orc, c.vocab_size)
    seconds = time.time() - t0
    print(f"\noracle: {name}, {c.n_layers} layers: {N} sequential steps and the nine trees in {seconds:.1f} s")
    for a in (toks, kv[0], kv[1]):
        a.setflags(write=False)
    return Ref(c, img, toks, kv[0], kv[1], trees, seconds)


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


# ---------------------------------------------------------------------------------------------- CPU tier: what the plan claims

def logical_T(i):
    base, shape = PLAN[i]
    return [base + depth_of(SHAPES[shape], j) + 1 for j in range(len(SHAPES[shape]))]


def storage(i):
    base, shape = PLAN[i]
    return list(range(base, base + len(SHAPES[shape])))


def test_the_plan_reaches_what_it_claims():
    by_base = {base: i for i, (base, _) in enumerate(PLAN)}
    assert len(by_base) == len(PLAN) == 9, "the bases are distinct"
    assert sum(len(SHAPES[s]) for _, s in PLAN) == 512, "kRunRowsMax exactly"
    assert all(base + len(SHAPES[s]) <= N for base, s in PLAN)
    for shape, par in SHAPES.items():
        assert all(p is None or 0 <= p < j for j, p in enumerate(par)), shape
        assert PATHS[shape] == path_of(par, PATHS[shape][-1]), f"{shape}: the accepted path is a root-to-node path"
    r = SHAPES["random64"]
    assert sum(p is None for p in r) >= 3 and max(depth_of(r, j) for j in range(64)) >= 8 and max(j - p for j, p in enumerate(r) if p is not None) >= 20
    T, st = {b: logical_T(i) for b, i in by_base.items()}, {b: storage(i) for b, i in by_base.items()}
    assert max(T[960]) == 1024 == N and st[960][-1] == 1023 and len(path_of(SHAPES["chain64"], 63)) == 64
    assert min(T[760]) <= 768 < max(T[760]) and 767 in st[760] and 768 in st[760]
    assert 640 % 64 == 0 and max(T[640]) == 704 and st[640] == list(range(640, 704))
    assert min(T[505]) == 506 and max(T[505]) == 538 and {512, 513} <= set(T[505]) and {511, 512} <= set(st[505])
    assert 449 % 64 == 1 and max(T[449]) == 513
    assert max(T[250]) == 256 and {255, 256} <= set(st[250]) and st[250][-1] == 312
    assert set(T[191]) == {192} and st[191] == list(range(191, 255))
    assert st[0][0] == 0 and max(T[0]) == 40 and T[0][-1] == 7
    assert len(PATHS["comb64"]) == 32 and 505 + 31 > 512 > 505, "the comb's spine moves across 512"
    # every later 256-key score pass of tree_attn_kernel is entered by some node, with one live lane (257 is no T of the plan: 513 is) and with many
    all_T = {t for i in range(9) for t in logical_T(i)}
    assert 513 in all_T and any(256 < t <= 512 for t in all_T) and any(512 < t <= 768 for t in all_T) and any(768 < t for t in all_T)


def test_the_reference_stays_within_its_forward_budget():
    orc = CountingOracle()
    walk(orc, 1000)
    assert N + orc.forwards <= MAX_FORWARDS, f"{N} + {orc.forwards} oracle forwards a model"


# ---------------------------------------------------------------------------------------------- GPU tier

def make_batch(L, m, form):
    """nine slots, one a tree; the paged forms hold a tenth for the fork and a pool that could take every slot to full depth"""
    if form in ("contiguous", "wide"):
        return L.Batch(m, 9, wide=form == "wide")
    return L.Batch(m, 10, page_len=form, n_pages=10 * pages_of(N, form))


KV = [(l, w) for l in range(2) for w in (0, 1)]
FORK_OF, FORK_SLOT = 3, 9                                 # the comb at 505: its spine moves into positions of the page below 512


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MODELS)
def test_nine_trees_in_one_call_and_their_accepted_paths(L, name, form):
    """PLAN in one forward_tree call: every node's argmax, logits and K/V rows of both layers at base + node (mini-llama-1k: with the top-5 outputs);
    then accept_path for all nine slots in one call, the moved rows, the rows below the bases, and one forward over the slots behind their paths"""
    ref = reference(name)
    k = 5 if name == MODELS[0] else 0
    what = f"{name} {form}"
    m = L.Transformer(ref.img)
    assert m.args.seq_len == N and m.args.n_layers == 2
    V, paged = m.args.vocab_size, form not in ("contiguous", "wide")
    b = make_batch(L, m, form)
    for i, (base, _) in enumerate(PLAN):
        if base:
            assert b.prefill(i, ref.toks[:base], 0) == base
    got = b.forward_tree([(i, base, SHAPES[shape], tree_tokens(i, V)) for i, (base, shape) in enumerate(PLAN)], k=k, logits=True)
    am, lg = got[0], got[1]
    assert am.shape == (512,)
    r = 0
    for i, (base, shape) in enumerate(PLAN):
        for j, (want, rows) in enumerate(ref.trees[i][0]):
            w = f"{what}: {shape} at {base}, node {j}"
            assert int(am[r]) == ref_argmax(want), f"{w}: argmax"
            assert_bit_equal(lg[r], want, f"{w}: logits")
            for x, (l, kv) in zip(rows, KV):
                assert_bit_equal(b.kv_row(i, kv, l, base + j), x, f"{w}: {'kv'[kv]} row of layer {l} at storage position {base + j}")
            if k:
                assert got[2][r].tolist() == rank_row(want)[:k].tolist(), f"{w}: top-{k} candidates"
            r += 1
    if k:
        topk_rule(got[3], got[2], np.stack([w for t in ref.trees for w, _ in t[0]]), what)

    def below(when):
        for i, (base, _) in enumerate(PLAN):
            for p in sorted({0, base - 1}) if base else []:
                for l, kv in KV:
                    assert_bit_equal(b.kv_row(i, kv, l, p), (ref.K, ref.V)[kv][l, p], f"{what}: slot {i} {'kv'[kv]} layer {l} pos {p} {when}")

    below("after the tree pass")
    if paged:
        at = [PLAN[FORK_OF][0] + j for j in (0, 1, 2, 6, 7, 8, 31, 32, 62, 63)]   # sources, destinations on both sides of 512, rows that stay
        b.fork(FORK_OF, FORK_SLOT, at[-1] + 1)
        stored = [b.kv_row(FORK_SLOT, kv, l, p).copy() for l, kv in KV for p in at]
    b.accept_path([(i, base, PATHS[shape]) for i, (base, shape) in enumerate(PLAN)])
    for i, (base, shape) in enumerate(PLAN):
        for l, kv in KV:
            for d in range(len(PATHS[shape])):
                assert_bit_equal(b.kv_row(i, kv, l, base + d), ref.trees[i][1][l, kv][d], f"{what}: {shape} at {base} after accept_path: {'kv'[kv]} layer {l} pos {base + d}")
    below("after accept_path")
    live = [i for i, (base, shape) in enumerate(PLAN) if base + len(PATHS[shape]) < N]
    assert live == list(range(1, 9))
    ends = [PLAN[i][0] + len(PATHS[PLAN[i][1]]) for i in live]
    am, lg = b.forward(live, [NEXT_TOKEN] * len(live), ends, logits=True)
    for n, (i, end) in enumerate(zip(live, ends)):
        want = ref.trees[i][2]
        assert_bit_equal(lg[n], want, f"{what}: slot {i}: the step at {end} behind the accepted path")
        assert int(am[n]) == ref_argmax(want)
        for l, kv in KV:
            assert_bit_equal(b.kv_row(i, kv, l, end), ref.trees[i][1][l, kv][-1], f"{what}: slot {i}: {'kv'[kv]} layer {l} written at {end}")
    if paged:
        for x, y in zip(stored, [b.kv_row(FORK_SLOT, kv, l, p) for l, kv in KV for p in at]):
            assert_bit_equal(y, x, f"{what}: the fork taken between the tree pass and accept_path keeps the rows as stored")
        for slot in range(10):
            b.release(slot)
        assert b.pages()[2] == b.pages()[1], f"{what}: pages lost"
    b.close(); m.close()
