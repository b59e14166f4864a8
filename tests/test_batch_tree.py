"""lmrs_batch_forward_tree / lmrs_batch_accept_path (include/lmrs_hip.h): token trees in one weight pass.  The reference is the slot's CPU oracle fed every
node's root-to-node path token by token behind the slot's prefix (Transformer::forward reads positions <= pos only, so one oracle that holds the prefix
serves every path: the positions from the paths' common part on are fed again).  Every comparison - argmax, logits, K/V rows - is bit for bit."""
import functools

import numpy as np
import pytest

import filter_rules as F
from parity_rules import assert_bit_equal, ref_argmax
from test_batch import CFGS, DEPTHS16, Seq, check_slot_rows, step
from test_batch_mask import masked
from test_topk import rank_row, topk_rule
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
KINDS = ["contiguous", "wide", "paged"]
SHAPES = {"chain7": [None] + list(range(6)), "star8": [None] * 8, "binary15": [None] + [(j - 1) // 2 for j in range(1, 15)],
          "comb20": [None if j == 0 else j - 2 + j % 2 for j in range(20)],          # spine 0, 2, 4, .. with the leaf 2i + 1 under spine node 2i
          "comb64": [None if j == 0 else j - 2 + j % 2 for j in range(64)], "one": [None], "star64": [None] * 64,
          "chain7+1": [None] + list(range(6)) + [None]}                              # a chain and a second root behind it


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def batch_of(L, m, kind, n_slots, n_pages=32, **kw):
    return L.Batch(m, n_slots, page_len=64, n_pages=n_pages, **kw) if kind == "paged" else L.Batch(m, n_slots, wide=kind == "wide")


def path_of(parents, j):
    return path_of(parents, parents[j]) + [j] if j is not None else []


def node_tokens(n, seed, V):
    return [(seed * 131 + j * 37 + 11) % V for j in range(n)]


def feed_tree(s, parents, tokens):
    """every node's path through s's oracle, which holds the prefix (s.n tokens) -> per node (logits, the K/V rows of every layer at s.n + depth)"""
    cur, out, nl = [], [], s.orc.args.n_layers
    for j in range(len(parents)):
        path = path_of(parents, j)
        same = next(d for d in range(len(path)) if d >= len(cur) or cur[d] != path[d])
        for d in range(same, len(path)):
            lg = s.orc.forward(int(tokens[path[d]]), s.n + d).copy()
        cur, p = path, s.n + len(path) - 1
        out.append((lg, [s.orc.kv_row(w, l, p).copy() for l in range(nl) for w in (0, 1)]))
    return out


@functools.lru_cache(maxsize=None)
def plan_reference(cfg, q, plan, seed):
    """image, and per (shape, base) of the plan: prefix tokens, node tokens, feed_tree's rows - computed once and shared by the batch kinds"""
    img = S.build_image(cfg, q, seed=seed)
    out = []
    for i, (shape, base) in enumerate(plan):
        s = Seq(img, i)
        prefix = S.prompt_tokens(cfg, base, seed + 1 + i) if base else []
        s.feed(prefix)
        toks = node_tokens(len(SHAPES[shape]), seed + i, s.orc.args.vocab_size)
        out.append((prefix, toks, feed_tree(s, SHAPES[shape], toks)))
    return img, out


def run_plan(L, kind, cfg, q, plan, seed, k=0, n_pages=32):
    """the plan's trees in ONE call on a batch of `kind`, every node judged against plan_reference -> (model, batch, reference)"""
    img, ref = plan_reference(cfg, q, plan, seed)
    m = L.Transformer(img); b = batch_of(L, m, kind, len(plan), n_pages)
    for i, (prefix, _, _) in enumerate(ref):
        if len(prefix):
            b.prefill(i, prefix, 0)
    got = b.forward_tree([(i, base, SHAPES[shape], ref[i][1]) for i, (shape, base) in enumerate(plan)], k=k, logits=True)
    am, lg = got[0], got[1]
    nl, r = m.args.n_layers, 0
    for i, (shape, base) in enumerate(plan):
        for j, (want, rows) in enumerate(ref[i][2]):
            what = f"{cfg} q{q} {kind}: {shape} at {base}, node {j}"
            assert int(am[r]) == ref_argmax(want), f"{what}: argmax"
            assert_bit_equal(lg[r], want, f"{what}: logits")
            for x, (l, w) in zip(rows, [(l, w) for l in range(nl) for w in (0, 1)]):
                assert_bit_equal(b.kv_row(i, w, l, base + j), x, f"{what}: {'kv'[w]} row of layer {l} at storage position {base + j}")
            if k:
                assert got[2][r].tolist() == rank_row(want)[:k].tolist(), f"{what}: top-{k} candidates"
            r += 1
    if k:
        topk_rule(got[3], got[2], np.stack([w for e in ref for w, _ in e[2]]), f"{cfg} {kind}")
    return m, b, ref


# bases: 0; 61 - the logical T crosses the 64-key chunk inside the tree; 64; 50 with the comb - storage 50 .. 69 crosses a page and chunk edge, the logical T
# stays at 61 or below; 241 - the last node at the model's last position (256 positions)
PLAN = (("chain7", 0), ("binary15", 61), ("star8", 64), ("comb20", 50), ("binary15", 241), ("star8", 0))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg,q", CFGS)
def test_trees_against_path_oracles(L, cfg, q, kind):
    m, b, ref = run_plan(L, kind, cfg, q, PLAN, 301)
    twin = L.Batch(m, 1)                                  # the chain is a run: forward_runs' bits on a twin batch
    am, lg = twin.forward_runs([(0, 0, ref[0][1], 7)], logits=True)
    for j, (want, rows) in enumerate(ref[0][2]):
        assert int(am[j]) == ref_argmax(want)
        assert_bit_equal(lg[j], want, f"{cfg} q{q}: forward_runs row {j}")
        assert_bit_equal(twin.kv_row(0, 0, 0, j), rows[0], f"{cfg} q{q}: forward_runs k row {j}")


@gpu
@pytest.mark.parametrize("kind,k", [("contiguous", 0), ("paged", 0), ("wide", 5)])
def test_a_64_node_tree_behind_300_positions(L, kind, k):
    """mini-llama-long: the prefix takes more than one 256-key score pass, the comb's logical keys 300 .. 332 span two value chunks and its storage
    300 .. 363 a page edge; 15 single-node trees of other slots make R = 79 rows - the ring GEMMs"""
    run_plan(L, kind, "mini-llama-long", S.Q8_0, (("comb64", 300),) + (("one", 0),) * 15, 311, k=k, n_pages=24)


# (parents, path): a destination that is an earlier source; a path with gaps; a chain that lies where it was stored
ACCEPT = (([None, None, 1], [1, 2], 62), ([None, 0, 0, 0, 1, 1, 2, 2, 3, 3], [0, 3, 9], 10), ([None, 0, 1, 2], [0, 1, 2], 0))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_accept_path(L, kind):
    cfg, q = "mini-llama", S.Q8_0
    img = S.build_image(cfg, q, seed=321)
    m = L.Transformer(img); b = batch_of(L, m, kind, 5)
    seqs, V, nl = [Seq(img, i) for i in range(3)], m.args.vocab_size, m.args.n_layers
    for s, (_, _, base) in zip(seqs, ACCEPT):
        if base:
            toks = S.prompt_tokens(cfg, base, 322 + s.slot)
            b.prefill(s.slot, toks, 0); s.feed(toks)
    if kind == "paged":
        b.fork(0, 3, 62)                                  # slot 3 shares slot 0's first page: the tree pass must un-share it
    below = [b.kv_row(0, w, l, p).copy() for l in range(nl) for w in (0, 1) for p in (0, 61)]
    toks = [node_tokens(len(par), 323 + i, V) for i, (par, _, _) in enumerate(ACCEPT)]
    b.forward_tree([(i, base, par, toks[i]) for i, (par, _, base) in enumerate(ACCEPT)])
    if kind == "paged":
        b.fork(1, 4, 20)                                  # slot 4 shares the page slot 1's tree is stored in: accept_path's own writes must un-share it
        stored = [b.kv_row(4, w, l, p).copy() for l in range(nl) for w in (0, 1) for p in range(10, 20)]
    b.accept_path([(i, base, path) for i, (_, path, base) in enumerate(ACCEPT)])
    for s, (_, path, base), t in zip(seqs, ACCEPT, toks):
        s.feed([t[j] for j in path])                      # the oracle takes the accepted path
        check_slot_rows(b, s, range(base, base + len(path)), f"{kind}: after accept_path {path}")
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in
               zip(below, [b.kv_row(0, w, l, p) for l in range(nl) for w in (0, 1) for p in (0, 61)])), "positions below the base changed"
    step(b, seqs, [5, 6, 7], f"{kind}: forward after accept_path")
    am, lg = b.forward_runs([(s.slot, s.n, [8 + s.slot, 9], 2) for s in seqs], logits=True)
    for i, s in enumerate(seqs):
        for j, t in enumerate([8 + s.slot, 9]):
            assert_bit_equal(lg[2 * i + j], s.feed([t]), f"{kind}: forward_runs after accept_path, slot {s.slot} row {j}")
    if kind == "paged":
        orc0 = Seq(img, 3); orc0.feed(S.prompt_tokens(cfg, 62, 322))
        check_slot_rows(b, orc0, [0, 31, 61], "the fork taken before the tree pass")
        for x, y in zip(stored, [b.kv_row(4, w, l, p) for l in range(nl) for w in (0, 1) for p in range(10, 20)]):
            assert_bit_equal(y, x, "the fork taken between the tree pass and accept_path keeps the rows as stored")
        for slot in range(5):
            b.release(slot)
        assert b.pages()[2] == b.pages()[1], "pages lost"


@gpu
@pytest.mark.parametrize("kind", ["contiguous", "paged"])
@pytest.mark.parametrize("cfg,q", CFGS)
def test_accept_a_path_of_20_nodes_on_every_geometry(L, cfg, q, kind):
    """every head size and kv width of the [layer][kv head][hs / 4][positions][4] K layout through tree_commit_kernel: the first 20 spine nodes of a
    comb at 50 - sources 50 .. 88, destinations 50 .. 69, both across the page edge at 64 - then a step that reads every moved row"""
    img = S.build_image(cfg, q, seed=361)
    m = L.Transformer(img); b = batch_of(L, m, kind, 1); s = Seq(img, 0)
    base, path = 50, list(range(0, 40, 2))
    prefix, toks = S.prompt_tokens(cfg, base, 362), node_tokens(64, 363, m.args.vocab_size)
    b.prefill(0, prefix, 0); s.feed(prefix)
    b.forward_tree([(0, base, SHAPES["comb64"], toks)])
    b.accept_path([(0, base, path)])
    s.feed([toks[j] for j in path])
    check_slot_rows(b, s, range(base, base + 20), f"{cfg} q{q} {kind}: after accept_path of 20 nodes")
    check_slot_rows(b, s, [0, base - 1], f"{cfg} q{q} {kind}: below the base")
    step(b, [s], [5], f"{cfg} q{q} {kind}: forward after accept_path of 20 nodes")


def check_nodes(b, slot, base, nodes, am, lg, r, what):
    """rows r .. of a forward_tree call against feed_tree's nodes: argmax, logits and the K/V rows of every layer at base + node -> the next row"""
    for j, (want, rows) in enumerate(nodes):
        assert int(am[r]) == ref_argmax(want), f"{what}, node {j}: argmax"
        assert_bit_equal(lg[r], want, f"{what}, node {j}: logits")
        for n, x in enumerate(rows):
            assert_bit_equal(b.kv_row(slot, n % 2, n // 2, base + j), x, f"{what}, node {j}: {'kv'[n % 2]} row of layer {n // 2} at storage position {base + j}")
        r += 1
    return r


@gpu
@pytest.mark.parametrize("kind", ["contiguous", "paged"])
def test_drafting_again_at_the_same_base(L, kind):
    """star64 at 70, then - no accept between - a chain7 of other tokens at 70, then a binary15: the smaller trees' gathered V chunk (64 .. 127) still
    holds the star's rows 77 .. 133 behind its last key, where tree_gload's clamp reads; nothing of them may reach a node"""
    cfg, q, base = "mini-llama", S.Q8_0, 70
    img = S.build_image(cfg, q, seed=371)
    m = L.Transformer(img); b = batch_of(L, m, kind, 1); s = Seq(img, 0)
    prefix = S.prompt_tokens(cfg, base, 372)
    b.prefill(0, prefix, 0); s.feed(prefix)
    for n, shape in enumerate(("star64", "chain7", "binary15")):
        toks = node_tokens(len(SHAPES[shape]), 373 + n, m.args.vocab_size)
        am, lg = b.forward_tree([(0, base, SHAPES[shape], toks)], logits=True)
        assert check_nodes(b, 0, base, feed_tree(s, SHAPES[shape], toks), am, lg, 0, f"{kind}: {shape} at {base}, pass {n}") == len(toks)
    check_slot_rows(b, s, [0, base - 1], f"{kind}: below the base")


WIDE_DEPTHS = [DEPTHS16[i] for i in (0, 3, 4, 8, 9)] + [248]                          # 0, 63, 64, 129, 200; 248: the last node at the last position


@gpu
def test_64_trees_fill_a_wide_batch(L):
    """a wide batch at its width and the call at kRunRowsMax: 64 trees of 8 nodes (star8 and chain7 + 1 by turns), slots in shuffled order, 512 rows.
    The slots of a depth are forks of one prompt, so one oracle a depth serves them: feed_tree feeds every tree from the base again"""
    cfg, q = "mini-llama", S.Q8_0
    img = S.build_image(cfg, q, seed=381)
    m = L.Transformer(img); b = L.Batch(m, 64, wide=True)
    V, first, orcs = m.args.vocab_size, {}, {}
    for slot in range(64):
        d = WIDE_DEPTHS[slot % len(WIDE_DEPTHS)]
        if d not in first:
            first[d], orcs[d] = slot, Seq(img, slot)
            if d:
                prefix = S.prompt_tokens(cfg, d, 382 + d)
                b.prefill(slot, prefix, 0); orcs[d].feed(prefix)
        elif d:
            b.fork(first[d], slot, d)
    order = [int(x) for x in np.random.default_rng(383).permutation(64)]
    trees = [(slot, WIDE_DEPTHS[slot % len(WIDE_DEPTHS)], SHAPES[("star8", "chain7+1")[(slot // len(WIDE_DEPTHS) + slot) % 2]], node_tokens(8, 384 + slot, V)) for slot in order]
    am, lg = b.forward_tree(trees, logits=True)
    assert am.shape == (512,)
    r = 0
    for slot, d, par, toks in trees:
        r = check_nodes(b, slot, d, feed_tree(orcs[d], par, toks), am, lg, r, f"wide: slot {slot} at {d}")
    assert r == 512


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_tree_speculative_greedy_equals_greedy(L, kind):
    """Per step a tree from the greedy continuation itself: the right token and a wrong sibling at each of 4 depths (step 2: the wrong one first, so the
    right branch is the sibling; steps 1, 4, ..: both tokens wrong at depth 2, so 2 nodes are accepted) - driven by tree_accept + accept_path"""
    cfg, q, n_new = "mini-llama", S.Q8_0, 24
    img = S.build_image(cfg, q, seed=331)
    m = L.Transformer(img); b = batch_of(L, m, kind, 2); twin = L.Batch(m, 2)
    prompts, V = [S.prompt_tokens(cfg, n, 332 + i) for i, n in enumerate((9, 60))], m.args.vocab_size
    for bb in (b, twin):
        for i, p in enumerate(prompts):
            bb.prefill(i, p[:-1], 0)
    truth = twin.generate_greedy([0, 1], [p[-1] for p in prompts], [len(p) - 1 for p in prompts], n_new + 8)
    first = b.forward([0, 1], [p[-1] for p in prompts], [len(p) - 1 for p in prompts])
    out, pos, lens = [[int(first[i])] for i in range(2)], [len(p) for p in prompts], []
    for stp in range(8):
        trees = []
        for i in range(2):
            g = [int(x) for x in truth[i][len(out[i]) - 1:len(out[i]) + 3]]            # the tokens greedy decoding feeds next
            par, tok = [], []
            for d in range(4):
                pair = [(g[d] + 1) % V, (g[d] + 2) % V] if d >= 2 and stp % 3 == 1 else [g[d], (g[d] + 1) % V]
                par += [None if d == 0 else len(par) - 2 + (stp == 2)] * 2             # under the right node of the depth above
                tok += pair[::-1] if stp == 2 else pair
            trees.append((i, pos[i], par, tok))
        am = b.forward_tree(trees)
        paths = []
        for i, (_, p, par, tok) in enumerate(trees):
            path, nxt = L.tree_accept(par, tok, am[8 * i:8 * i + 8], out[i][-1])
            out[i] += [int(am[8 * i + j]) for j in path]
            assert nxt == out[i][-1]
            paths.append((i, p, path)); pos[i] += len(path)
        b.accept_path(paths)
        lens.append([len(p[2]) for p in paths])
    assert lens == [[2, 2] if stp % 3 == 1 else [4, 4] for stp in range(8)], lens
    for i in range(2):
        assert out[i][:n_new] == truth[i][:n_new].tolist(), f"{kind}: slot {i}"


@gpu
def test_refusals(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=341)
    m = L.Transformer(img); b = L.Batch(m, 9); s = Seq(img, 0)
    b.set_penalties([1], repetition=1.3)
    b.attach([2], b.automaton(L.TokenAutomaton(np.zeros(m.args.vocab_size, np.uint16), [[0]])))
    for trees, msg in [
            ([(0, 0, [None] * 65, [1] * 65)], r"tree 0: n_nodes = 65 is outside 1 \.\. 64"), ([(0, 0, [], [])], r"n_nodes = 0 is outside"),
            ([(i, 0, [None] * 64, [1] * 64) for i in range(9)], "the trees hold more than 512 nodes"),
            ([(0, 0, [None, 1], [1, 2])], r"parent\[1\] = 1 is neither LMRS_TREE_ROOT nor below its own index"),
            ([(0, 250, [None] * 7, [1] * 7)], r"start_pos \+ n_nodes exceeds seq_len"),
            ([(0, 0, [None], [1]), (0, 3, [None], [1])], "slot 0 appears in more than one tree"),
            ([(1, 0, [None], [1])], "slot 1 has penalties set"), ([(2, 0, [None], [1])], "slot 2 has an automaton attached")]:
        with pytest.raises(L.LmrsError, match="lmrs_batch_forward_tree: .*" + msg):
            b.forward_tree(trees)
    for paths, msg in [([(0, 0, [1, 1])], "path is not strictly ascending at 1"), ([(0, 250, [3, 6])], "lies outside seq_len"), ([(0, 0, [64])], "is no node index")]:
        with pytest.raises(L.LmrsError, match="lmrs_batch_accept_path: .*" + msg):
            b.accept_path(paths)
    for kv in ("q8", "q4"):
        pool = L.Batch(m, 1, page_len=64, n_pages=4, kv=kv)
        with pytest.raises(L.LmrsError, match=f"lmrs_batch_forward_tree: token trees over a {kv.upper()} page pool are not built yet"):
            pool.forward_tree([(0, 0, [None], [1])])
        with pytest.raises(L.LmrsError, match=f"lmrs_batch_accept_path: token trees over a {kv.upper()} page pool are not built yet"):
            pool.accept_path([(0, 0, [1])])
    am, lg = b.forward_tree([(0, 0, [None, 0], [3, 4])], logits=True)                # the batch serves a valid call after all of them
    assert_bit_equal(lg[1], s.feed([3, 4]), "a valid tree after the refusals")


@gpu
def test_masks_and_filters_apply_to_every_node(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=351)
    m = L.Transformer(img); b = L.Batch(m, 2)
    V, par, tok = m.args.vocab_size, [None, 0, None], [21, 22, 23]
    want = [feed_tree(Seq(img, i), par, tok) for i in range(2)]
    mask = np.ones(V, bool); mask[[ref_argmax(w) for w, _ in want[0]]] = False        # ban what every node would pick
    b.set_masks([0], mask[None]); b.set_filters([1], top_k=3)
    am, lg = b.forward_tree([(0, 0, par, tok), (1, 0, par, tok)], logits=True)
    for r, exp in enumerate([masked(w, mask) for w, _ in want[0]] + [F.filtered(w, top_k=3) for w, _ in want[1]]):
        assert_bit_equal(lg[r], exp, f"row {r}")
        assert int(am[r]) == ref_argmax(exp), f"row {r}: argmax"
