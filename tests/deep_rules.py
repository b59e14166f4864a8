"""Deep-context parity (tests/test_deep_context.py): the geometries, the token sequence, the reasoned position sets and the ONE oracle run per geometry
that every test of that module shares.  Not a test module.

The models are the mini shapes with one layer and 8192 positions (the library's clamp of seq_len), Q8_0.  With one layer a K/V row depends on its token
and its position alone, never on attention: a cache mismatch and an attention mismatch are told apart at once, and a row that is re-forwarded with its
own token is restored bit for bit.  Every context, slot and run of the tests replays toks[p] at position p, so the one oracle pass serves all of them,
shallow slots included.  Everything the oracle is asked beyond that pass - greedy chains, fill_kv_cache calls, the teeth - runs on the kept oracle object
and puts the rows it touched back (restore), asserting a kept logits vector is reproduced."""
import collections
import dataclasses
import functools
import time

import numpy as np

import oracle_lib as O
from parity_rules import assert_bit_equal, bits, ref_argmax
from tools import synth_lmrs as S

SEED = 5
SEQ_LEN = 8192
# how far the oracle walks: the 64-wide and the 256-wide (Gemma-2: soft-cap, window) geometry to the clamp; the 128-wide one into the 32-chunk bucket
# (from 4096); Phi's 96-wide heads - 32 kv heads, the costly oracle - into the 16-chunk bucket (from 2048)
DEPTH = {"mini-llama": 8192, "mini-gemma": 8192, "mini-llama3b": 4416, "mini-phi": 2320}
NAMES = tuple(DEPTH)

# ---- the positions of the single decode steps
# step_form_for: the split form starts at 384; its buckets of 4, 8, 16, 32 chunks of 256 keys change at 1024, 2048, 4096 (below 1024 the unsplit merged
# launch ends too: qa_max_T)
EDGES = (383, 384, 1023, 1024, 2047, 2048, 4095, 4096)
# inside the 32-chunk bucket: the first position whose value chunk / score chunk count grows past 17 (4351 | 4352), the middle chunk edge (6143 | 6144, and
# 6145: the second key of a fresh chunk), the last chunk's first key (7935 | 7936), and the last two positions the library holds
DEEP32 = (4351, 4352, 6143, 6144, 6145, 7935, 7936, 8190, 8191)
INTERIOR = (3000, 5000, 7000)
# Gemma-2's 4096-key window: at 4097 key 0 is the first key masked; at 4224 the whole first 128-key value chunk (SplitGeom<256>::CHK) is behind the window
# for the first time, at 4352 the whole first 256-key score chunk
GEMMA_WINDOW = (4097, 4223, 4224, 4351, 4352)
# the 128-wide geometry's capped-grid case of tests/test_gpu_split_merged.py (24 heads x 16 chunks no longer fit the resident slots), kept comparable
CAPPED_GRID = (2100, 2101, 2102, 2103)

# ---- consecutive steps across the bucket edges and up to the clamp; Gemma's across the window's chunk edges
DENSE = (range(1020, 1029), range(2044, 2053), range(4092, 4101), range(8184, 8192))
GEMMA_DENSE = (range(4220, 4229), range(4348, 4357))

# ---- the cache a batched prefill leaves: about 20 rows over every bucket, the 512-row pass edges among them
CACHE_AT = (0, 1, 255, 256, 383, 511, 512, 1023, 1024, 2047, 2048, 3000, 4095, 4096, 4607, 4608, 6143, 6144, 7000, 7935, 8189)

N_GREEDY = 12
FILL_ROWS = 40
# ---- batches: slot 0 deep beside three shallow slots
BATCH_DEEP = 8000
BATCH_SHALLOW = (3, 255, 400)
BATCH_RUN = 7                     # slot 0's run in forward_runs: positions 8002 .. 8008
BATCH_GREEDY = 4
BATCH_KV = (0, 4095, 7999, 8000, 8001, 8002, 8008, 8009, 8100, 8190, 8191)
PENALTY_AT = (8191, 4097, 4095)   # cap 8192 with every key live; cap 8192 about half live; cap 4096


def depth_of(name):
    return DEPTH[name]


def is_gemma(name):
    return name == "mini-gemma"


def config(name):
    return dataclasses.replace(S.CONFIGS[name], name=name + "-deep", n_layers=1, max_pos=SEQ_LEN)


def clip(positions, depth):
    return sorted({p for p in positions if p < depth})


def step_positions(name):
    """the single steps of a geometry: every set above that its depth holds, and its own last position"""
    d = DEPTH[name]
    ps = set(EDGES) | set(DEEP32) | set(INTERIOR) | {d - 1}
    if is_gemma(name):
        ps |= set(GEMMA_WINDOW)
    if name == "mini-llama3b":
        ps |= set(CAPPED_GRID)
    return clip(ps, d)


def dense_ranges(name):
    d = DEPTH[name]
    return [r for r in DENSE + (GEMMA_DENSE if is_gemma(name) else ()) if r[-1] < d]


def cache_positions(name):
    """rows of prefill_tokens(toks[:depth - 1]): CACHE_AT below the depth, and the last row of the call"""
    d = DEPTH[name]
    return clip(set(CACHE_AT) | {d - 2}, d - 1)


def greedy_starts(name):
    """generate_greedy of 12 steps: across a bucket edge (4096, Phi: 2048), and the run whose last written position is the geometry's last"""
    d = DEPTH[name]
    return [2042 if d < 4102 else 4090, d - N_GREEDY]


def fill_one_positions(name):
    """one-row fill_kv_cache calls (the plain attention kernel at depth): the last position, and a chunk edge"""
    d = DEPTH[name]
    return [d - 1, 6144 if d > 6144 else (4096 if d > 4096 else 2048)]


def fill_run_start(name):
    return DEPTH[name] - FILL_ROWS - 2          # 8150 at the clamp


def tokens_runs(name):
    """forward_tokens calls (start, n): the rows of block attention at depth"""
    d = DEPTH[name]
    if d == SEQ_LEN:
        return [(8000, 192), (4090, 20)]        # 192 rows over about 8k keys; in-block queries on both sides of Gemma's window
    return [(d - 64, 64)]


def batch_positions():
    """what the batch test feeds, call by call: (slots' positions of the two forward calls, the runs' first positions, the greedy starts)"""
    first = (BATCH_DEEP,) + BATCH_SHALLOW
    second = tuple(p + 1 for p in first)
    runs = (BATCH_DEEP + 2,) + tuple(p + 2 for p in BATCH_SHALLOW)
    greedy = (BATCH_DEEP + 2 + BATCH_RUN,) + tuple(p + 3 for p in BATCH_SHALLOW)
    return first, second, runs, greedy


def keep_positions(name):
    """KEEP: the union of every position whose logits or K/V rows a test of this geometry reads"""
    d = DEPTH[name]
    ps = set(step_positions(name)) | set(cache_positions(name))
    for r in dense_ranges(name):
        ps |= set(r)
    for s in greedy_starts(name):
        ps |= set(range(s, s + N_GREEDY))
    ps |= set(fill_one_positions(name)) | set(range(fill_run_start(name), fill_run_start(name) + FILL_ROWS))
    for s, n in tokens_runs(name):
        ps |= set(range(s, s + n))
    if d == SEQ_LEN:
        first, second, runs, greedy = batch_positions()
        ps |= set(first) | set(second) | set(runs[1:]) | set(range(runs[0], runs[0] + BATCH_RUN)) | set(BATCH_KV) | set(PENALTY_AT)
        for s in greedy:
            ps |= set(range(s, s + BATCH_GREEDY))
    return clip(ps, d)


Ref = collections.namedtuple("Ref", "name cfg img toks depth logits K V chains fill_toks fill_emb fills orc seconds")


def restore(ref_or_orc, toks, positions, logits):
    """the oracle's rows at `positions` back to toks' (one layer: a row is its token and position), each forward's logits against the kept vector"""
    orc = getattr(ref_or_orc, "orc", ref_or_orc)
    for p in positions:
        got = orc.forward(int(toks[p]), p)
        if p in logits:
            assert_bit_equal(got, logits[p], f"oracle: logits at {p} after the restore")


def _chain(orc, toks, logits, start, n):
    """the greedy chain of generate_greedy([toks[start]], n, start): toks[start] fed at start, then each argmax at the next position; the rows it
    overwrote are put back"""
    t, out = int(toks[start]), []
    for k in range(n):
        t = ref_argmax(orc.forward(t, start + k)); out.append(t)
    restore(orc, toks, range(start + 1, start + n), logits)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """ONE oracle pass forward(toks[p], p) for p = 0 .. depth - 1 over the geometry's seeded tokens -> Ref, read-only: logits / K / V as dicts by position
    over keep_positions(name); chains[start] = the greedy tokens the oracle continues toks[:start + 1] with (12 for the context's starts, 4 for the batch's);
    fills: what orc.fill_kv_cache leaves - ("one", p) -> (residual row, K row, V row) of fill_toks[0]'s embedding at p, ("run", p0) -> (residual [40, dim],
    {p: (K row, V row)}) of fill_toks' 40 rows at p0; and the oracle object itself, its rows as the pass left them, for the teeth."""
    cfg, d = config(name), DEPTH[name]
    img = S.build_image(cfg, S.Q8_0, seed=SEED)
    toks = S.prompt_tokens(cfg, d, SEED)
    orc = O.Oracle(img)
    keep = set(keep_positions(name))
    logits, K, V = {}, {}, {}
    t0 = time.time()
    for p in range(d):
        lg = orc.forward(int(toks[p]), p)
        if p in keep:
            logits[p] = lg.copy(); K[p] = orc.kv_row(0, 0, p); V[p] = orc.kv_row(1, 0, p)
    seconds = time.time() - t0
    print(f"\noracle: {name}, one layer: {d} sequential steps in {seconds:.1f} s")
    chains = {s: _chain(orc, toks, logits, s, N_GREEDY) for s in greedy_starts(name)}
    if d == SEQ_LEN:
        chains.update({s: _chain(orc, toks, logits, s, BATCH_GREEDY) for s in batch_positions()[3]})
    fill_toks = S.prompt_tokens(cfg, FILL_ROWS, SEED + 1)
    fill_emb = orc.get_embeddings(fill_toks).reshape(FILL_ROWS, cfg.dim)
    fills = {}
    for p in fill_one_positions(name):
        e = fill_emb[0].copy()
        assert orc.fill_kv_cache(e, p) == p + 1
        fills["one", p] = (e, orc.kv_row(0, 0, p), orc.kv_row(1, 0, p))
        restore(orc, toks, [p], logits)
    p0 = fill_run_start(name)
    e = fill_emb.copy().reshape(-1)
    assert orc.fill_kv_cache(e, p0) == p0 + FILL_ROWS
    fills["run", p0] = (e.reshape(FILL_ROWS, cfg.dim), {p: (orc.kv_row(0, 0, p), orc.kv_row(1, 0, p)) for p in (p0, p0 + FILL_ROWS // 2, p0 + FILL_ROWS - 1)})
    restore(orc, toks, range(p0, p0 + FILL_ROWS), logits)
    for a in [toks, fill_toks, fill_emb] + list(logits.values()) + list(K.values()) + list(V.values()):
        a.setflags(write=False)
    return Ref(name, cfg, img, toks, d, logits, K, V, chains, fill_toks, fill_emb, fills, orc, seconds)


def rows(ref, positions):
    return np.stack([ref.logits[p] for p in positions])


def moved_by(ref, key, query):
    """Teeth, on the oracle alone: does another token at position `key` move the logits at `query`?  The key's row is put back and the query's kept
    logits must come out again, bit for bit."""
    V = ref.cfg.vocab_size
    try:
        ref.orc.forward(int((ref.toks[key] + 1) % V), key)
        got = ref.orc.forward(int(ref.toks[query]), query).copy()
    finally:
        ref.orc.forward(int(ref.toks[key]), key)
    restore(ref, ref.toks, [query], ref.logits)
    return int((bits(got) != bits(ref.logits[query])).sum())
