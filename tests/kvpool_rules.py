"""Quantised page pools (tests/test_batch_kvpool_deep.py): the formats, their block floors, and the round-trip witnesses every test of that module
shares.  Not a test module.

The witness is the standing one (tests/test_batch_kvq.py, tests/test_batch_kv4.py): the per-sequence CPU oracle with, after each forward(token, pos), the
K and V rows of pos in every layer replaced by their quantise -> read-back round trip (QSeq).  Chunking, page length and call form never enter it, so ONE
run per (class, format) serves every slot of every test: a slot that holds toks[:d] and is fed toks[d] must give the run's logits row d and leave the
run's K/V row d."""
import collections
import functools
import types

import numpy as np

import oracle_lib as O
import test_batch_kv4 as kv4
import test_batch_kvq as kvq
from parity_rules import assert_bit_equal, ref_argmax
from test_batch_paged_deep import N_NEW, SEED, config
from tools import synth_lmrs as S

FORMATS = ("q8", "q4")
FLOOR = {"q8": 256, "q4": 320}                                # the shortest prompt chunk that takes block attention (kKvqBlockMin, kKv4BlockMin)
QSEQ = {"q8": kvq.QSeq, "q4": kv4.QSeq}
ROUND_TRIP = {"q8": kvq.round_trip, "q4": kv4.round_trip}
PAGE_SCALE = {"q8": (9, 8), "q4": (5, 8)}                     # bytes a value: 1 + 4 / 32 and 1 / 2 + 4 / 32
CHUNK = 512                                                   # rows a prefill pass (kPrefillTokens)
# one class per kernel instantiation: head sizes 64, 96, 128 and Gemma's 256; 1024 positions each
DEEP = [("mini-llama-1k", S.Q8_0), ("mini-phi-long", S.Q8_0), ("mini-llama3b-1k", S.Q8_0), ("mini-gemma-1k", S.Q4_0)]
BRANCH_FROM = (250, 505, 760)                                 # the greedy branches' first positions
BRANCH_EDGE = {250: 256, 505: 512, 760: 768}

Ref = collections.namedtuple("Ref", "cfg img toks logits K V branch brows")


def pages_of(n, page_len):
    return -(-n // page_len)


def expected_form(fmt, n, forced_table=False):
    """(chunks, block chunks) of a prefill of n rows by the documented rule: passes of 512 rows, block attention from the format's floor on"""
    chunks = [min(CHUNK, n - i) for i in range(0, n, CHUNK)]
    return len(chunks), 0 if forced_table else sum(m >= FLOOR[fmt] for m in chunks)


def kv_rows(orc, n_layers, positions):
    return [np.stack([np.stack([orc.kv_row(w, l, p) for p in positions]) for l in range(n_layers)]) for w in (0, 1)]


@functools.lru_cache(maxsize=None)
def witness(cfg, q, fmt, n=1024):
    """The round-trip oracle over positions 0 .. n - 1 of one seeded token run: image, tokens, logits [n, vocab], K and V rows [layers, n, kv_dim] as
    the pages must read back, read-only.  For the 1024-position runs also the greedy branches the device loop is judged by, continued on the same
    QSeq after that capture, from each d of BRANCH_FROM in DESCENDING order: toks[d] fed at d, then the argmax at d + 1, and so on for 12 steps;
    branch[d] are the tokens, brows[d] the K and V rows [layers, 12, kv_dim] the branch left at d .. d + 11, copied before the next branch runs.  A
    branch overwrites only rows above its own d and the starts lie more than 12 apart, so a shallower branch never reads a row a deeper one rewrote:
    each is what a fresh QSeq fed toks[:d + 1] would continue with (tests/test_batch_paged_deep.py's reference() and branch_rows() in one run)."""
    c = config(cfg)
    img = S.build_image(c, q, seed=SEED)
    toks = S.prompt_tokens(c, n, SEED)
    seq = QSEQ[fmt](img, 0)
    logits = np.stack([seq.feed([t]) for t in toks])
    K, V = kv_rows(seq.orc, c.n_layers, range(n))
    branch, brows = {}, {}
    for d in sorted(BRANCH_FROM, reverse=True) if n == 1024 else ():
        seq.n = d
        t, out = int(toks[d]), []
        for _ in range(N_NEW):
            t = ref_argmax(seq.feed([t])); out.append(t)
        branch[d], brows[d] = out, kv_rows(seq.orc, c.n_layers, range(d, d + N_NEW))
        assert_bit_equal(brows[d][0][:, 0], K[:, d], f"{cfg} {fmt}: the branch from {d} starts on the run's own row")
    for a in (toks, logits, K, V):
        a.setflags(write=False)
    return Ref(c, img, toks, logits, K, V, branch, brows)


class RefCache:
    """what check_slot_rows asks of an oracle, answered from a witness"""

    def __init__(self, ref):
        self.ref, self.args = ref, types.SimpleNamespace(n_layers=ref.K.shape[0])

    def kv_row(self, which, layer, pos):
        return (self.ref.K, self.ref.V)[which][layer, pos]


class WSeq:
    """a slot that holds toks[:n] of a witness run and may only be fed toks[n]: what test_batch.step, check_slot_rows and test_batch_runs.run_pass need of
    a sequence (slot, n, feed, orc)"""

    def __init__(self, ref, slot, n=0):
        self.ref, self.slot, self.n, self.orc = ref, slot, n, RefCache(ref)

    def feed(self, toks):
        lg = None
        for t in toks:
            assert int(t) == int(self.ref.toks[self.n]), f"slot {self.slot} at {self.n}: the witness knows one token sequence only"
            lg = self.ref.logits[self.n]
            self.n += 1
        return lg

    def next(self, n=1):
        return [int(t) for t in self.ref.toks[self.n:self.n + n]]


def qbatch(L, m, fmt, page_len, n_slots, n_pages=None):
    """a paged batch of the format whose pool could hold every slot at full depth; its kv_format is the one asked for"""
    b = L.Batch(m, n_slots, page_len=page_len, n_pages=n_pages or n_slots * pages_of(m.args.seq_len, page_len), kv=fmt)
    a, (num, den) = m.args, PAGE_SCALE[fmt]
    assert b.kv_format() == (fmt, 32, 2 * a.n_layers * page_len * a.n_kv_heads * a.head_size * num // den)
    return b


def prefill(b, fmt, slot, toks, at=0, forced_table=False):
    """one prefill call, after asserting that the library routes its chunks as the floors say"""
    n = len(toks)
    assert b.prefill_form(n, at) == expected_form(fmt, n, forced_table), f"prefill_form({n}, {at}) on a {fmt} pool: {b.prefill_form(n, at)}"
    assert b.prefill(slot, toks, at) == at + n


def assert_reads_zero(b, slot, n_layers, positions, what):
    """a position nobody wrote, or a released one, reads as zero numerically (an all-zero Q4 page reads back as -0.0: lmrs_kv4.inc)"""
    for layer in range(n_layers):
        for p in positions:
            for w in (0, 1):
                assert not b.kv_row(slot, w, layer, p).any(), f"{what}: slot {slot} {'kv'[w]} layer {layer} pos {p} is not zero"


def stats_run(img, cfg, fmt, n, seed):
    """a QSeq run of n positions on `img` with the oracle's regime counters of every single position -> (Ref, stats per position)"""
    toks = S.prompt_tokens(cfg, n, seed)
    seq = QSEQ[fmt](img, 0)
    rows, stats = [], []
    for t in toks:
        O.stats_reset()
        rows.append(seq.feed([t]))
        stats.append(O.stats())
    logits = np.stack(rows)
    K, V = kv_rows(seq.orc, cfg.n_layers, range(n))
    for a in (toks, logits, K, V):
        a.setflags(write=False)
    return Ref(cfg, img, toks, logits, K, V, {}, {}), tuple(stats)
