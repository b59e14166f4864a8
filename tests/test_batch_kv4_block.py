"""Prompts of a Q4 paged batch through block attention over Q4 pages (launch_kv4_attention_block, lm.rs_amd/csrc/lmrs_kv4.inc): from MIN_ROWS rows on
(kKv4BlockMin in lmrs_api.hip) a chunk of one slot runs in 64-query blocks whose key staging and value tiles read the nibbles back, the diagonal taken
from the row's own f32 key and value.  Judged against the round-trip witness of tests/test_batch_kv4.py (one run per class) and against the table pass
of the same batch (lmrs_batch_debug_prefill_table).  Every comparison is bit for bit.  No tolerances."""
import functools

import numpy as np
import pytest

from parity_rules import assert_bit_equal
from test_batch import check_slot_rows, step
from test_batch_embed import random_rows
from test_batch_kv4 import QSeq
from test_batch_paged_deep import config
from tools import synth_lmrs as S

pytestmark = pytest.mark.gpu

N = 400
PL = 64
SEED = 913
MIN_ROWS = 320                                              # a Q4 paged batch's shortest chunk that takes block attention
# one class per kernel instantiation: head sizes 64, 96, 128 and Gemma's 256
CLASSES = [("mini-llama-1k", S.Q8_0), ("mini-phi-long", S.Q8_0), ("mini-llama3b-1k", S.Q8_0), ("mini-gemma-1k", S.Q4_0)]
# five whole blocks | a sixth block of one row | a start inside a page and a key chunk behind a table-pass call, diagonal tiles that straddle a chunk, a
# partial last block | a start on a page edge, the end one past a chunk edge (T = 385)
PLANS = [[320], [321], [70, 320], [64, 321]]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


@functools.lru_cache(maxsize=None)
def witness(cfg, q):
    """the round-trip oracle over one 400-token run -> (image, tokens, the QSeq holding every K/V row, logits per position); chunking never enters it"""
    img = S.build_image(config(cfg), q, seed=SEED)
    toks = S.prompt_tokens(config(cfg), N, SEED)
    seq = QSeq(img, 0)
    logits = np.stack([seq.feed([t]) for t in toks])
    logits.setflags(write=False)
    return img, toks, seq, logits


class Prefix:
    """a slot that holds the first n tokens of the witness run: check_slot_rows and step read the witness through it"""

    def __init__(self, w, slot, n):
        self.slot, self.orc, self.n, self.logits = slot, w[2].orc, n, w[3]

    def feed(self, toks):
        self.n += len(toks)
        return self.logits[self.n - 1]


@pytest.mark.parametrize("cfg,q", CLASSES)
def test_against_the_witness(L, cfg, q):
    w = witness(cfg, q)
    img, toks = w[0], w[1]
    m = L.Transformer(img)
    b = L.Batch(m, len(PLANS), page_len=PL, n_pages=32, kv="q4")
    seqs = []
    for slot, plan in enumerate(PLANS):
        at = 0
        for n in plan:
            assert b.prefill_form(n, at) == (1, 1 if n >= MIN_ROWS else 0), f"{cfg}: prefill_form({n}, {at})"
            assert b.prefill(slot, toks[at:at + n], at) == at + n
            at += n
        seqs.append(Prefix(w, slot, at))
        check_slot_rows(b, seqs[-1], range(at), f"{cfg} q{q}: {plan}")
    step(b, seqs, [int(toks[s.n]) for s in seqs], f"{cfg} q{q}: the decode pass behind the prefills")


def test_routing(L):
    m = L.Transformer(S.build_image(config("mini-llama-1k"), S.Q8_0, seed=SEED))
    b = L.Batch(m, 1, page_len=PL, n_pages=4, kv="q4")
    # kPrefillTokens = 512: 600 rows are a chunk of 512, which the rule takes, and one of 88, which it does not
    asked = [(300, 0), (319, 0), (320, 0), (600, 0), (330, 600)]
    assert [b.prefill_form(*x) for x in asked] == [(1, 0), (1, 0), (1, 1), (2, 1), (1, 1)]
    b.debug_prefill_table(True)
    assert b.prefill_form(320, 0) == (1, 0)
    b.debug_prefill_table(False)
    assert b.prefill_form(320, 0) == (1, 1)
    assert L.Batch(m, 1, page_len=PL, n_pages=4, kv="q8").prefill_form(256, 0) == (1, 1), "a Q8 paged batch keeps its own rule"
    assert L.Batch(m, 1, page_len=PL, n_pages=4).prefill_form(130, 0) == (1, 1), "an f32 paged batch keeps its own rule"


# the memory-resident softmax between the new launches | Gemma-2's 64-key score form and 64-dim value slices | embedding rows
ROUTES = [("mini-llama-1k", S.Q8_0, "LMRS_ATT_LDS_KEYS", "64", False), ("mini-gemma-1k", S.Q4_0, "LMRS_ATT_LONG_BATCH_FORMS", "1", False),
          ("mini-phi-long", S.Q8_0, None, None, True)]


@pytest.mark.parametrize("cfg,q,env,value,embed", ROUTES)
def test_block_route_equals_the_table_pass(L, monkeypatch, cfg, q, env, value, embed):
    """slot 0 by the library's rule, slot 1 forced to the table pass, the same 70 + 330 rows: every K/V row and one decode step's logits are equal"""
    if env:
        monkeypatch.setenv(env, value)
    m = L.Transformer(S.build_image(config(cfg), q, seed=SEED + 1))
    b = L.Batch(m, 2, page_len=PL, n_pages=16, kv="q4")
    toks = S.prompt_tokens(config(cfg), N + 1, SEED + 2)
    rows = random_rows(N, m.args.dim, SEED + 3) if embed else None
    for slot in (0, 1):
        b.debug_prefill_table(slot == 1)
        for at, n in ((0, 70), (70, 330)):
            assert b.prefill_form(n, at) == (1, 1 if n >= MIN_ROWS and slot == 0 else 0), f"{cfg}: prefill_form({n}, {at}), slot {slot}"
            if embed:
                assert b.prefill_embeddings(slot, rows[at:at + n], at) == at + n
            else:
                assert b.prefill(slot, toks[at:at + n], at) == at + n
    for layer in range(m.args.n_layers):
        for p in range(N):
            for which in (0, 1):
                assert_bit_equal(b.kv_row(0, which, layer, p), b.kv_row(1, which, layer, p), f"{cfg}: {'kv'[which]} layer {layer} pos {p}, block against table")
    am, lg = b.forward([0, 1], [int(toks[N])] * 2, [N, N], logits=True)
    assert_bit_equal(lg[0], lg[1], f"{cfg}: the decode step's logits, block against table")
