"""Paged K/V in 4 bits (lmrs_batch_create_paged_q4, lm.rs_amd/csrc/lmrs_kv4.inc).  The witness is tests/test_batch_kvq.py's: the per-sequence CPU oracle
with, after each forward(token, pos), the K and V rows of pos in every layer replaced by their round trip - here the reference's Q4_0 rule at groups of 32
(lmrs_ref_op_quantize_q4), read back as (nibble - 8) * scale in f32.  Every comparison is bit for bit, signs of zero included."""
import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from test_batch import Seq, check_slot_rows, step
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
PL = 64
CLASSES = [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-llama3b", S.Q8_0), ("mini-gemma", S.Q4_0)]       # head sizes 64, 96, 128, Gemma's 256


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def round_trip(row):
    q, s = O.quantize_q4(row, gs=32)
    nib = np.stack([q & 15, q >> 4], axis=1).reshape(-1).astype(np.float32)
    return (nib - np.float32(8)) * np.repeat(s, 32)


class QSeq(Seq):
    def feed(self, toks):
        lg, a = None, self.orc.args
        for t in toks:
            lg = self.orc.forward(int(t), self.n).copy()
            for layer in range(a.n_layers):
                for which in (0, 1):
                    row = np.ctypeslib.as_array(O.lib().lmrs_ref_kv(self.orc.h, which, layer, self.n), shape=(a.n_kv_heads * a.head_size,))
                    row[:] = round_trip(row)
            self.n += 1
        return lg


def among_zeros(*vals):
    g = np.zeros(32, np.float32)
    g[3:3 + 2 * len(vals):2] = vals
    return g


HOSTILE = {
    "all zeros": np.zeros(32, np.float32),
    "linspace": np.linspace(-1, 1, 32, dtype=np.float32),
    "denormal maximum": among_zeros(1e-45, -1e-45),
    "huge": among_zeros(3e38, -3e38, 1e38),
    "every half-way point, scale 1": np.concatenate([7.5 - np.arange(16), [-8.0] * 16]).astype(np.float32),      # x / -1 + 8 = k + 0.5, k = 0 .. 15
    "signed zeros": among_zeros(-0.0, 2.0, -2.0),
}


@gpu
def test_hostile_groups_through_the_hook(L):
    x = np.concatenate(list(HOSTILE.values()))
    want = round_trip(x)
    assert np.isfinite(want).all()
    got = L.kv4_round_trip(x)
    for i, name in enumerate(HOSTILE):
        assert_bit_equal(got[32 * i:32 * i + 32], want[32 * i:32 * i + 32], name)


@gpu
@pytest.mark.parametrize("cfg,q", CLASSES)
def test_rows_and_steps(L, cfg, q):
    img = S.build_image(cfg, q, seed=701)
    m = L.Transformer(img)
    depths = [0, 1, 63, 64, 65, 130]
    b = L.Batch(m, len(depths), page_len=PL, n_pages=16, kv="q4")
    a = m.args
    assert b.kv_format() == ("q4", 32, 2 * a.n_layers * PL * a.n_kv_heads * a.head_size * 5 // 8)
    # (these classes' caches hold 256 positions: the longest prompt they admit, one chunk at the Q8 pool's block floor; 300 rows: test_beyond_one_key_pass)
    assert b.prefill_form(min(300, a.seq_len))[1] == 0
    seqs = [QSeq(img, i) for i in range(len(depths))]
    for s, n in zip(seqs, depths):
        toks = S.prompt_tokens(cfg, n, 710 + s.slot) if n else []
        for part, p0 in ((toks[:n // 2], 0), (toks[n // 2:], n // 2)):
            if len(part):
                b.prefill(s.slot, part, p0)
        s.feed(toks)
        check_slot_rows(b, s, sorted({0, n // 2, n - 1}) if n else [], f"{cfg} q{q}: Q4 prefill of {n}")
    assert not b.kv_row(2, 0, 0, 63).any() and not b.kv_row(0, 1, 1, 5).any(), "a position nobody wrote reads as zero"
    V = a.vocab_size
    for k in range(3):
        step(b, seqs, [(13 * i + 5 * k + 3) % V for i in range(len(depths))], f"{cfg} q{q} Q4 step {k}")


@gpu
@pytest.mark.parametrize("cfg,q", CLASSES)
def test_forks(L, cfg, q):
    img = S.build_image(cfg, q, seed=721)
    m = L.Transformer(img)
    b = L.Batch(m, 5, page_len=PL, n_pages=16, kv="q4")
    prefix = S.prompt_tokens(cfg, 70, 722)
    b.prefill(0, prefix, 0)
    seqs = [QSeq(img, i) for i in range(4)]
    for s in seqs:
        s.feed(prefix)
        if s.slot:
            b.fork(0, s.slot, 70)
    assert [b.slot_pages(i) for i in range(4)] == [(2, 1)] * 4 and b.pages()[2] == 16 - 5, "a shared whole page, one copied"
    check_slot_rows(b, seqs[2], [0, 63, 64, 69], f"{cfg} q{q}: the forked prefix")
    own = S.prompt_tokens(cfg, 70, 723)
    m.prefill_tokens(own, 0)
    b.fork(L.BATCH_CTX, 4, 70)
    for layer in range(m.args.n_layers):
        for p in (0, 63, 64, 69):
            for w in (0, 1):
                assert_bit_equal(b.kv_row(4, w, layer, p), round_trip(m.kv_row(w, layer, p)), f"{cfg} q{q}: fork from the context, {'kv'[w]} layer {layer} pos {p}")
    for k in range(2):
        step(b, seqs, [(31 * i + 7 * k + 1) % m.args.vocab_size for i in range(4)], f"{cfg} q{q} Q4 forked step {k}")


@gpu
def test_device_loop_crosses_a_page_edge(L):
    cfg, q = "mini-llama", S.Q8_0
    img = S.build_image(cfg, q, seed=731)
    m = L.Transformer(img)
    b = L.Batch(m, 2, page_len=PL, n_pages=8, kv="q4")
    seqs, first = [QSeq(img, 0), QSeq(img, 1)], [3, 400]
    for s, n in zip(seqs, (61, 3)):
        toks = S.prompt_tokens(cfg, n, 732 + s.slot)
        b.prefill(s.slot, toks, 0)
        s.feed(toks)
    out = b.generate_greedy([0, 1], first, [61, 3], 6)
    for i, s in enumerate(seqs):
        t, want = first[i], []
        for _ in range(6):
            t = ref_argmax(s.feed([t])); want.append(t)
        assert out[i].tolist() == want, f"row {i}"
        check_slot_rows(b, s, list(range(s.n - 6, s.n)), "rows written by the device loop")


@gpu
def test_beyond_one_key_pass(L):
    cfg, q = "mini-llama-long", S.Q8_0
    img = S.build_image(cfg, q, seed=741)
    m = L.Transformer(img)
    b = L.Batch(m, 1, page_len=PL, n_pages=6, kv="q4")
    assert b.prefill_form(300)[1] == 0 and L.Batch(m, 1, page_len=PL, n_pages=6, kv="q8").prefill_form(300)[1] == 1, "a chunk the Q8 pool sends to block attention"
    s, toks = QSeq(img, 0), S.prompt_tokens(cfg, 290, 742)
    b.prefill(0, toks, 0)
    s.feed(toks)
    for k in range(2):
        step(b, [s], [(17 * k + 9) % m.args.vocab_size], f"Q4 step {k} at {290 + k} keys")
