"""lmrs_verify_tokens / lmrs_draft_lookup / lmrs_generate_speculative (include/lmrs_hip.h) and the skinny GEMM under them (lmrs_debug_gemm_skinny).
The reference is the CPU oracle's SEQUENTIAL forward (one call per token, transformer.rs:316-384) with lmrs_ref_argmax, and the oracle's matmul_q8 /
matmul_q4 for the kernel: everything bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, check_kv_rows, check_scores, oracle_rows, ref_argmax, run_positions
from tools import synth_lmrs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def oracle_argmax(orc, toks, start):
    """sample_argmax of the oracle's sequential forward for toks[i] at start + i"""
    return [ref_argmax(orc.forward(int(t), start + i)) for i, t in enumerate(toks)]


def check_forward_after(m, orc, pos, what):
    t = 7 % orc.args.vocab_size
    assert_bit_equal(m.forward(t, pos), orc.forward(t, pos), f"{what}: forward at {pos} after the call")


# ---------------------------------------------------------------------------------------------- 1. the kernel

def _gemm_operands(rng, n, o, n_tok, q4):
    G = n // 128
    ws = rng.uniform(0.001, 0.02, (o, G)).astype(np.float32)
    xs = rng.uniform(0.001, 0.05, (n_tok, G)).astype(np.float32)
    if not q4:
        wq = rng.integers(-127, 128, (o, n), dtype=np.int8)
        xq = rng.integers(-127, 128, (n_tok, n), dtype=np.int8)
        xq[:, 128:256] = 0                                       # a group of all-zero activations
        xq[0, :] = 127; wq[0, :] = 127; wq[o - 1, :] = -127      # saturated rows
        if n_tok > 1:
            xq[n_tok - 1, :] = -127
    else:
        wq = rng.integers(0, 256, (o, n // 2), dtype=np.uint8)
        xq = rng.integers(0, 256, (n_tok, n // 2), dtype=np.uint8)
        xq[:, 64:128] = 0x88                                     # nibble 8 = value 0
        xq[0, :] = 0xFF; wq[0, :] = 0xFF; wq[o - 1, :] = 0x00    # +7 / -8: the format's extremes
        if n_tok > 1:
            xq[n_tok - 1, :] = 0x00
    return xq, xs, wq, ws


def _gemm_reference(xq, xs, wq, ws, n, o, n_tok, q4):
    if not q4:
        return O.matmul_q8(xq, xs, wq, ws, n, o, sl=n_tok).reshape(n_tok, o)
    return np.stack([O.matmul_q4(xq[t], xs[t], wq, ws, n, o) for t in range(n_tok)])


@gpu
@pytest.mark.parametrize("q4", [False, True], ids=["q8", "q4"])
@pytest.mark.parametrize("n", [256, 2304, 9216])
def test_skinny_gemm_matches_the_oracle(L, n, q4):
    """one tile, a ragged last wave's worth of rows and several workgroups; every token count class of the 16-wide tile"""
    rng = np.random.default_rng(1000 + n + int(q4))
    for o in (16, 48, 272):
        full = _gemm_operands(rng, n, o, 16, q4)
        for n_tok in (1, 2, 3, 7, 8, 15, 16):
            xq, xs, wq, ws = full[0][:n_tok].copy(), full[1][:n_tok].copy(), full[2], full[3]
            got = L.debug_gemm_skinny(xq, xs, wq, ws, n, o, n_tok, q4)
            assert_bit_equal(got, _gemm_reference(xq, xs, wq, ws, n, o, n_tok, q4), f"n {n} o {o} n_tok {n_tok} q4 {q4}")


@gpu
@pytest.mark.parametrize("q4", [False, True], ids=["q8", "q4"])
def test_skinny_gemm_wide_rows(L, q4):
    """from 8192 rows on a workgroup owns 32 rows: 8208 = 256 whole tiles and a ragged one"""
    n, o = 2048, 8208
    rng = np.random.default_rng(77 + int(q4))
    full = _gemm_operands(rng, n, o, 16, q4)
    for n_tok in (3, 16):
        xq, xs, wq, ws = full[0][:n_tok].copy(), full[1][:n_tok].copy(), full[2], full[3]
        got = L.debug_gemm_skinny(xq, xs, wq, ws, n, o, n_tok, q4)
        assert_bit_equal(got, _gemm_reference(xq, xs, wq, ws, n, o, n_tok, q4), f"wide rows n_tok {n_tok} q4 {q4}")


@gpu
def test_skinny_gemm_refuses_bad_shapes(L):
    z8 = np.zeros((17, 256), np.int8); zs = np.ones((17, 2), np.float32)
    for n, o, n_tok in ((128, 16, 2), (256, 8, 2), (256, 16, 17)):
        with pytest.raises(L.LmrsError, match="lmrs_debug_gemm_skinny"):
            L.debug_gemm_skinny(z8, zs, z8, zs, n, o, n_tok)


# ---------------------------------------------------------------------------------------------- 2. verify_tokens against the oracle

VERIFY_CFGS = [("mini-llama", S.Q8_0), ("mini-llama", S.Q4_0), ("mini-phi", S.Q8_0), ("mini-llama3b", S.Q8_0), ("mini-gemma", S.Q8_0), ("mini-gemma", S.Q4_0)]
NS = (2, 5, 16)


def _setup(L, cfg, q, start, seed=61, env=None):
    img = S.build_image(cfg, q, seed=seed)
    m = L.Transformer(img); orc = O.Oracle(img)
    if start:
        pre = S.prompt_tokens(cfg, start, seed + 1)
        if start >= 8:
            assert m.prefill_tokens(pre, 0) == start
        else:
            for i, t in enumerate(pre):
                m.forward(int(t), i)
        for i, t in enumerate(pre):
            orc.forward(int(t), i)
    return m, orc


def _true_continuation(orc, t0, start, length):
    """G[0] = t0 at `start`, G[i + 1] = the oracle's argmax after G[i]"""
    G = [int(t0)]
    for i in range(length - 1):
        G.append(ref_argmax(orc.forward(G[-1], start + i)))
    return G


def _verify_patterns(L, m, orc, start, what, ns=NS):
    V = orc.args.vocab_size
    G = _true_continuation(orc, 11 % V, start, 34)
    for n in ns:
        # the oracle's own greedy continuation: every draft accepted
        toks = np.array(G[:n], np.uint32)
        want = oracle_argmax(orc, toks, start)
        assert want == G[1:n + 1]
        am, acc = m.verify_tokens(toks, start)
        assert am.tolist() == want and acc == n - 1, f"{what} n {n}: true continuation"
        check_kv_rows(m, orc, run_positions(start, n), f"{what} n {n} true")
        check_forward_after(m, orc, start + n, f"{what} n {n} true")
        # draft j corrupted: the drafts before it accepted, the argmax of every position still forward's for the tokens given
        for j in sorted({0, n - 2}):
            bad = toks.copy(); bad[j + 1] = (G[j + 1] + 1) % V
            want = oracle_argmax(orc, bad, start)
            am, acc = m.verify_tokens(bad, start)
            assert am.tolist() == want and acc == j, f"{what} n {n}: draft {j} corrupted"
            check_kv_rows(m, orc, run_positions(start, n), f"{what} n {n} corrupt {j}")
            # the next pass: from start + n_accept + 1 with argmax[n_accept], over the stale rows of the rejected drafts
            assert int(am[acc]) == G[j + 1]
            nxt = np.array(G[j + 1:j + 1 + n], np.uint32)
            am2, acc2 = m.verify_tokens(nxt, start + acc + 1)
            assert am2.tolist() == G[j + 2:j + 2 + n] and acc2 == n - 1, f"{what} n {n}: the pass after a partial acceptance at {j}"


@gpu
@pytest.mark.parametrize("start", [0, 5, 70])
@pytest.mark.parametrize("cfg,q", VERIFY_CFGS)
def test_verify_tokens_matches_the_oracle(L, cfg, q, start):
    m, orc = _setup(L, cfg, q, start)
    _verify_patterns(L, m, orc, start, f"{cfg} q{q} start {start}")


# ---------------------------------------------------------------------------------------------- 3. fallbacks and witnesses

@gpu
@pytest.mark.parametrize("cfg,q,env", [("mini-llama", S.Q_NONE, False), ("mini-gemma9b", S.Q8_0, False), ("mini-llama", S.Q8_0, True)],
                         ids=["f32", "gemma9b", "no-batched-prefill"])
def test_verify_tokens_on_contexts_without_the_batched_pass(L, monkeypatch, cfg, q, env):
    if env:
        monkeypatch.setenv("LMRS_NO_BATCHED_PREFILL", "1")
    m, orc = _setup(L, cfg, q, 3)
    if env:
        monkeypatch.delenv("LMRS_NO_BATCHED_PREFILL")
    _verify_patterns(L, m, orc, 3, f"{cfg} q{q} token path", ns=(2, 5))


@gpu
def test_verify_tokens_with_classifier_rows_not_a_multiple_of_16(L):
    m, orc = _setup(L, "mini-llama-v4102", S.Q8_0, 3)
    _verify_patterns(L, m, orc, 3, "mini-llama-v4102", ns=(5,))
    toks = S.prompt_tokens("mini-llama-v4102", 12, 63)
    am, _ = m.verify_tokens(toks, 3)
    assert am.tolist() == m.score(toks, 3)[1].tolist() == oracle_argmax(orc, toks, 3)


@gpu
def test_the_token_run_rules_have_not_moved(L):
    m = L.Transformer(S.build_image("mini-llama", S.Q8_0, seed=61))
    assert m.tokens_path(4) is False and m.tokens_path(60) is True
    m.verify_tokens(S.prompt_tokens("mini-llama", 4, 1), 0)
    assert m.tokens_path(4) is False and m.tokens_path(60) is True


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_token_entry_points_interleaved_on_one_context(L, cfg, q):
    """Every token entry point on ONE context, each call starting where the one before it ended and judged by its own rule against the
    oracle's sequential forward: passes of both forms (up to 16 tokens: skinny; more: tiled) and runs on both sides of the batch minimum of 8
    follow each other, so a form or a state that outlived its call would show in the next one.  No forward between the calls: the K/V rows
    are read back instead, and the single forward comes last."""
    img = S.build_image(cfg, q, seed=67)
    m = L.Transformer(img); orc = O.Oracle(img)
    V = m.args.vocab_size
    toks = S.prompt_tokens(cfg, 60, 67)
    at = {"pos": 0}

    def run(n, continuation=False):
        """the next n tokens (or the oracle's own greedy continuation of the next one), their position, the oracle's logits rows for them"""
        pos = at["pos"]; at["pos"] += n
        t = np.array(_true_continuation(orc, toks[pos], pos, n), np.uint32) if continuation else toks[pos:pos + n].copy()
        return t, pos, oracle_rows(orc, t, pos)

    def verify(n, what, continuation=False):
        t, pos, rows = run(n, continuation)
        am, acc = m.verify_tokens(t, pos)
        want = [ref_argmax(r) for r in rows]
        want_acc = 0
        while want_acc + 1 < n and int(t[want_acc + 1]) == want[want_acc]:
            want_acc += 1
        assert am.tolist() == want and acc == want_acc, f"{cfg} q{q} {what}"
        assert not continuation or acc == n - 1
        check_kv_rows(m, orc, run_positions(pos, n), f"{cfg} q{q} {what}")

    verify(16, "1. verify_tokens of 16")
    t, pos, rows = run(20)
    check_scores(m.score(t, pos), rows, t, f"{cfg} q{q} 2. score of 20")
    check_kv_rows(m, orc, run_positions(pos, 20), f"{cfg} q{q} 2. score of 20")
    verify(5, "3. verify_tokens of 5", continuation=True)
    t, pos, rows = run(9)
    assert m.tokens_path(9) and m.prefill_tokens(t, pos) == pos + 9
    check_kv_rows(m, orc, run_positions(pos, 9), f"{cfg} q{q} 4. prefill_tokens of 9")
    t, pos, rows = run(3)
    assert not m.tokens_path(3)
    assert_bit_equal(m.forward_tokens(t, pos), rows, f"{cfg} q{q} 5. forward_tokens of 3")
    check_kv_rows(m, orc, run_positions(pos, 3), f"{cfg} q{q} 5. forward_tokens of 3")
    bad = toks[:12].copy(); bad[7] = V
    with pytest.raises(L.LmrsError, match="token 7 out of range"):
        m.score(bad, at["pos"])
    verify(2, "7. verify_tokens of 2", continuation=True)
    pos = at["pos"]
    assert pos == 16 + 20 + 5 + 9 + 3 + 2
    assert_bit_equal(m.forward(int(toks[pos]), pos), orc.forward(int(toks[pos]), pos), f"{cfg} q{q} 8. forward at {pos}")
    check_kv_rows(m, orc, [0, 15, 16, 35, 36, 40, 41, 49, 50, 52, 53, 54, pos], f"{cfg} q{q}: the rows of every call at the end")


# ---------------------------------------------------------------------------------------------- 4. generate_speculative

def _spec_prompts(cfg):
    block = S.prompt_tokens(cfg, 8, 71)
    return {"repeated": np.tile(block, 5).astype(np.uint32), "plain": S.prompt_tokens(cfg, 40, 72)}


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_generate_speculative_gives_greedys_tokens(L, cfg, q):
    m = L.Transformer(S.build_image(cfg, q, seed=73))
    n_new = 64
    for name, prompt in _spec_prompts(cfg).items():
        want = m.generate_greedy(prompt, n_new)
        for max_draft in (1, 7, 15):
            got, st = m.generate_speculative(prompt, n_new, max_draft=max_draft, ngram_max=3)
            assert got.tolist() == want.tolist(), f"{cfg} {name} max_draft {max_draft}"
            passes, drafted, accepted, plain = (int(v) for v in st)
            assert accepted <= drafted <= passes * max_draft
            assert passes + accepted + plain == n_new, (name, max_draft, st.tolist())
    # at a position other than 0, and a run that ends inside a pass
    prompt = _spec_prompts(cfg)["repeated"]
    got, st = m.generate_speculative(prompt, 9, start_pos=6, max_draft=15, ngram_max=2)
    assert got.tolist() == m.generate_greedy(prompt, 9, start_pos=6).tolist()
    assert int(st[0] + st[2] + st[3]) == 9


# ---------------------------------------------------------------------------------------------- 5. argument errors

@gpu
def test_argument_errors_leave_the_context_usable(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=61)
    m = L.Transformer(img); orc = O.Oracle(img)
    V, T = m.args.vocab_size, m.args.seq_len
    toks = S.prompt_tokens("mini-llama", 6, 81)
    want = oracle_argmax(orc, toks, 0)

    def good():
        assert m.verify_tokens(toks, 0)[0].tolist() == want

    with pytest.raises(L.LmrsError, match="outside 2 .. 16"):
        m.verify_tokens(toks[:1], 0)
    good()
    with pytest.raises(L.LmrsError, match="outside 2 .. 16"):
        m.verify_tokens(S.prompt_tokens("mini-llama", 17, 82), 0)
    good()
    with pytest.raises(L.LmrsError, match="seq_len"):
        m.verify_tokens(toks, T - 5)
    good()
    bad = toks.copy(); bad[3] = V
    with pytest.raises(L.LmrsError, match="out of range"):
        m.verify_tokens(bad, 0)
    good()
    am = np.zeros(6, np.uint32); acc = ctypes.c_uint32()
    lib = L.lib()
    assert lib.lmrs_verify_tokens(m._h, None, 6, 0, am.ctypes.data, ctypes.byref(acc)) != 0 and "NULL" in lib.lmrs_last_error().decode()
    assert lib.lmrs_verify_tokens(m._h, toks.ctypes.data, 6, 0, None, ctypes.byref(acc)) != 0 and "NULL" in lib.lmrs_last_error().decode()
    assert lib.lmrs_verify_tokens(m._h, toks.ctypes.data, 6, 0, am.ctypes.data, None) != 0 and "NULL" in lib.lmrs_last_error().decode()
    assert lib.lmrs_verify_tokens(None, toks.ctypes.data, 6, 0, am.ctypes.data, ctypes.byref(acc)) != 0 and "NULL" in lib.lmrs_last_error().decode()
    good()
    for md, ng, msg in ((0, 2, "max_draft"), (16, 2, "max_draft"), (4, 0, "ngram_max")):
        with pytest.raises(L.LmrsError, match=msg):
            m.generate_speculative(toks, 4, max_draft=md, ngram_max=ng)
    with pytest.raises(L.LmrsError, match="seq_len"):
        m.generate_speculative(toks, T, max_draft=4)
    good()
    grp = L.ShardGroup(img, 2)
    rc = lib.lmrs_verify_tokens(grp._arr[0], toks.ctypes.data, toks.size, 0, am.ctypes.data, ctypes.byref(acc))
    assert rc != 0 and "single-GPU" in lib.lmrs_last_error().decode()
    out = np.zeros(4, np.uint32)
    rc = lib.lmrs_generate_speculative(grp._arr[0], toks.ctypes.data, toks.size, 4, 0, 4, 2, out.ctypes.data, None, None)
    assert rc != 0 and "single-GPU" in lib.lmrs_last_error().decode()
    grp.close()
    good()


# ---------------------------------------------------------------------------------------------- 6. draft_lookup (no GPU)

def py_draft_lookup(hist, ngram_max, max_draft):
    hist = list(hist); n = len(hist)
    for ln in range(min(ngram_max, n - 1), 0, -1):               # the longest suffix first
        suf = hist[n - ln:]
        for s in range(n - ln - 1, -1, -1):                      # its latest earlier occurrence first
            if hist[s:s + ln] == suf:
                return hist[s + ln:s + ln + max_draft]
    return []


def test_draft_lookup_matches_its_transcription(L):
    rng = np.random.default_rng(91)
    hits = 0
    for _ in range(2000):
        hist = rng.integers(0, 6, int(rng.integers(0, 61))).astype(np.uint32)
        ng, md = int(rng.integers(1, 5)), int(rng.integers(1, 16))
        got = L.draft_lookup(hist, ng, md).tolist()
        assert got == py_draft_lookup(hist.tolist(), ng, md), (hist.tolist(), ng, md)
        hits += bool(got)
    assert hits > 1000


def test_draft_lookup_named_cases(L):
    assert L.draft_lookup([1, 2, 3, 4, 5], 3, 4).tolist() == []                              # no match
    assert L.draft_lookup([9], 3, 4).tolist() == []                                          # a history of length 1
    assert L.draft_lookup([], 3, 4).tolist() == []
    assert L.draft_lookup([1, 2, 3, 9, 1, 2], 2, 15).tolist() == [3, 9, 1, 2]                # the continuation ends with the history: shorter than max_draft
    assert L.draft_lookup([1, 2, 3, 1, 2, 4, 5, 1, 2], 2, 3).tolist() == [4, 5, 1]           # two earlier occurrences: the later one wins
    assert L.draft_lookup([7, 1, 2, 8, 3, 1, 2], 3, 2).tolist() == [8, 3]                    # no 3-gram match: the 2-gram's
    assert L.draft_lookup([5, 5, 5], 2, 4).tolist() == [5]                                   # an occurrence may overlap the suffix
    with pytest.raises(L.LmrsError, match="ngram_max"):
        L.draft_lookup([1, 2, 1], 0, 4)


# ---------------------------------------------------------------------------------------------- 7. ABI presence (no GPU)

NAMES = ("lmrs_verify_tokens", "lmrs_draft_lookup", "lmrs_generate_speculative", "lmrs_debug_gemm_skinny")


def test_entry_points_exist_in_every_layer(L):
    lib = L.lib()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in L.EXPORTS
    assert callable(L.Transformer.verify_tokens) and callable(L.Transformer.generate_speculative) and callable(L.draft_lookup)
    header = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in the header"
        assert re.search(rf"\bpub fn {name}\(", ffi), f"{name} is not declared in the Rust crate"
    for name in NAMES[:3]:
        assert name in hpp, f"{name} is not mirrored in transformer.hpp"
    rs = open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "transformer.rs")).read()
    assert "pub fn verify_tokens" in rs and "pub fn generate_speculative" in rs and "pub fn draft_lookup" in rs
