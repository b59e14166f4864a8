"""lmrs_forward_tokens / lmrs_score_tokens (include/lmrs_hip.h): the logits of every position of a token sequence and the log-probability of
each next token.  The reference is the CPU oracle's SEQUENTIAL forward (one call per token, transformer.rs:316-384): logits, K/V rows and the
forward that follows bit for bit, argmax by lmrs_ref_argmax, log-probabilities against a float64 log-softmax of the oracle's logits."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, check_after, check_scores, oracle_rows
from tools import synth_lmrs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def _random_cfg():
    rng = np.random.default_rng(2001)
    return S.random_cfg(rng, 1, max_pos=128)


FORWARD_CASES = [
    ("mini-llama", S.Q8_0, 70, 5), ("mini-llama", S.Q4_0, 70, 5), ("mini-phi", S.Q8_0, 140, 0),
    ("mini-llama3b", S.Q8_0, 57, 0),                 # one ragged ring tile
    ("mini-llama", S.Q8_0, 20, 3),                   # below the ring kernel's 48 tokens
    ("mini-llama", S.Q8_0, 1, 9),
    ("mini-llama-long", S.Q8_0, 600, 3),             # two layer passes of 512 tokens
    ("mini-llama-v4102", S.Q8_0, 40, 2),             # zero tail, classifier rows not a multiple of 16: token path
    ("mini-gemma", S.Q8_0, 30, 4), ("mini-gemma", S.Q4_0, 30, 0),     # token path
    ("mini-llama", S.Q_NONE, 12, 1),                 # unquantised
    ("random", S.Q8_0, 40, 2),                      # a 128- or 256-wide geometry: outside what the batched pass admits, token path (tests/test_lattice.py: the batched one)
]


@gpu
@pytest.mark.parametrize("cfg,q,n,start", FORWARD_CASES)
def test_forward_tokens_matches_sequential_forward(L, cfg, q, n, start):
    c = _random_cfg() if cfg == "random" else cfg
    img = S.build_image(c, q, seed=31)
    m = L.Transformer(img); orc = O.Oracle(img)
    toks = S.prompt_tokens(c, n, 31)
    got = m.forward_tokens(toks, start)
    want = oracle_rows(orc, toks, start)
    assert_bit_equal(got, want, f"{cfg} q{q} n={n}: logits of every position")
    check_after(m, orc, n, start, f"{cfg} q{q} n={n}")


SCORE_CASES = [("mini-llama", S.Q8_0, 70, 5), ("mini-llama", S.Q4_0, 70, 5), ("mini-phi", S.Q8_0, 140, 0), ("mini-llama-v4102", S.Q8_0, 40, 2),
               ("mini-gemma", S.Q8_0, 30, 4), ("mini-llama", S.Q8_0, 1, 0), ("mini-llama-long", S.Q8_0, 600, 3)]


@gpu
@pytest.mark.parametrize("cfg,q,n,start", SCORE_CASES)
def test_score_tokens_matches_the_oracle(L, cfg, q, n, start):
    img = S.build_image(cfg, q, seed=37)
    m = L.Transformer(img); orc = O.Oracle(img)
    toks = S.prompt_tokens(cfg, n, 37)
    got = m.score(toks, start)
    rows = oracle_rows(orc, toks, start)
    check_scores(got, rows, toks, f"{cfg} q{q} n={n}")
    check_after(m, orc, n, start, f"{cfg} q{q} n={n}")


@gpu
def test_score_llama_1b_at_full_size(L):
    """Llama-3.2-1B Q8_0, 600 tokens: two batched passes, the classifier GEMM over 128 256 rows; logits of positions 0, 511, 512, 599."""
    cfg = "llama-3.2-1b"
    img = S.build_image(cfg, S.Q8_0, seed=1234)
    toks = S.prompt_tokens(cfg, 600, 41)
    m = L.Transformer(img)
    got = m.score(toks, 0)
    lg = m.forward_tokens(toks, 0)[[0, 511, 512, 599]].copy()
    orc = O.Oracle(img)
    rows = oracle_rows(orc, toks, 0)
    check_scores(got, rows, toks, "llama-3.2-1b")
    assert_bit_equal(lg, rows[[0, 511, 512, 599]], "llama-3.2-1b logits at 0, 511, 512, 599")


@gpu
@pytest.mark.parametrize("cfg,q,n", [("mini-llama", S.Q8_0, 70), ("mini-phi", S.Q8_0, 100), ("mini-llama", S.Q4_0, 60)])
def test_batched_and_token_paths_give_the_same_bits(L, monkeypatch, cfg, q, n):
    img = S.build_image(cfg, q, seed=43)
    toks = S.prompt_tokens(cfg, n, 43)
    a = L.Transformer(img)
    monkeypatch.setenv("LMRS_NO_BATCHED_PREFILL", "1")
    b = L.Transformer(img)
    monkeypatch.delenv("LMRS_NO_BATCHED_PREFILL")
    ra, rb = a.score(toks, 2), b.score(toks, 2)
    assert_bit_equal(ra[0], rb[0], "logprobs, batched vs token by token")
    assert ra[1].tolist() == rb[1].tolist() and ra[2] == rb[2]
    check_scores(ra, oracle_rows(O.Oracle(img), toks, 2), toks, f"{cfg} q{q}")


@gpu
def test_errors_are_reported_and_leave_the_context_usable(L):
    img = S.build_image("mini-llama", S.Q8_0, seed=47)
    m = L.Transformer(img); orc = O.Oracle(img)
    V, T = m.args.vocab_size, m.args.seq_len
    toks = S.prompt_tokens("mini-llama", 24, 47)
    bad = toks.copy(); bad[5] = V
    for call in (m.score, m.forward_tokens):
        with pytest.raises(L.LmrsError, match="out of range"):
            call(bad, 0)
        with pytest.raises(L.LmrsError, match="seq_len"):
            call(toks, T - 10)
        with pytest.raises(L.LmrsError, match="n == 0"):
            call(np.zeros(0, np.uint32), 0)
    check_scores(m.score(toks, 0), oracle_rows(orc, toks, 0), toks, "after the errors")
    grp = L.ShardGroup(img, 2)
    lp = np.zeros(23, np.float32); am = np.zeros(24, np.uint32); s = ctypes.c_double()
    rc = L.lib().lmrs_score_tokens(grp._arr[0], toks.ctypes.data, toks.size, 0, lp.ctypes.data, am.ctypes.data, ctypes.byref(s))
    assert rc != 0 and "single-GPU" in L.lib().lmrs_last_error().decode()
    grp.close()
    check_scores(m.score(toks, 0), oracle_rows(orc, toks, 0), toks, "after the refused shard")


@gpu
def test_scoring_releases_its_device_memory(L):
    hip = ctypes.CDLL("libamdhip64.so")
    def free_bytes():
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    img = S.build_image("mini-llama", S.Q8_0, seed=5)
    toks = S.prompt_tokens("mini-llama", 80, 5)
    def one_round():
        m = L.Transformer(img)
        m.score(toks, 0); m.forward_tokens(toks[:30], 0); m.score(toks[:1], 0)
        m.close()
    import gc
    gc.collect()                                   # (contexts of earlier tests that only a collection frees go first)
    one_round(); one_round(); one_round()          # (the first rounds may grow runtime-internal pools)
    before = free_bytes()
    for _ in range(10):
        one_round()
    gc.collect()
    after = free_bytes()
    assert before - after < 64 << 20, f"device memory shrank by {(before - after) >> 20} MiB over 10 create / score / destroy rounds"


def _ppl_fixture(tmp_path):
    """a 2-layer Llama-geometry model and a tokenizer.bin in the layout tokenizer.rs:24-64 reads (full Llama vocabulary size)"""
    import struct
    cfg = S.ModelCfg("llama-2layer", 2048, 8192, 2, 32, 64, 8, 128256, 131072, 1e-5, 500000.0, S.LLAMA)
    img = S.build_image(cfg, S.Q8_0, seed=53)
    img.tofile(tmp_path / "model.lmrs")
    toks = [("<unk>", 0.0), ("<s>", 0.0), ("</s>", 0.0)] + [("<0x%02X>" % b, 0.0) for b in range(256)]
    toks += [(ch, -1.0 - i) for i, ch in enumerate(" abcdefghijklmnopqrstuvwxyz.,")]
    toks += [(w, 5.0 - 0.1 * i) for i, w in enumerate(["he", "ll", "hell", "hello", " w", "or", "ld", " world", "th", " th", "the", " the"])]
    toks += [("<fill_%d>" % i, 0.0) for i in range(cfg.vocab_size - len(toks))]
    blob = struct.pack("IIII", len(toks), 16, 128000, 128009)
    for s_, sc in toks:
        b = s_.encode(); blob += struct.pack("fI", sc, len(b)) + b
    (tmp_path / "tokenizer.bin").write_bytes(blob)
    return img, blob


@gpu
def test_perplexity_program(L, tmp_path):
    """hostcpp/perplexity.cpp, built with g++ and run: its nll is the sum of Transformer.score over the same windows."""
    img, blob = _ppl_fixture(tmp_path)
    text = "hello world, the world. " * 9 + "the hello.\n"
    (tmp_path / "text.txt").write_text(text)
    exe = str(tmp_path / "perplexity")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "lm.rs_amd", "hostcpp", "perplexity.cpp"), "-I", os.path.join(ROOT, "include"),
                    "-L", os.path.join(ROOT, "lm.rs_amd"), "-llmrs_hip", f"-Wl,-rpath,{os.path.join(ROOT, 'lm.rs_amd')}", "-o", exe], check=True)
    ctx, stride = 48, 20
    out = subprocess.run([exe, "--model", str(tmp_path / "model.lmrs"), "--tokenizer", str(tmp_path / "tokenizer.bin"), "--text",
                          str(tmp_path / "text.txt"), "--ctx", str(ctx), "--stride", str(stride)], capture_output=True, text=True, check=True).stdout
    res = json.loads(out.strip().splitlines()[-1])
    ids = L.Tokenizer(blob).encode(text, True, False, False, 1)
    N = len(ids)
    assert N > ctx + stride, N
    m = L.Transformer(img)
    nll, count, done, b = 0.0, 0, 1, 0
    while True:
        e = min(b + ctx, N)
        if done < e:
            lp, _, _ = m.score(ids[b:e], 0)
            for j in range(max(b + 1, done), e):
                nll -= float(lp[j - b - 1]); count += 1
            done = e
        if e == N:
            break
        b += stride
    assert res["tokens"] == count == N - 1
    assert res["nll"] == nll, (res["nll"], nll)
    assert abs(res["ppl"] - np.exp(nll / count)) <= 1e-12 * res["ppl"]


# ------------------------------------------------------------------ CPU
def test_rust_ffi_declares_the_scoring_entry_points():
    import test_rust_crate as R
    c, r = R.c_prototypes(), R.rust_externs()
    for name in ("lmrs_forward_tokens", "lmrs_score_tokens"):
        assert name in c, f"{name} is not in include/lmrs_hip.h"
        assert name in r, f"{name} is not declared in rust/lmrs-hip/src/ffi.rs"
        (cret, cargs), (rret, rargs) = c[name], r[name]
        assert R.CMAP[cret] == rret and [R.CMAP[a] for a in cargs] == rargs, (name, cargs, rargs)
    t = re.sub(r"\s+", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "transformer.rs")).read())
    assert "pub fn forward_tokens(&mut self, tokens: &[u32], start_pos: u32) -> Vec<f32>" in t
    assert "pub fn score(&mut self, tokens: &[u32], start_pos: u32) -> (Vec<f32>, Vec<u32>, f64)" in t


def test_score_kernels_have_no_scratch_and_no_spills():
    import lmrs_amd
    from tools import kernel_resources as KR
    lmrs_amd.build()
    ks = KR._kernels_of(os.path.join(KR.CSRC, "lmrs_score.o"))
    names = " ".join(n for n, _ in ks)
    assert "score_chunk_kernel" in names and "score_merge_kernel" in names, names
    for n, k in ks:
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (n, k)


def test_perplexity_program_and_host_mirror_compile(tmp_path):
    import lmrs_amd
    lmrs_amd.build()
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "lm.rs_amd", "hostcpp", "perplexity.cpp")],
                   check=True, capture_output=True)
    assert "lmrs_forward_tokens" in lmrs_amd.EXPORTS and "lmrs_score_tokens" in lmrs_amd.EXPORTS
    lib = ctypes.CDLL(lmrs_amd.LIB_PATH)
    assert hasattr(lib, "lmrs_forward_tokens") and hasattr(lib, "lmrs_score_tokens")
