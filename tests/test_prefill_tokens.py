"""lmrs_prefill_tokens / lmrs_tokens_path (include/lmrs_hip.h) and Gemma-2 on the batched token path: a run of token ids leaves the K/V rows
that one Transformer::forward per token leaves (transformer.rs:316-384), whichever path the library takes.  The reference is the CPU oracle's
SEQUENTIAL forward; every comparison is on uint32 views, except log-probabilities (the rule of tests/parity_rules.py: one f32 ulp of a float64
log-softmax of the oracle's logits, the sum to 1e-9 relative)."""
import ctypes
import dataclasses
import os
import re
import subprocess
import time

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, bits, check_after, check_kv_rows, check_scores, oracle_rows
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


def no_batch_ctx(L, monkeypatch, img):
    monkeypatch.setenv("LMRS_NO_BATCHED_PREFILL", "1")
    try:
        return L.Transformer(img)
    finally:
        monkeypatch.delenv("LMRS_NO_BATCHED_PREFILL")


# ------------------------------------------------------------------ 1. the rows
PREFILL_CASES = [
    ("mini-llama", S.Q8_0, 70, 5), ("mini-llama", S.Q4_0, 70, 5), ("mini-phi", S.Q8_0, 140, 0),
    ("mini-llama-long", S.Q8_0, 600, 3),             # two passes of 512 tokens
    ("mini-gemma", S.Q8_0, 60, 4), ("mini-gemma", S.Q4_0, 75, 0),
    ("mini-llama", S.Q_NONE, 12, 1),                 # unquantised: token path
    ("mini-gemma9b", S.Q8_0, 30, 0),                 # a Gemma geometry the batched pass refuses: token path
    ("random", S.Q8_0, 40, 2),                      # a 128- or 256-wide geometry: outside what the batched pass admits, token path (tests/test_lattice.py: the batched one)
]


@gpu
@pytest.mark.parametrize("cfg,q,n,start", PREFILL_CASES)
def test_prefill_tokens_leaves_the_rows_of_sequential_forward(L, cfg, q, n, start):
    c = _random_cfg() if cfg == "random" else cfg
    img = S.build_image(c, q, seed=31)
    m = L.Transformer(img); orc = O.Oracle(img)
    toks = S.prompt_tokens(c, n, 31)
    assert m.prefill_tokens(toks, start) == start + n
    for i, t in enumerate(toks):
        orc.forward(int(t), start + i)
    check_after(m, orc, n, start, f"{cfg} q{q} n={n} (batched: {m.tokens_path(n)})")


# ------------------------------------------------------------------ 2. the path
@gpu
@pytest.mark.parametrize("q", [S.Q8_0, S.Q4_0])
def test_gemma_token_runs_take_the_batched_pass(L, monkeypatch, q):
    img = S.build_image("mini-gemma", q, seed=33)
    m = L.Transformer(img)
    assert m.tokens_path(60) is True
    assert m.tokens_path(1) is False
    assert no_batch_ctx(L, monkeypatch, img).tokens_path(60) is False
    assert L.Transformer(S.build_image("mini-gemma9b", q, seed=33)).tokens_path(60) is False
    ll = L.Transformer(S.build_image("mini-llama", q, seed=33))
    assert ll.tokens_path(60) is True and ll.tokens_path(1) is False


# ------------------------------------------------------------------ 3. Gemma through the existing entry points
@gpu
@pytest.mark.parametrize("q", [S.Q8_0, S.Q4_0])
def test_gemma_forward_tokens_score_and_greedy_on_the_batched_path(L, monkeypatch, q):
    cfg, n, start = "mini-gemma", 60, 4
    img = S.build_image(cfg, q, seed=35)
    toks = S.prompt_tokens(cfg, n, 35)
    a = L.Transformer(img); b = no_batch_ctx(L, monkeypatch, img); orc = O.Oracle(img)
    assert a.tokens_path(n) and not b.tokens_path(n)
    want = oracle_rows(orc, toks, start)
    dim = a.args.dim
    ga, gb = a.forward_tokens(toks, start), b.forward_tokens(toks, start)
    assert_bit_equal(ga[:, :dim], want[:, :dim], f"q{q}: soft-capped logits [0, dim) of every position")
    assert_bit_equal(ga[:, dim:], want[:, dim:], f"q{q}: logits [dim, vocab) of every position")
    assert_bit_equal(ga, gb, f"q{q}: batched vs token by token")
    check_after(a, orc, n, start, f"forward_tokens q{q}")
    sa, sb = a.score(toks, start), b.score(toks, start)
    check_scores(sa, want, toks, f"score q{q}")
    assert_bit_equal(sa[0], sb[0], "logprobs, batched vs token by token")
    assert sa[1].tolist() == sb[1].tolist() and sa[2] == sb[2]
    prompt = S.prompt_tokens(cfg, 40, 36)
    ids = a.generate_greedy(prompt, 8, 2)
    assert ids.tolist() == O.Oracle(img).generate_greedy(prompt, 8, 2).tolist(), f"q{q}: greedy ids after a batched 40-token prompt"
    assert ids.tolist() == b.generate_greedy(prompt, 8, 2).tolist()


# ------------------------------------------------------------------ 4. the window
@gpu
def test_gemma_window_is_tested_per_query_in_a_batched_pass():
    """Keys behind Gemma's 4096-key window.  mini-gemma's geometry with 4352 positions: 4080 tokens are ingested, then a batched run of 80
    tokens starts at 4080 - its queries at 4097 .. 4159 mask keys 0 .. 62, its earlier queries mask none.  A pass that tested the window
    against its first position (fill_kv_cache's meaning) would mask no old key at all.

    Teeth, on the oracle alone: after the run, K/V rows 0 .. 62 are overwritten (forward of other tokens at those positions).  forward at
    4159, whose window ends at key 63, must not move by a bit; forward at 4158, for which key 62 is live, must move."""
    import lmrs_amd as L
    cfg = dataclasses.replace(S.CONFIGS["mini-gemma"], name="mini-gemma-window", max_pos=4352)
    img = S.build_image(cfg, S.Q8_0, 29)
    n0, n1 = 4080, 80
    toks = S.prompt_tokens(cfg, n0 + n1, 29)
    m = L.Transformer(img); orc = O.Oracle(img)
    assert m.tokens_path(n0) and m.tokens_path(n1)
    assert m.prefill_tokens(toks[:n0], 0) == n0
    got = m.forward_tokens(toks[n0:], n0)
    t0 = time.time()
    for i in range(n0):
        orc.forward(int(toks[i]), i)
    want = oracle_rows(orc, toks[n0:], n0)
    print(f"\noracle: {n0 + n1} sequential steps in {time.time() - t0:.1f} s")
    assert_bit_equal(got, want, "logits of the 80 positions 4080 .. 4159")
    check_kv_rows(m, orc, [0, 2040, n0 - 1, n0, n0 + 17, n0 + 18, n0 + 40, n0 + n1 - 1], "window")
    # teeth
    for p in range(63):
        orc.forward(int((toks[p] + 1) % cfg.vocab_size), p)
    again = orc.forward(int(toks[-1]), n0 + n1 - 1).copy()
    assert_bit_equal(again, want[-1], "oracle: position 4159 does not see keys 0 .. 62")
    before = orc.forward(int(toks[-2]), n0 + n1 - 2).copy()
    assert (bits(before) != bits(want[-2])).any(), "oracle: position 4158 sees key 62 - the window test would be vacuous otherwise"


# ------------------------------------------------------------------ 5. fill_kv_cache keeps its own meaning
@gpu
@pytest.mark.parametrize("order", ["prefill_first", "fill_first"])
def test_gemma_fill_kv_cache_keeps_the_batched_call_semantics(L, order):
    """fill_kv_cache = ONE forward_layer(sl = n) call: rows as given (no sqrt(dim)), the window tested against curr_pos for the whole batch
    (lmrs_ref_fill_kv_cache).  prefill_tokens = n forward calls.  Neither leaks into the other, in either order on one context."""
    cfg = "mini-gemma"
    img = S.build_image(cfg, S.Q8_0, seed=39)
    m = L.Transformer(img); orc = O.Oracle(img)
    assert m.tokens_path(60)
    ta, tb = S.prompt_tokens(cfg, 50, 39), S.prompt_tokens(cfg, 60, 40)

    def fill(pos):
        a = m.get_embeddings(ta); b = orc.get_embeddings(ta)
        assert m.fill_kv_cache(a, pos) == orc.fill_kv_cache(b, pos) == pos + 50
        assert_bit_equal(a, b, f"{order}: residual stream after fill_kv_cache at {pos}")
        check_kv_rows(m, orc, [pos, pos + 25, pos + 49], f"{order}: fill_kv_cache at {pos}")

    def prefill(pos):
        assert m.prefill_tokens(tb, pos) == pos + 60
        for i, t in enumerate(tb):
            orc.forward(int(t), pos + i)
        check_kv_rows(m, orc, [pos, pos + 30, pos + 59], f"{order}: prefill_tokens at {pos}")

    if order == "prefill_first":
        prefill(0); fill(60)
        end = 110
    else:
        fill(3); prefill(53)
        end = 113
    assert_bit_equal(m.forward(7, end), orc.forward(7, end), f"{order}: forward at {end}")


# ------------------------------------------------------------------ 6. errors
@gpu
@pytest.mark.parametrize("cfg", ["mini-llama", "mini-gemma"])
def test_prefill_errors_are_reported_and_leave_the_context_usable(L, cfg):
    img = S.build_image(cfg, S.Q8_0, seed=47)
    m = L.Transformer(img); orc = O.Oracle(img)
    V, T = m.args.vocab_size, m.args.seq_len
    toks = S.prompt_tokens(cfg, 24, 47)
    bad = toks.copy(); bad[5] = V
    with pytest.raises(L.LmrsError, match="out of range"):
        m.prefill_tokens(bad, 0)
    with pytest.raises(L.LmrsError, match="seq_len"):
        m.prefill_tokens(toks, T - 10)
    with pytest.raises(L.LmrsError, match="n == 0"):
        m.prefill_tokens(np.zeros(0, np.uint32), 0)
    newp = ctypes.c_uint32()
    assert L.lib().lmrs_prefill_tokens(m._h, None, 24, 0, ctypes.byref(newp)) != 0 and "NULL" in L.lib().lmrs_last_error().decode()
    assert L.lib().lmrs_tokens_path(m._h, 24, None) != 0 and "NULL" in L.lib().lmrs_last_error().decode()
    assert_bit_equal(m.forward(int(toks[0]), 0), orc.forward(int(toks[0]), 0), "forward after the errors")
    assert L.lib().lmrs_prefill_tokens(m._h, toks.ctypes.data, toks.size, 1, None) == 0          # new_pos may be NULL
    for i, t in enumerate(toks):
        orc.forward(int(t), 1 + i)
    check_after(m, orc, 24, 1, "after the errors")


# ------------------------------------------------------------------ 7. full size
@gpu
def test_gemma_2b_q4_prefill_tokens_at_full_size(L):
    """Gemma-2-2B Q4_0: prefill_tokens of 300 tokens (one batched pass with forward's semantics), then 8 greedy ids from token 300 on -
    the ids the oracle produces after the same 300 tokens one forward at a time; K/V rows of the first and last layer."""
    cfg = "gemma-2-2b"
    img = S.build_image(cfg, S.Q4_0, seed=77)
    toks = S.prompt_tokens(cfg, 301, 78)
    m = L.Transformer(img)
    assert m.tokens_path(300)
    m.prefill_tokens(toks[:16], 0)                                         # (warm-up: buffers, first launches)
    t0 = time.perf_counter()
    assert m.prefill_tokens(toks[:300], 0) == 300
    ms = (time.perf_counter() - t0) * 1e3
    print(f"\ngemma-2-2b q4_0: prefill_tokens(300) {ms:.2f} ms")
    ids = m.generate_greedy(toks[300:], 8, 300)
    orc = O.Oracle(img)
    want = orc.generate_greedy(toks, 8, 0)
    assert ids.tolist() == want.tolist()
    check_kv_rows(m, orc, [0, 150, 299], "gemma-2-2b")


# ------------------------------------------------------------------ 8. the chat program
def _chat_fixture(tmp_path):
    import struct
    cfg = S.ModelCfg("llama-2layer", 2048, 8192, 2, 32, 64, 8, 128256, 2048, 1e-5, 500000.0, S.LLAMA)
    img = S.build_image(cfg, S.Q8_0, seed=91)
    img.tofile(tmp_path / "model.lmrs")
    # a tokenizer.bin in the layout tokenizer.rs:24-64 reads, full Llama vocabulary size (the chat template ids must exist)
    toks = [("<unk>", 0.0), ("<s>", 0.0), ("</s>", 0.0)] + [("<0x%02X>" % b, 0.0) for b in range(256)]
    toks += [(ch, -1.0 - i) for i, ch in enumerate(" abcdefghijklmnopqrstuvwxyzSO0123456789")]
    toks += [(m, 5.0 - 0.1 * i) for i, m in enumerate(["he", "ll", "hell", "hello", " w", "or", "ld", " world", "wor", "Se", "ep", "Sep", "20", "24", "2024", "23"])]
    toks += [("<fill_%d>" % i, 0.0) for i in range(cfg.vocab_size - len(toks))]
    blob = struct.pack("IIII", len(toks), 16, 128000, 128009)
    for s_, sc in toks:
        b = s_.encode(); blob += struct.pack("fI", sc, len(b)) + b
    (tmp_path / "tokenizer.bin").write_bytes(blob)
    return cfg, img, blob


def _step_by_step_chat(L, cfg, img, blob, lines, temperature, top_p, seed, date, max_tokens, turn_tokens):
    """The loop of chat.rs:148-227 with one forward + one sampler call per prompt token (what hostcpp/chat.cpp did before prefill_tokens),
    over the library: the bytes the program must print."""
    tk = L.Tokenizer(blob); m = L.Transformer(img); smp = L.Sampler(cfg.vocab_size, temperature, top_p, seed)

    def piece(token):
        buf = ctypes.create_string_buffer(256); n = ctypes.c_size_t()
        assert L.lib().lmrs_tokenizer_decode(tk._h, token, buf, 256, ctypes.byref(n)) == 0
        return buf.raw[: n.value]

    out, pos, nxt, sampled = b"", 0, 0, 0
    for line in lines:
        out += b"You: "
        prompt = []
        if pos == 0:
            prompt += [128000, 128006, 9125, 128007, 271, 38766, 1303, 33025, 2696, 25, 6790, 220, 2366, 18, 198, 15724, 2696, 25, 220]
            prompt += tk.encode(date, False, False, False, 1).tolist() + [271, 128009]
        prompt += tk.encode(line.strip(), False, False, True, 1).tolist()
        out += b"Assistant:\n"
        idx, turn = 0, 0
        while True:
            if idx < len(prompt):
                token = prompt[idx]; idx += 1
            else:
                token = nxt
            if token == tk.eos and idx >= len(prompt):
                out += b"\n"
                break
            nxt = m.forward_argmax(token, pos) if temperature == 0.0 else m.forward_sample(token, pos, smp)
            pos += 1
            gen = idx >= len(prompt)
            if gen and turn_tokens >= 0:
                turn += 1
                if turn >= turn_tokens:
                    nxt = tk.eos
            if gen and nxt != tk.eos:
                out += piece(nxt)
            if gen and max_tokens >= 0:
                sampled += 1
                if sampled >= max_tokens:
                    return out + b"\n"
    return out + b"You: "


@gpu
@pytest.mark.parametrize("temperature,top_p", [(0.0, None), (0.7, None), (0.7, 1.0)])
def test_chat_program_prints_what_the_step_by_step_loop_prints(L, tmp_path, temperature, top_p):
    """hostcpp/chat.cpp, two turns: the bytes of a run whose library takes the batched pass, of a run with LMRS_NO_BATCHED_PREFILL=1, and of
    the step-by-step loop (one forward and one sampler call per prompt token) are the same.  temperature 0.7 at the default top-p 0.9 keeps
    the step-by-step prompt in the program itself (sample_topp's candidate vector carries earlier calls' entries: sampler.rs:81);
    top-p 1.0 is sample_mult, where the discarded prompt draws leave no trace and the prompt is prefilled."""
    cfg, img, blob = _chat_fixture(tmp_path)
    exe = str(tmp_path / "chat")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "lm.rs_amd", "hostcpp", "chat.cpp"), "-I", os.path.join(ROOT, "include"),
                    "-L", os.path.join(ROOT, "lm.rs_amd"), "-llmrs_hip", f"-Wl,-rpath,{os.path.join(ROOT, 'lm.rs_amd')}", "-o", exe], check=True)
    args = [exe, "--model", str(tmp_path / "model.lmrs"), "--tokenizer", str(tmp_path / "tokenizer.bin"), "--temperature", str(temperature),
            "--seed", "7", "--date", "23 Sep 2024", "--max-tokens", "12", "--turn-tokens", "6"]
    if top_p is not None:
        args += ["--top-p", str(top_p)]
    lines = ["  hello world  ", "the world says hello"]
    stdin = ("\n".join(lines) + "\n").encode()
    env = dict(os.environ); env.pop("LMRS_NO_BATCHED_PREFILL", None)
    a = subprocess.run(args, input=stdin, capture_output=True, check=True, env=env).stdout
    b = subprocess.run(args, input=stdin, capture_output=True, check=True, env=dict(env, LMRS_NO_BATCHED_PREFILL="1")).stdout
    assert a == b, (a, b)
    want = _step_by_step_chat(L, cfg, img, blob, lines, temperature, 0.9 if top_p is None else top_p, 7, "23 Sep 2024", 12, 6)
    assert a == want, (a, want)
    assert a.count(b"Assistant:\n") == 2, a                                # the second turn's prompt starts past position 0


# ------------------------------------------------------------------ CPU
def test_every_binding_names_both_entry_points():
    import lmrs_amd
    import test_rust_crate as R
    c, r = R.c_prototypes(), R.rust_externs()
    for name in ("lmrs_prefill_tokens", "lmrs_tokens_path"):
        assert name in c, f"{name} is not in include/lmrs_hip.h"
        assert name in r, f"{name} is not declared in rust/lmrs-hip/src/ffi.rs"
        (cret, cargs), (rret, rargs) = c[name], r[name]
        assert R.CMAP[cret] == rret and [R.CMAP[a] for a in cargs] == rargs, (name, cargs, rargs)
        assert name in lmrs_amd.EXPORTS
        assert name in open(os.path.join(ROOT, "lm.rs_amd", "__init__.py")).read()
        assert name in open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    lib = ctypes.CDLL(lmrs_amd.build())
    assert hasattr(lib, "lmrs_prefill_tokens") and hasattr(lib, "lmrs_tokens_path")
    assert hasattr(lmrs_amd.Transformer, "prefill_tokens") and hasattr(lmrs_amd.Transformer, "tokens_path")
    t = re.sub(r"\s+", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "transformer.rs")).read())
    assert "pub fn prefill_tokens(&mut self, tokens: &[u32], start_pos: u32) -> u32" in t
    assert "pub fn tokens_path(&self, n: usize) -> bool" in t
    assert "prefill_tokens" in open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "chat.cpp")).read()


def test_chat_program_and_host_mirror_compile(tmp_path):
    host = os.path.join(ROOT, "lm.rs_amd", "hostcpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(host, "chat.cpp")], check=True, capture_output=True)
    tu = tmp_path / "mirror.cpp"
    tu.write_text('#include "transformer.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", host, str(tu)], check=True, capture_output=True)


def test_softcap_kernel_has_no_scratch_and_no_spills():
    import lmrs_amd
    from tools import kernel_resources as KR
    lmrs_amd.build()
    ks = [(n, k) for n, k in KR._kernels_of(os.path.join(KR.CSRC, "lmrs_score.o")) if "softcap_rows_kernel" in n]
    assert len(ks) == 1, ks
    for n, k in ks:
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (n, k)


def test_prompt_rate_tool_and_its_profiles_are_listed():
    readme = open(os.path.join(ROOT, "profiles", "README.md")).read()
    assert "tools/prompt_rate.py" in readme
    for f in ("prompt_rate_gemma2b_q4.txt", "prompt_rate_llama1b.txt", "score_rate_gemma2b_q4.txt"):
        assert f in readme, f
        assert os.path.exists(os.path.join(ROOT, "profiles", f)), f
    assert os.path.exists(os.path.join(ROOT, "tools", "prompt_rate.py"))
