"""Wide batches (lmrs_batch_create_wide, include/lmrs_hip.h): up to 64 sequences a step in one weight pass, and the stream GEMM that serves a pass of
17 .. 47 rows (lmrs_debug_gemm_wide runs it at 1 .. 64 tokens).  The reference is one CPU oracle PER SEQUENCE fed token by token (tests/test_batch.py's Seq); every comparison -
argmax, logits, K/V rows, the hook's products - is bit for bit (tests/parity_rules.py)."""
import ctypes
import dataclasses

import numpy as np
import pytest

from parity_rules import assert_bit_equal, ref_argmax
from test_batch import CFGS, DEPTHS16, Seq, check_slot_rows, snapshot, step
from test_batch_runs import run_pass, toks_for
from test_verify import _gemm_operands, _gemm_reference
from tools import synth_lmrs as S

gpu = pytest.mark.gpu

# 64 slots: sixteen at the depths the attention forms change at, the other 48 at 0 .. 5, cycling
DEPTHS64 = DEPTHS16 + [i % 6 for i in range(48)]
EVERY_N = [17, 31, 32, 33, 47, 48, 49, 63, 64]                 # both sides of every token tile of the stream GEMM and of its hand-over to the ring kernels (48)
FEW_N = [17, 33, 64]


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def wide_prefilled(L, img, cfg, lengths, seed, n_slots=64):
    """test_batch.prefilled on a WIDE batch: slot i prefilled with lengths[i] tokens, one oracle per slot"""
    m = L.Transformer(img)
    b = L.Batch(m, n_slots, wide=True)
    assert b.width == 64
    seqs = []
    for i, n in enumerate(lengths):
        s = Seq(img, i)
        if n:
            toks = S.prompt_tokens(cfg, n, seed + i)
            assert b.prefill(i, toks, 0) == n
            s.feed(toks)
        seqs.append(s)
    return m, b, seqs


def step_in_place(b, seqs, toks, what):
    """test_batch.step, then every sequence that stands within 8 positions of the fixtures' 256 goes back one: the next pass rewrites that row (both sides
    read nothing of it), so a slot at 252 can take part in every pass of a test"""
    am = step(b, seqs, toks, what)
    for s in seqs:
        if s.n > 248:
            s.n -= 1
    return am


# ---------------------------------------------------------------------------------------------- 1. the GEMM hook

@gpu
@pytest.mark.parametrize("q4", [False, True], ids=["q8", "q4"])
@pytest.mark.parametrize("n", [256, 2304, 8192, 9216])
def test_wide_gemm_matches_the_oracle(L, n, q4):
    """G = 2 (fewer groups than waves), 18 (a ragged last round), 64 and 72 (eight and nine rounds); one row tile, three, seventeen; every token count
    class of two, three and four 16-wide tiles, and the one-tile counts the kernel also serves"""
    rng = np.random.default_rng(2000 + n + int(q4))
    for o in (16, 48, 272):
        full = _gemm_operands(rng, n, o, 64, q4)
        ref = _gemm_reference(full[0], full[1], full[2], full[3], n, o, 64, q4)          # one reference per shape: row t depends on token t alone
        for n_tok in (1, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64):
            xq, xs = full[0][:n_tok].copy(), full[1][:n_tok].copy()
            got = L.debug_gemm_wide(xq, xs, full[2], full[3], n, o, n_tok, q4)
            assert_bit_equal(got, ref[:n_tok], f"n {n} o {o} n_tok {n_tok} q4 {q4}")


@gpu
@pytest.mark.parametrize("q4", [False, True], ids=["q8", "q4"])
def test_wide_gemm_wide_rows(L, q4):
    """from 8192 rows on a workgroup owns 32 rows: 8208 = 256 whole tiles and a ragged one"""
    n, o = 2048, 8208
    rng = np.random.default_rng(2100 + int(q4))
    full = _gemm_operands(rng, n, o, 49, q4)
    ref = _gemm_reference(full[0], full[1], full[2], full[3], n, o, 49, q4)
    for n_tok in (17, 33, 49):
        got = L.debug_gemm_wide(full[0][:n_tok].copy(), full[1][:n_tok].copy(), full[2], full[3], n, o, n_tok, q4)
        assert_bit_equal(got, ref[:n_tok], f"o {o} n_tok {n_tok} q4 {q4}")


@gpu
def test_wide_gemm_refuses_bad_shapes(L):
    rng = np.random.default_rng(5)
    xq, xs, wq, ws = _gemm_operands(rng, 512, 32, 65, False)
    for n, o, n_tok in ((512, 32, 65), (512, 32, 0), (384, 32, 17), (0, 32, 17), (512, 24, 17), (512, 0, 17)):
        with pytest.raises(L.LmrsError, match="lmrs_debug_gemm_wide"):
            L.debug_gemm_wide(xq, xs, wq, ws, n, o, n_tok, False)
    lib = L.lib()
    assert lib.lmrs_debug_gemm_wide(0, None, xq.ctypes.data, xs.ctypes.data, wq.ctypes.data, ws.ctypes.data, 512, 32, 17, 0) != 0
    assert "lmrs_debug_gemm_wide" in lib.lmrs_last_error().decode()
    got = L.debug_gemm_wide(xq[:17].copy(), xs[:17].copy(), wq, ws, 512, 32, 17, False)          # ... and a valid call still works
    assert_bit_equal(got, _gemm_reference(xq[:17], xs[:17], wq, ws, 512, 32, 17, False), "after the refusals")
    with pytest.raises(L.LmrsError, match="lmrs_debug_gemm_skinny"):                              # the skinny hook keeps its own limit
        L.debug_gemm_skinny(xq[:17].copy(), xs[:17].copy(), wq, ws, 512, 32, 17, False)


# ---------------------------------------------------------------------------------------------- 2. one pass, rows at many depths

@gpu
@pytest.mark.parametrize("cfg,q", CFGS)
def test_many_rows_at_different_depths_in_one_pass(L, cfg, q):
    img = S.build_image(cfg, q, seed=271)
    m, b, seqs = wide_prefilled(L, img, cfg, DEPTHS64, 272)
    V = seqs[0].orc.args.vocab_size
    every = (cfg, q) in (("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0))
    for k, n in enumerate(EVERY_N if every else FEW_N):
        toks = [(13 * i + 5 * k + 3) % V for i in range(n)]
        step_in_place(b, seqs[:n], toks, f"{cfg} q{q} n {n}")


@gpu
def test_gemma_window_per_row_in_a_wide_pass(L):
    """tests/test_batch.py's window case in a 20-row pass: slot 0 stands at 4100 - its queries mask keys 0 .. pos - 4097 - beside 19 short rows that mask none"""
    cfg = dataclasses.replace(S.CONFIGS["mini-gemma"], name="mini-gemma-window", max_pos=4352)
    img = S.build_image(cfg, S.Q8_0, 29)
    m, b, seqs = wide_prefilled(L, img, cfg, [4100] + [i % 4 for i in range(19)], 29, n_slots=20)
    for k in range(2):
        step(b, seqs, [50 + k + i for i in range(20)], f"window step {k}")
    step(b, seqs[::-1], [90 + i for i in range(20)], "window step, the shallow rows first")


# ---------------------------------------------------------------------------------------------- 3. the device loop

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_generate_greedy_of_40_and_64_rows(L, cfg, q):
    img = S.build_image(cfg, q, seed=287)
    m, b, seqs = wide_prefilled(L, img, cfg, DEPTHS64, 288)
    for s in seqs:
        s.n = min(s.n, 240)                                    # (two loops of 5 steps end below the fixtures' 256 positions: the deepest rows are rewritten)
    V = seqs[0].orc.args.vocab_size
    for n, rows in ((40, seqs[12:52][::-1]), (64, seqs)):
        first = [(7 * i + n) % V for i in range(n)]
        pos0 = [s.n for s in rows]
        out, sec = b.generate_greedy([s.slot for s in rows], first, pos0, 5, timing=True)
        assert out.shape == (n, 5) and sec > 0
        for i, s in enumerate(rows):
            t, want = first[i], []
            for _ in range(5):
                t = ref_argmax(s.feed([t])); want.append(t)
            assert out[i].tolist() == want, f"{cfg} q{q} n {n}: row {i} (slot {s.slot} from {pos0[i]})"
            check_slot_rows(b, s, [pos0[i], pos0[i] + 2, pos0[i] + 4], f"{cfg} q{q} n {n}: rows left by generate")
    step(b, seqs[:20], [int(out[i, -1]) for i in range(20)], f"{cfg} q{q}: the step after generate")


# ---------------------------------------------------------------------------------------------- 4. ragged passes on a wide batch

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_ragged_passes_on_a_wide_batch(L, cfg, q):
    """40 runs in one call - 30 decode rows, 9 runs of 2 .. 5 tokens, a 20-token prompt: 30 + 31 + 20 = 81 rows (40 such runs hold 68 at the least), so the
    layers take the ring kernels and the classifier, with 33 rows asked for, the stream kernel; then 39 runs of 45 rows, the stream kernel in the layers
    too, 35 rows asked for.  n_out of 0, 1 and more; k = 5 on every row asked for."""
    img = S.build_image(cfg, q, seed=291)
    depths = [(0, 1, 7, 63, 64, 65, 100, 128, 129, 31)[i % 10] for i in range(40)]
    m, b, seqs = wide_prefilled(L, img, cfg, depths, 292, n_slots=64)
    lens = [1] * 30 + [2, 3, 4, 5, 2, 3, 4, 5, 3] + [20]
    n_out = [1] * 15 + [0] * 15 + [2, 0, 1, 5, 1, 3, 0, 2, 3] + [1]
    assert sum(lens) == 81 and len(lens) == 40
    work = [(s, toks_for(cfg, n, 300 + i), no) for i, (s, n, no) in enumerate(zip(seqs, lens, n_out))]
    ams, rows, (ti, tl) = run_pass(b, work, f"{cfg} q{q}: 40 runs, 81 rows", k=5, kv="ends")
    assert ti.shape == (sum(n_out), 5) and ti[:, 0].tolist() == np.concatenate(ams).tolist(), "rank 0 is the argmax"
    lens = [1] * 33 + [2, 3, 2, 3, 1, 1]
    n_out = [1] * 15 + [0] * 10 + [1] * 8 + [2, 3, 2, 3, 1, 1]
    assert sum(lens) == 45 and len(lens) == 39 and sum(n_out) == 35
    work = [(s, toks_for(cfg, n, 400 + i), no) for i, (s, n, no) in enumerate(zip(seqs[::-1][1:], lens, n_out))]
    ams, rows, (ti, tl) = run_pass(b, work, f"{cfg} q{q}: 39 runs, 45 rows", k=5, kv="ends")
    assert ti.shape == (35, 5) and ti[:, 0].tolist() == np.concatenate(ams).tolist()


# ---------------------------------------------------------------------------------------------- 5. slots

@gpu
def test_slots_above_15_and_31(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=293)
    m = L.Transformer(img); b = L.Batch(m, 64, wide=True)
    nl = m.args.n_layers
    seqs = {i: Seq(img, i) for i in (3, 8, 40, 50, 63)}
    for i in (3, 8, 40):
        toks = S.prompt_tokens(cfg, 10 + i, 294 + i)
        b.prefill(i, toks, 0); seqs[i].feed(toks)
    step(b, [seqs[8], seqs[40]], [5, 6], "slots 8 and 40 in one call")          # 40 = 8 + 32: distinct bits of a 64-bit mask
    with pytest.raises(L.LmrsError, match="slot 40 appears twice"):
        b.forward([40, 8, 40], [1, 2, 3], [0, 0, 1])
    with pytest.raises(L.LmrsError, match="slot 40 appears in more than one run"):
        b.forward_runs([(40, 0, [1], 1), (8, 0, [2], 1), (40, 1, [3], 1)])
    step(b, [seqs[40], seqs[8]], [7, 8], "the valid call after the refusals")
    pc = S.prompt_tokens(cfg, 20, 299)
    assert m.prefill_tokens(pc, 0) == 20
    b.fork(3, 50, 9); seqs[50].feed(S.prompt_tokens(cfg, 13, 297)[:9])
    b.fork(L.BATCH_CTX, 63, 13); seqs[63].feed(pc[:13])
    for s in (seqs[50], seqs[63]):
        check_slot_rows(b, s, [0, s.n // 2, s.n - 1], "forked rows")
    assert_bit_equal(b.kv_row(63, 1, nl - 1, 12), seqs[63].orc.kv_row(1, nl - 1, 12), "kv_row(63, ..)")
    step(b, [seqs[63], seqs[3], seqs[50]], [100, 101, 102], "continuation after fork")
    with pytest.raises(L.LmrsError, match="slot 64 of 64"):
        b.kv_row(64, 0, 0, 0)
    with pytest.raises(L.LmrsError, match="slots"):
        b.fork(0, 64, 4)


# ---------------------------------------------------------------------------------------------- 6. limits

@gpu
def test_limits_of_a_wide_batch(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=295)
    m = L.Transformer(img)
    for n_slots in (0, 65):
        with pytest.raises(L.LmrsError, match=r"lmrs_batch_create_wide: n_slots = \d+ is outside 1 \.\. 64"):
            L.Batch(m, n_slots, wide=True)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_create: n_slots = 17 is outside 1 \.\. 16"):
        L.Batch(m, 17)
    m2, b, seqs = wide_prefilled(L, img, cfg, [6, 0, 3] + [0] * 61, 296)
    k = [0]

    def good():
        step(b, seqs[:18], [50 + k[0] + i for i in range(18)], f"the valid call after refusal {k[0]}")
        k[0] += 1

    rows65 = ([i % 64 for i in range(65)], [1] * 65, [0] * 65)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward: n = 65 is outside 1 \.\. 64"):
        b.forward(*rows65)
    good()
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_generate_greedy: n = 65 is outside 1 \.\. 64"):
        b.generate_greedy(*rows65, 3)
    good()
    with pytest.raises(L.LmrsError, match=r"n_runs = 65 is outside 1 \.\. 64"):
        b.forward_runs([(i % 64, 0, [1], 1) for i in range(65)])
    good()
    T = m.args.seq_len
    with pytest.raises(L.LmrsError, match="seq_len"):
        b.generate_greedy(list(range(20)), [1] * 20, [T - 3] + [0] * 19, 5)
    good()
    # the sampled step keeps 16 rows on any batch ...
    samplers = [L.Sampler(m.args.vocab_size, 0.8, 0.9 if i % 2 else 1.0, 100 + i) for i in range(17)]
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward_sample: n = 17 is outside 1 \.\. 16"):
        b.forward_sample(list(range(20, 37)), [3] * 17, [0] * 17, samplers)
    good()
    # ... and with 16 it gives lmrs_forward_sample's tokens: slots 20 .. 35 are empty, every row is token 3 + i at position 0
    got = b.forward_sample(list(range(20, 36)), [3 + i for i in range(16)], [0] * 16, samplers[:16])
    own = L.Transformer(img)
    ref = [L.Sampler(m.args.vocab_size, 0.8, 0.9 if i % 2 else 1.0, 100 + i) for i in range(16)]
    assert got.tolist() == [own.forward_sample(3 + i, 0, ref[i]) for i in range(16)]
    good()
    # an ordinary batch keeps its limits and messages
    b16 = L.Batch(m, 16)
    assert b16.width == 16
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward: n = 17 is outside 1 \.\. 16"):
        b16.forward(list(range(17)), [1] * 17, [0] * 17)
    with pytest.raises(L.LmrsError, match=r"n_runs = 17 is outside 1 \.\. 16"):
        b16.forward_runs([(i % 16, 0, [1], 1) for i in range(17)])
    lib = L.lib()
    h = ctypes.c_void_p(); w = ctypes.c_uint32()
    assert lib.lmrs_batch_create_wide(None, 2, ctypes.byref(h)) != 0 and "NULL" in lib.lmrs_last_error().decode()
    assert lib.lmrs_batch_width(None, ctypes.byref(w)) != 0 and "NULL" in lib.lmrs_last_error().decode()
    assert lib.lmrs_batch_width(b._h, None) != 0 and "NULL" in lib.lmrs_last_error().decode()
    good()


@gpu
def test_create_wide_refuses_contexts_without_the_pass(L, monkeypatch):
    """tests/test_batch.py::test_create_refuses_contexts_without_the_pass for lmrs_batch_create_wide: a message each, every one under this call's name"""
    seen = set()

    def refused(m, match):
        with pytest.raises(L.LmrsError, match=match) as e:
            L.Batch(m, 40, wide=True)
        assert str(e.value).startswith("lmrs_batch_create_wide: ")
        seen.add(str(e.value))

    img = S.build_image("mini-llama", S.Q8_0, seed=93)
    refused(L.Transformer(S.build_image("mini-llama", S.Q_NONE, seed=93)), "f32")
    refused(L.Transformer(S.build_image("mini-gemma9b", S.Q8_0, seed=93)), "geometry")
    refused(L.Transformer(S.build_image("mini-llama-v4102", S.Q8_0, seed=93)), "multiple of 16")
    monkeypatch.setenv("LMRS_NO_BATCHED_PREFILL", "1")
    off = L.Transformer(img)
    monkeypatch.delenv("LMRS_NO_BATCHED_PREFILL")
    refused(off, "LMRS_NO_BATCHED_PREFILL")
    refused(L.Transformer(img, rank=0, world=1, unique_id=L.comm_unique_id()), "sharded")
    grp = L.ShardGroup(img, 2)
    h = ctypes.c_void_p()
    assert L.lib().lmrs_batch_create_wide(grp._arr[0], 40, ctypes.byref(h)) != 0 and not h.value
    msg = L.lib().lmrs_last_error().decode()
    assert "group" in msg and msg.startswith("lmrs_batch_create_wide: ")
    seen.add(msg)
    grp.close()
    assert len(seen) == 6, "a distinct message each"
    m = L.Transformer(img)                                     # ... and a context that takes one still does, bit-exact
    b = L.Batch(m, 40, wide=True)
    step(b, [Seq(img, 39)], [5], "after the refusals")


# ---------------------------------------------------------------------------------------------- 7. 16 rows or fewer on a wide batch

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_narrow_calls_on_a_wide_batch(L, cfg, q):
    """three steps with 3 rows and three with 16 on slots spread over the 64: the row-table path of an ordinary batch on the wider allocation"""
    img = S.build_image(cfg, q, seed=297)
    slots = [60, 2, 33, 17, 63, 31, 32, 0, 48, 5, 21, 40, 9, 55, 12, 26]
    m = L.Transformer(img); b = L.Batch(m, 64, wide=True)
    seqs = []
    for i, slot in enumerate(slots):
        s = Seq(img, slot)
        n = (65, 0, 128, 7, 64, 1)[i % 6]
        if n:
            toks = S.prompt_tokens(cfg, n, 298 + i)
            b.prefill(slot, toks, 0); s.feed(toks)
        seqs.append(s)
    V = m.args.vocab_size
    for k in range(3):
        step(b, seqs[:3], [(11 * i + k + 2) % V for i in range(3)], f"{cfg} q{q}: 3 rows, step {k}")
    for k in range(3):
        step(b, seqs, [(17 * i + k + 4) % V for i in range(16)], f"{cfg} q{q}: 16 rows, step {k}")
    out = b.generate_greedy([s.slot for s in seqs], [9] * 16, [s.n for s in seqs], 3)
    for i, s in enumerate(seqs):
        t, want = 9, []
        for _ in range(3):
            t = ref_argmax(s.feed([t])); want.append(t)
        assert out[i].tolist() == want, f"{cfg} q{q}: generate over 16 rows, row {i}"


# ---------------------------------------------------------------------------------------------- 8. interleaving

@gpu
def test_wide_batch_context_and_ordinary_batch_interleave(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=299)
    m, b, seqs = wide_prefilled(L, img, cfg, [12, 0, 66] + [i % 5 for i in range(21)], 300, n_slots=24)
    b16 = L.Batch(m, 3)
    narrow = [Seq(img, i) for i in range(3)]
    own = Seq(img, None)                                       # the context's sequence: an oracle that never sees a batch
    nl = own.orc.args.n_layers

    def check_own(what):
        for layer in range(nl):
            for p in sorted({0, own.n // 2, own.n - 1}):
                for w in (0, 1):
                    assert_bit_equal(m.kv_row(w, layer, p), own.orc.kv_row(w, layer, p), f"{what}: the context's {'kv'[w]} row layer {layer} pos {p}")

    assert_bit_equal(m.forward(5, 0), own.feed([5]), "forward before any step")
    step(b, seqs, [1 + i for i in range(24)], "wide step 0")
    step(b16, narrow, [4, 5, 6], "ordinary batch step 0")
    snap = {s.slot: snapshot(b, s.slot, range(s.n), nl) for s in seqs[:4]}
    assert_bit_equal(m.forward(6, 1), own.feed([6]), "forward between steps")
    toks = np.array([7, 8, 9, 10, 11], np.uint32)
    am, _ = m.verify_tokens(toks, own.n)
    assert am.tolist() == [ref_argmax(own.feed([t])) for t in toks], "verify_tokens between steps"
    for s in seqs[:4]:
        for x, y in zip(snap[s.slot], snapshot(b, s.slot, range(s.n), nl)):
            assert_bit_equal(x, y, f"slot {s.slot} moved by a context call")
    step(b, seqs[::-1], [30 + i for i in range(24)], "wide step 1")
    check_own("after wide step 1")
    prompt = S.prompt_tokens(cfg, 10, 301)
    got = m.generate_greedy(prompt, 6, own.n)
    assert got.tolist() == own.orc.generate_greedy(prompt, 6, own.n).tolist(), "generate_greedy between steps"
    own.n += 10 + 5
    step(b16, narrow[::-1], [7, 8, 9], "ordinary batch step 1")
    out = b.generate_greedy([s.slot for s in seqs[:20]], [9] * 20, [s.n for s in seqs[:20]], 3)
    for i, s in enumerate(seqs[:20]):
        t, w = 9, []
        for _ in range(3):
            t = ref_argmax(s.feed([t])); w.append(t)
        assert out[i].tolist() == w
    check_own("after the wide batch's generate_greedy")
    assert_bit_equal(m.forward(3, own.n), own.feed([3]), "forward after everything")
    step(b16, narrow, [1, 2, 3], "ordinary batch step 2")
    step(b, seqs, [60 + i for i in range(24)], "wide step 2")
