"""lmrs_batch_* (include/lmrs_hip.h): up to 16 sequences a step over one copy of the weights, each on a K/V cache of its own.  The reference is one
CPU oracle PER SEQUENCE running the sequential forward (one call per token, transformer.rs:316-384) with lmrs_ref_argmax: every comparison - argmax,
logits, K/V rows - is bit for bit."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from tools import synth_lmrs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

CFGS = [("mini-llama", S.Q8_0), ("mini-llama", S.Q4_0), ("mini-phi", S.Q8_0), ("mini-llama3b", S.Q8_0), ("mini-gemma", S.Q8_0), ("mini-gemma", S.Q4_0)]
NAMES = ("lmrs_batch_create", "lmrs_batch_destroy", "lmrs_batch_prefill", "lmrs_batch_fork", "lmrs_batch_forward", "lmrs_batch_generate_greedy",
         "lmrs_batch_debug_kv")


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


class Seq:
    """one sequence: its slot, its own oracle, the tokens fed so far"""

    def __init__(self, img, slot):
        self.slot, self.orc, self.n = slot, O.Oracle(img), 0

    def feed(self, toks):
        """the oracle's sequential forward over toks from the sequence's end -> the last logits"""
        lg = None
        for t in toks:
            lg = self.orc.forward(int(t), self.n).copy()
            self.n += 1
        return lg


def check_slot_rows(b, s, positions, what):
    """K and V rows of every layer of slot s.slot at `positions`, against the sequence's oracle"""
    for layer in range(s.orc.args.n_layers):
        for p in positions:
            for which in (0, 1):
                assert_bit_equal(b.kv_row(s.slot, which, layer, p), s.orc.kv_row(which, layer, p), f"{what}: slot {s.slot} {'kv'[which]} layer {layer} pos {p}")


def snapshot(b, slot, positions, n_layers):
    return [b.kv_row(slot, w, l, p).copy() for l in range(n_layers) for p in positions for w in (0, 1)]


def step(b, seqs, toks, what, logits=True):
    """one batch_forward over `seqs` (in that order) feeding toks[i] at each sequence's end, judged against the oracles -> the argmax"""
    pos = [s.n for s in seqs]
    got = b.forward([s.slot for s in seqs], toks, pos, logits=logits)
    am, lg = got if logits else (got, None)
    for i, s in enumerate(seqs):
        want = s.feed([toks[i]])
        assert int(am[i]) == ref_argmax(want), f"{what}: row {i} (slot {s.slot}, pos {pos[i]}): argmax"
        if logits:
            assert_bit_equal(lg[i], want, f"{what}: row {i} (slot {s.slot}, pos {pos[i]}): logits")
        check_slot_rows(b, s, [pos[i]], what)
    return am


def prefilled(L, img, cfg, lengths, seed, n_slots=None):
    """a model, a batch and one Seq per length, slot i prefilled with lengths[i] tokens (batch.prefill; the oracle token by token)"""
    m = L.Transformer(img)
    b = L.Batch(m, n_slots or len(lengths))
    seqs = []
    for i, n in enumerate(lengths):
        s = Seq(img, i)
        if n:
            toks = S.prompt_tokens(cfg, n, seed + i)
            assert b.prefill(i, toks, 0) == n
            s.feed(toks)
        seqs.append(s)
    return m, b, seqs


# ---------------------------------------------------------------------------------------------- 1. rows at different depths in one pass

# the positions the attention forms change at (one wave's 64 keys, the 128 / 256-key passes), both sides of each, and the ends of the fixtures' 256 positions
DEPTHS3 = [65, 0, 128]
DEPTHS16 = [0, 1, 7, 63, 64, 65, 127, 128, 129, 200, 252, 2, 31, 32, 33, 96]


@gpu
@pytest.mark.parametrize("n_slots", [3, 16])
@pytest.mark.parametrize("cfg,q", CFGS)
def test_rows_at_different_depths_in_one_pass(L, cfg, q, n_slots):
    img = S.build_image(cfg, q, seed=71)
    lengths = DEPTHS3 if n_slots == 3 else DEPTHS16
    m, b, seqs = prefilled(L, img, cfg, lengths, 72)
    for s in seqs:
        check_slot_rows(b, s, sorted({0, s.n // 2, s.n - 1}) if s.n else [], f"{cfg} q{q}: prefill of {s.n}")
    V = seqs[0].orc.args.vocab_size
    for k in range(3):
        toks = [(13 * i + 5 * k + 3) % V for i in range(n_slots)]
        step(b, seqs, toks, f"{cfg} q{q} n {n_slots} step {k}")


@gpu
def test_a_row_beyond_384_positions(L):
    """mini-llama with 512 positions: a slot at 400 (the decode step's split attention would start at 384) beside slots at 0 and 255 .. 257"""
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-512", max_pos=512)
    img = S.build_image(cfg, S.Q8_0, seed=73)
    m, b, seqs = prefilled(L, img, cfg, [255, 400, 0, 256, 257], 74)
    for k in range(3):
        step(b, seqs, [17 + k, 5, 900 + k, 3, 77], f"512 positions step {k}")


# ---------------------------------------------------------------------------------------------- 2. subsets and order, 3. n = 1

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_subsets_and_order(L, cfg, q):
    img = S.build_image(cfg, q, seed=75)
    m, b, seqs = prefilled(L, img, cfg, [9, 0, 70, 3, 130], 76)
    nl = seqs[0].orc.args.n_layers
    for k, pick in enumerate(([3, 0], [1], [4, 2, 0])):
        rest = [s for s in seqs if s.slot not in pick]
        before = {s.slot: snapshot(b, s.slot, range(s.n + 1), nl) for s in rest}
        step(b, [seqs[i] for i in pick], [40 + 7 * k + i for i in pick], f"{cfg} q{q} slots {pick}")
        for s in rest:
            for x, y in zip(before[s.slot], snapshot(b, s.slot, range(s.n + 1), nl)):
                assert_bit_equal(x, y, f"{cfg} q{q}: slot {s.slot} untouched by a step over {pick}")


@gpu
@pytest.mark.parametrize("cfg,q", CFGS)
def test_one_row_goes_through_the_pass(L, cfg, q):
    """n = 1 (and a one-token prefill) is the same pass: a sequence built from single rows only"""
    img = S.build_image(cfg, q, seed=77)
    m = L.Transformer(img); b = L.Batch(m, 2); s = Seq(img, 1)
    assert b.prefill(1, [21], 0) == 1
    s.feed([21])
    check_slot_rows(b, s, [0], f"{cfg} q{q}: one-token prefill")
    for k in range(3):
        step(b, [s], [30 + k], f"{cfg} q{q} single row {k}")


# ---------------------------------------------------------------------------------------------- 4. Gemma's window per row

@gpu
def test_gemma_window_is_tested_per_row():
    """mini-gemma's geometry with 4352 positions (the recipe of tests/test_prefill_tokens.py): slot 0 stands at 4100 - its queries mask keys
    0 .. pos - 4097 - and is stepped in the same passes as slot 1 at position 3, which masks none."""
    import lmrs_amd as L
    cfg = dataclasses.replace(S.CONFIGS["mini-gemma"], name="mini-gemma-window", max_pos=4352)
    img = S.build_image(cfg, S.Q8_0, 29)
    m, b, seqs = prefilled(L, img, cfg, [4100, 3], 29)
    check_slot_rows(b, seqs[0], [0, 2040, 4095, 4096, 4099], "window: prefill")
    for k in range(2):
        step(b, seqs, [50 + k, 60 + k], f"window step {k}")
        step(b, seqs[::-1], [70 + k, 80 + k], f"window step {k}, the shallow row first")


# ---------------------------------------------------------------------------------------------- 5. the context's own cache is a private sequence

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q8_0)])
def test_context_and_batch_calls_interleave(L, cfg, q):
    img = S.build_image(cfg, q, seed=79)
    m, b, seqs = prefilled(L, img, cfg, [12, 0, 66], 80)
    own = Seq(img, None)                                     # the context's sequence: an oracle that never sees the batch
    V, nl = own.orc.args.vocab_size, own.orc.args.n_layers

    def check_own(what):
        for layer in range(nl):
            for p in sorted({0, own.n // 2, own.n - 1}):
                for w in (0, 1):
                    assert_bit_equal(m.kv_row(w, layer, p), own.orc.kv_row(w, layer, p), f"{what}: the context's {'kv'[w]} row layer {layer} pos {p}")

    def slots_before():
        return {s.slot: snapshot(b, s.slot, range(s.n), nl) for s in seqs}

    def slots_unmoved(before, what):
        for s in seqs:
            for x, y in zip(before[s.slot], snapshot(b, s.slot, range(s.n), nl)):
                assert_bit_equal(x, y, f"{what}: slot {s.slot} moved by a context call")

    assert_bit_equal(m.forward(5, 0), own.feed([5]), "forward before any step")
    step(b, seqs, [1, 2, 3], "step 0")
    snap = slots_before()
    assert_bit_equal(m.forward(6, 1), own.feed([6]), "forward between steps")
    toks = np.array([7, 8, 9, 10, 11], np.uint32)
    am, _ = m.verify_tokens(toks, own.n)
    want = []
    for t in toks:
        want.append(ref_argmax(own.feed([t])))
    assert am.tolist() == want, "verify_tokens between steps"
    slots_unmoved(snap, "forward + verify_tokens")
    step(b, seqs[::-1], [4, 5, 6], "step 1")
    check_own("after step 1")
    snap = slots_before()
    prompt = S.prompt_tokens(cfg, 10, 81)
    got = m.generate_greedy(prompt, 6, own.n)
    ref = own.orc.generate_greedy(prompt, 6, own.n)
    assert got.tolist() == ref.tolist(), "generate_greedy between steps"
    own.n += 10 + 5
    slots_unmoved(snap, "generate_greedy")
    out = b.generate_greedy([0, 2], [9, 9], [seqs[0].n, seqs[2].n], 4)
    for i, s in zip((0, 1), (seqs[0], seqs[2])):
        t, w = 9, []
        for _ in range(4):
            t = ref_argmax(s.feed([t])); w.append(t)
        assert out[i].tolist() == w
    check_own("after the batch's generate_greedy")
    assert_bit_equal(m.forward(3 % V, own.n), own.feed([3 % V]), "forward after everything")
    step(b, seqs, [7, 7, 7], "step 2")


# ---------------------------------------------------------------------------------------------- 6. fork

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_fork(L, cfg, q):
    img = S.build_image(cfg, q, seed=83)
    m = L.Transformer(img); b = L.Batch(m, 5)
    nl = m.args.n_layers
    pa, pc = S.prompt_tokens(cfg, 20, 84), S.prompt_tokens(cfg, 20, 85)
    assert b.prefill(0, pa, 0) == 20 and m.prefill_tokens(pc, 0) == 20
    for dst in (1, 2, 3, 4):                                   # former contents of the destinations: rows 0 .. 19 of another run
        b.prefill(dst, S.prompt_tokens(cfg, 20, 90 + dst), 0)
    old = {dst: snapshot(b, dst, range(13, 20), nl) for dst in (1, 2, 3, 4)}
    for dst in (1, 2, 3):
        b.fork(0, dst, 13)
    b.fork(L.BATCH_CTX, 4, 13)
    for dst in (1, 2, 3, 4):
        for x, y in zip(old[dst], snapshot(b, dst, range(13, 20), nl)):
            assert_bit_equal(x, y, f"fork into {dst}: rows >= n_pos keep their bits")
    seqs = []
    for slot in range(5):
        s = Seq(img, slot)
        s.feed(pa if slot == 0 else (pc[:13] if slot == 4 else pa[:13]))
        seqs.append(s)
        check_slot_rows(b, s, [0, 6, 12], f"{cfg} q{q}: forked rows")
    for k in range(3):
        step(b, seqs, [100 + 11 * s.slot + k for s in seqs], f"{cfg} q{q}: continuation {k} after fork")
    own = Seq(img, None); own.feed(pc)
    assert_bit_equal(m.forward(2, 20), own.feed([2]), "the context after being a fork's source")


# ---------------------------------------------------------------------------------------------- 7. generate

@gpu
@pytest.mark.parametrize("cfg,q", CFGS)
def test_generate_greedy(L, cfg, q):
    img = S.build_image(cfg, q, seed=87)
    m, b, seqs = prefilled(L, img, cfg, [0, 5, 60, 121], 88, n_slots=6)
    rows = [seqs[2], seqs[0], seqs[3], seqs[1]]
    first = [3, 400, 77, 1000]
    pos0 = [s.n for s in rows]
    out, sec = b.generate_greedy([s.slot for s in rows], first, pos0, 12, timing=True)
    assert out.shape == (4, 12) and sec > 0
    for i, s in enumerate(rows):
        t, want = first[i], []
        for _ in range(12):
            t = ref_argmax(s.feed([t])); want.append(t)
        assert out[i].tolist() == want, f"{cfg} q{q}: row {i} (slot {s.slot} from {pos0[i]})"
        check_slot_rows(b, s, [pos0[i], pos0[i] + 6, pos0[i] + 11], f"{cfg} q{q}: rows left by generate")
    step(b, rows, [int(out[i, -1]) for i in range(4)], f"{cfg} q{q}: the step after generate")


# ---------------------------------------------------------------------------------------------- 8. stale rows

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q8_0)])
def test_stale_rows_are_not_seen(L, cfg, q):
    """a slot stepped at p + 2, then at p: a later step at p + 1 sees rows 0 .. p + 1 only, whatever p + 2 holds"""
    img = S.build_image(cfg, q, seed=89)
    m, b, seqs = prefilled(L, img, cfg, [66, 4], 90)
    s, other = seqs
    p = s.n
    b.forward([0, 1], [9, 9], [p + 2, other.n])               # garbage at p + 2 (rows p, p + 1 are unwritten zeros there)
    other.feed([9])
    step(b, [s, other], [31, 32], "step at p")
    step(b, [other, s], [33, 34], "step at p + 1")
    step(b, [s], [35], "step at p + 2: the stale row is rewritten")


# ---------------------------------------------------------------------------------------------- 9. errors

@gpu
def test_errors_are_reported_before_device_work(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=91)
    m, b, seqs = prefilled(L, img, cfg, [6, 0, 0], 92)
    V, T = m.args.vocab_size, m.args.seq_len
    lib = L.lib()
    k = [0]

    def good():
        step(b, seqs[:2], [50 + k[0], 60 + k[0]], f"the valid call after refusal {k[0]}", logits=k[0] % 4 == 0)
        k[0] += 1

    for n_slots in (0, 17):
        with pytest.raises(L.LmrsError, match="n_slots"):
            L.Batch(m, n_slots)
    for args, msg in ((([0, 3], [1, 2], [0, 0]), "slot 3 of 3"), (([0, 0], [1, 2], [6, 7]), "appears twice"), (([0, 1], [1, V], [6, 0]), "out of range"),
                      (([0, 1], [1, 2], [6, T]), "seq_len"), ((list(range(17)), [1] * 17, [0] * 17), "outside 1 .. 16")):
        with pytest.raises(L.LmrsError, match=msg):
            b.forward(*args)
        good()
        with pytest.raises(L.LmrsError, match=msg):
            b.generate_greedy(*args, 3)
        good()
    with pytest.raises(L.LmrsError, match="seq_len"):
        b.generate_greedy([0, 2], [1, 2], [6, T - 3], 5)       # pos + n_new - 1 = T + 1
    b.generate_greedy([2], [1], [T - 3], 3)                    # ... and the last position is allowed
    good()
    for slot, toks, start, msg in ((3, [1, 2], 0, "slot 3 of 3"), (0, [1, V], 0, "out of range"), (0, [1, 2, 3], T - 2, "seq_len"), (0, [], 0, "no tokens")):
        with pytest.raises(L.LmrsError, match=msg):
            b.prefill(slot, toks, start)
        good()
    for src, dst, n_pos, msg in ((0, 0, 4, "same slot"), (0, 1, T + 1, "seq_len"), (3, 1, 4, "slots"), (0, 3, 4, "slots"), (L.BATCH_CTX, 5, 4, "slots")):
        with pytest.raises(L.LmrsError, match=msg):
            b.fork(src, dst, n_pos)
        good()
    with pytest.raises(L.LmrsError, match="slot 3 of 3"):
        b.kv_row(3, 0, 0, 0)
    a3 = np.zeros(3, np.uint32); h = ctypes.c_void_p()
    p3 = a3.ctypes.data
    null_calls = (lambda: lib.lmrs_batch_create(None, 2, ctypes.byref(h)), lambda: lib.lmrs_batch_create(m._h, 2, None),
                  lambda: lib.lmrs_batch_forward(None, 1, p3, p3, p3, p3, None), lambda: lib.lmrs_batch_forward(b._h, 1, None, p3, p3, p3, None),
                  lambda: lib.lmrs_batch_forward(b._h, 1, p3, None, p3, p3, None), lambda: lib.lmrs_batch_forward(b._h, 1, p3, p3, None, p3, None),
                  lambda: lib.lmrs_batch_forward(b._h, 1, p3, p3, p3, None, None), lambda: lib.lmrs_batch_generate_greedy(b._h, 1, p3, p3, p3, 2, None, None),
                  lambda: lib.lmrs_batch_generate_greedy(None, 1, p3, p3, p3, 2, p3, None), lambda: lib.lmrs_batch_prefill(None, 0, p3, 2, 0),
                  lambda: lib.lmrs_batch_prefill(b._h, 0, None, 2, 0), lambda: lib.lmrs_batch_fork(None, 0, 1, 2), lambda: lib.lmrs_batch_debug_kv(b._h, 0, 0, 0, 0, None))
    for call in null_calls:
        assert call() != 0 and "NULL" in lib.lmrs_last_error().decode()
    lib.lmrs_batch_destroy(None)
    good()


@gpu
def test_create_refuses_contexts_without_the_pass(L, monkeypatch):
    seen = set()

    def refused(m, match):
        with pytest.raises(L.LmrsError, match=match) as e:
            L.Batch(m, 2)
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
    assert L.lib().lmrs_batch_create(grp._arr[0], 2, ctypes.byref(h)) != 0 and not h.value
    msg = L.lib().lmrs_last_error().decode()
    assert "group" in msg
    seen.add(msg)
    grp.close()
    assert len(seen) == 6, "a distinct message each"
    m = L.Transformer(img)                                     # ... and a context that takes one still does, bit-exact
    b = L.Batch(m, 1)
    step(b, [Seq(img, 0)], [5], "after the refusals")


# ---------------------------------------------------------------------------------------------- 10. resources, ABI presence (no GPU)

def _collect_new_kernels():
    import shutil
    pytest.importorskip("yaml", reason="PyYAML is needed to read the code objects' metadata")
    from tools import kernel_resources as KR
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(KR.LLVM, tool)):
            pytest.skip(f"{tool} not found under {KR.LLVM}")
    if not shutil.which("c++filt"):
        pytest.skip("c++filt not found")
    import lmrs_amd
    lmrs_amd.build()
    return KR, KR.collect(hot_only=False)


def test_new_kernels_have_no_scratch_and_the_tables_have_not_moved():
    KR, rows = _collect_new_kernels()
    new = {n: r for n, r in rows.items() if re.search(r"rope_scatter_rows_kernel|attention_table_kernel|table_advance_kernel", n)}
    # RoPE + scatter, the advance, attention over the table for head sizes 64 / 96 / 128 and Gemma's 256
    assert len(new) == 6, sorted(new)
    for n, r in new.items():
        # (the gate of tests/test_skinny_resources.py: scratch bytes and spilled VGPRs)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{n}: scratch {r['scratch']} bytes per lane, spilled VGPRs {r['vgpr_spill']}"
        assert not KR.HOT.match(n), f"{n} must not enter the hot table"
        if "attention_table_kernel" in n:
            # the body is attention_rows_kernel's, so are its registers - Gemma's form included, whose f64 tanh parks SGPRs in VGPR lanes there too
            twin = rows[n.replace("attention_table_kernel", "attention_rows_kernel")]
            assert (r["sgpr_spill"], r["waves_per_simd"]) == (twin["sgpr_spill"], twin["waves_per_simd"]) and abs(r["vgpr"] - twin["vgpr"]) <= 16, f"{n}: {r} vs {twin}"
        else:
            assert r["sgpr_spill"] == 0, f"{n}: spilled SGPRs {r['sgpr_spill']}"
    import json
    hot = json.load(open(KR.TABLE))
    assert set(hot) == {n for n in rows if KR.HOT.match(n)}, "the hot table's kernel classes moved"
    skinny = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_skinny.json")))
    assert set(skinny) == {n for n in rows if "gemm_skinny_kernel" in n}, "the skinny table's kernel classes moved"
    for table in (hot, skinny):
        for n, w in table.items():
            g = rows[n]
            assert (g["scratch"], g["vgpr_spill"], g["waves_per_simd"]) == (w["scratch"], w["vgpr_spill"], w["waves_per_simd"]), f"{n}: {w} -> {g}"


def test_entry_points_exist_in_every_layer(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in L.EXPORTS
        assert re.search(rf"\b(int|void)\s+{name}\(", header), f"{name} is not declared in the header"
        assert re.search(rf"\bpub fn {name}\(", ffi), f"{name} is not declared in the Rust crate"
        assert name in hpp, f"{name} is not mirrored in transformer.hpp"
    for method in ("prefill", "fork", "forward", "generate_greedy", "debug_kv"):
        assert callable(getattr(L.Batch, method))
    assert L.BATCH_CTX == 0xFFFFFFFF and re.search(r"#define LMRS_BATCH_CTX 0xFFFFFFFFu", header)


def test_rust_batch_externs_match_the_header():
    """tests/test_rust_crate.py::test_every_extern_declaration_matches_the_header for the batch block of ffi.rs (that test reads the crate's first
    extern block and has no mapping for the batch handle): name, arity, every argument type and the return type against include/lmrs_hip.h"""
    import test_rust_crate as R
    cmap = dict(R.CMAP)
    cmap.update({"lmrs_batch*": "*mut LmrsBatch", "lmrs_batch**": "*mut *mut LmrsBatch"})
    c = R.c_prototypes()
    txt = re.sub(r"//[^\n]*", " ", open(os.path.join(R.CRATE, "src", "ffi.rs")).read())
    blocks = re.findall(r'extern\s+"C"\s*\{(.*?)\n\}', txt, flags=re.S)
    assert len(blocks) == 2 and "lmrs_batch" not in blocks[0], "the batch declarations have a block of their own, the second"
    got = {}
    for m in re.finditer(r"pub\s+fn\s+(\w+)\s*\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", blocks[1], flags=re.S):
        args = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in m.group(2).split(",") if a.strip()]
        got[m.group(1)] = (re.sub(r"\s+", " ", (m.group(3) or "()").strip()), args)
    assert set(got) == set(NAMES), sorted(set(got) ^ set(NAMES))
    for name, (rret, rargs) in got.items():
        cret, cargs = c[name]
        assert len(cargs) == len(rargs), f"{name}: {len(rargs)} arguments in Rust, {len(cargs)} in C ({cargs})"
        assert cmap[cret] == rret, f"{name}: returns {rret} in Rust, {cret} in C"
        for i, (ca, ra) in enumerate(zip(cargs, rargs)):
            assert ca in cmap, f"{name}: no Rust mapping for C type '{ca}'"
            assert cmap[ca] == ra, f"{name}: argument {i} is {ra} in Rust, {ca} in C"
    assert re.search(r"pub struct LmrsBatch\b", txt)
