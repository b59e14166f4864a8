"""lmrs_batch_forward_runs (include/lmrs_hip.h): one weight pass whose rows are RUNS - consecutive tokens of one slot - of up to 16 sequences, outputs
only for the rows asked for.  The reference is one CPU oracle PER SEQUENCE fed token by token (tests/test_batch.py's Seq); every comparison - argmax,
logits, K/V rows - is bit for bit (tests/parity_rules.py)."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from parity_rules import assert_bit_equal, ref_argmax, run_positions
from test_batch import CFGS, Seq, check_slot_rows, prefilled, snapshot
from test_topk import rank_row
from tools import synth_lmrs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
NEW_KERNELS = r"rope_scatter_runs_kernel|attention_runs_kernel|select_rows_kernel"


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def run_pass(b, work, what, k=0, kv="all"):
    """One forward_runs over work = [(Seq, tokens, n_out), ...], every run starting at its sequence's end, with logits on; the oracles are fed the same
    tokens one by one.  Checks argmax and logits of every requested row and the K/V rows the runs left (kv: "all" positions of a run, or "ends": first,
    middle, last) -> (argmax rows per run, the oracle's logits rows per run, the call's top-k results or None)"""
    runs = [(s.slot, s.n, list(toks), n_out) for s, toks, n_out in work]
    got = b.forward_runs(runs, k=k, logits=True)
    am, lg = got[0], got[1]
    assert am.shape == (sum(n for _, _, n in work),) and lg.shape[0] == am.size
    o, ams, rows = 0, [], []
    for s, toks, n_out in work:
        start = s.n
        want = [s.feed([t]) for t in toks]
        for j in range(len(toks) - n_out, len(toks)):
            where = f"{what}: slot {s.slot} pos {start + j} (output row {o})"
            assert int(am[o]) == ref_argmax(want[j]), f"{where}: argmax"
            assert_bit_equal(lg[o], want[j], f"{where}: logits")
            o += 1
        ams.append(am[o - n_out:o].copy()); rows.append(want)
        check_slot_rows(b, s, range(start, start + len(toks)) if kv == "all" else run_positions(start, len(toks)), what)
    return ams, rows, (got[2:] if k else None)


def toks_for(cfg, n, seed):
    return [int(t) for t in S.prompt_tokens(cfg, n, seed)]


# ---------------------------------------------------------------------------------------------- 1. mixed runs in a skinny pass

@gpu
@pytest.mark.parametrize("cfg,q", CFGS)
def test_mixed_runs_in_a_skinny_pass(L, cfg, q):
    """R = 16 rows as runs of 1, 4, 1, 7 and 3 on slots standing at 65, 0, 128, 61 and 252: the 7-row run covers 61 .. 67 (it crosses the 64-key chunk
    of the attention), the last run ends at 254; every row is returned.  A second pass continues every sequence."""
    img = S.build_image(cfg, q, seed=171)
    m, b, seqs = prefilled(L, img, cfg, [65, 0, 128, 61, 252], 172)
    lens = [1, 4, 1, 7, 3]
    work = [(s, toks_for(cfg, n, 180 + i), n) for i, (s, n) in enumerate(zip(seqs, lens))]
    run_pass(b, work, f"{cfg} q{q}: first pass")
    assert [s.n for s in seqs] == [66, 4, 129, 68, 255]
    work = [(s, toks_for(cfg, n, 190 + i), n) for i, (s, n) in enumerate(zip(seqs, [3, 1, 2, 1, 1]))]
    run_pass(b, work, f"{cfg} q{q}: second pass")


# ---------------------------------------------------------------------------------------------- 2. every GEMM form

# R -> run lengths: the full skinny tile, the first direct-kernel size, both sides of the ring switch (48), one row past a 64-token tile, a ragged multi-tile pass
FORMS = {16: [1, 5, 7, 3], 17: [2, 9, 1, 5], 47: [20, 1, 17, 9], 48: [21, 3, 24], 65: [30, 1, 25, 9], 130: [70, 3, 40, 16, 1]}
STARTS = [0, 63, 64, 5, 100]


@gpu
@pytest.mark.parametrize("R", sorted(FORMS))
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_every_gemm_form(L, cfg, q, R):
    lens = FORMS[R]
    assert sum(lens) == R and 3 <= len(lens) <= 5
    img = S.build_image(cfg, q, seed=173)
    m, b, seqs = prefilled(L, img, cfg, STARTS[:len(lens)], 174)
    n_out = [(n, 0, 1, n, 1)[i] for i, n in enumerate(lens)]              # every row, none, the last one
    work = [(s, toks_for(cfg, n, 200 + R + i), no) for i, (s, n, no) in enumerate(zip(seqs, lens, n_out))]
    run_pass(b, work, f"{cfg} q{q} R {R}", kv="ends")


# ---------------------------------------------------------------------------------------------- 3. single-token runs are lmrs_batch_forward's rows

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_single_token_runs_equal_batch_forward(L, cfg, q):
    img = S.build_image(cfg, q, seed=175)
    m, b, seqs = prefilled(L, img, cfg, [9, 0, 70, 3, 130, 64], 176)
    order = [seqs[i] for i in (3, 0, 5, 1, 4, 2)]
    toks = [41, 7, 300, 5, 77, 12]
    pos = [s.n for s in order]
    am1, lg1 = b.forward([s.slot for s in order], toks, pos, logits=True)
    am2, lg2 = b.forward_runs([(s.slot, s.n, [t], 1) for s, t in zip(order, toks)], logits=True)     # the same rows again: they rewrite what they read nothing of
    assert am1.tolist() == am2.tolist()
    assert_bit_equal(lg1, lg2, f"{cfg} q{q}: logits of the two calls")
    for i, s in enumerate(order):
        want = s.feed([toks[i]])
        assert int(am2[i]) == ref_argmax(want)
        assert_bit_equal(lg2[i], want, f"{cfg} q{q}: row {i} against its oracle")
        check_slot_rows(b, s, [pos[i]], f"{cfg} q{q}")


# ---------------------------------------------------------------------------------------------- 4. output selection and order

@gpu
def test_output_selection_and_order(L):
    """A run without outputs between runs with outputs; a call with no output at all (argmax = NULL); more than 16 output rows, so the classifier leaves
    the skinny form while the layers (R = 40 > 16) already have.  No fixture has a vocabulary large enough for the logits block to hold fewer than 512
    rows (sc_rows = 512 MiB / (vocab x 4) is far above 512 here), so the classifier's slab loop runs once in every test of this file."""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=177)
    m, b, seqs = prefilled(L, img, cfg, [10, 0, 70], 178)
    ams, _, _ = run_pass(b, [(seqs[0], toks_for(cfg, 3, 1), 2), (seqs[1], toks_for(cfg, 5, 2), 0), (seqs[2], toks_for(cfg, 2, 3), 1)], "n_out = 0 in the middle")
    assert [a.size for a in ams] == [2, 0, 1]
    # no outputs at all: K/V rows only, argmax may be NULL
    runs = [(s.slot, s.n, toks_for(cfg, n, 10 + s.slot), 0) for s, n in zip(seqs, (4, 1, 6))]
    lib = L.lib()
    sl, st, ln, no = (np.array([r[i] if i != 2 else len(r[2]) for r in runs], np.uint32) for i in (0, 1, 2, 3))
    tk = np.array([t for r in runs for t in r[2]], np.uint32)
    assert lib.lmrs_batch_forward_runs(b._h, 3, sl.ctypes.data, st.ctypes.data, ln.ctypes.data, no.ctypes.data, tk.ctypes.data, None, None, 0, None, None) == 0, \
        lib.lmrs_last_error().decode()
    for s, r in zip(seqs, runs):
        start = s.n
        s.feed(r[2])
        check_slot_rows(b, s, range(start, s.n), "O = 0")
    assert b.forward_runs([(0, seqs[0].n - 1, [tk[3]], 0)]).size == 0        # (Batch.forward_runs passes NULL too: slot 0's last row again)
    # O = 3 + 30 + 1 = 34 > 16
    ams, _, _ = run_pass(b, [(seqs[0], toks_for(cfg, 3, 21), 3), (seqs[1], toks_for(cfg, 36, 22), 30), (seqs[2], toks_for(cfg, 1, 23), 1)], "O = 34")
    assert [a.size for a in ams] == [3, 30, 1]


# ---------------------------------------------------------------------------------------------- 5. top-k

@gpu
@pytest.mark.parametrize("k", [1, 5, 256])
def test_topk_of_a_mixed_pass(L, k):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=179)
    depths = [12, 0, 66]
    m, b, seqs = prefilled(L, img, cfg, depths, 180)
    hist = [toks_for(cfg, n, 180 + i) if n else [] for i, n in enumerate(depths)]          # prefilled()'s prompts
    work = [(seqs[0], toks_for(cfg, 1, 31), 1), (seqs[1], toks_for(cfg, 4, 32), 4), (seqs[2], toks_for(cfg, 6, 33), 2)]
    ams, rows, (ti, tl) = run_pass(b, work, f"top-{k}", k=k)
    assert ti.shape == (7, k) and tl.shape == (7, k) and tl.dtype == np.float32
    assert ti[:, 0].tolist() == np.concatenate(ams).tolist(), "rank 0 is the argmax"
    own = L.Transformer(img)                                 # the same sequences, one at a time, on a context of its own
    o = 0
    for i, (s, toks, n_out) in enumerate(work):
        full = hist[i] + toks
        _, _, _, ti1, tl1, _ = own.score_topk(full, k, 0)
        for j in range(len(toks) - n_out, len(toks)):
            p = depths[i] + j
            assert ti[o].tolist() == rank_row(rows[i][j])[:k].tolist(), f"top-{k}: slot {s.slot} pos {p}: indices against the ranked oracle row"
            assert ti[o].tolist() == ti1[p].tolist()
            assert_bit_equal(tl[o], tl1[p], f"top-{k}: slot {s.slot} pos {p}: log-probabilities against score_topk")
            o += 1


# ---------------------------------------------------------------------------------------------- 6. drafts verified per sequence

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q8_0)])
def test_drafts_verified_per_sequence(L, cfg, q):
    """Three sequences with 4 drafts each behind their last confirmed token: the oracle's greedy continuation as it is, with draft 2 wrong, with draft 0
    wrong.  Every argmax row is the oracle's for the tokens fed; the next pass starts each sequence behind its accepted drafts and rewrites the stale rows."""
    img = S.build_image(cfg, q, seed=181)
    m, b, seqs = prefilled(L, img, cfg, [20, 62, 3], 182)
    V = m.args.vocab_size
    work, accept = [], []
    for i, s in enumerate(seqs):
        start, run = s.n, [40 + i]
        for _ in range(4):
            run.append(ref_argmax(s.feed([run[-1]])))         # the greedy continuation ...
        s.n = start                                            # ... then back: the pass below feeds the oracle again, position by position
        wrong = (None, 2, 0)[i]
        if wrong is not None:
            run[1 + wrong] = (run[1 + wrong] + 1) % V
        work.append((s, run, 5)); accept.append(4 if wrong is None else wrong)
    starts = [s.n for s in seqs]
    ams, _, _ = run_pass(b, work, f"{cfg} q{q}: verify")
    nxt = []
    for (s, run, _), am, acc, start in zip(work, ams, accept, starts):
        got = 0
        while got + 1 < len(run) and run[got + 1] == am[got]:
            got += 1
        assert got == acc, f"slot {s.slot}: {got} drafts accepted, {acc} expected"
        s.n = start + acc + 1                                  # rows behind it are stale in the slot (and in the oracle: both rewrite them next)
        nxt.append((s, [int(am[acc])] + toks_for(cfg, 2, 50 + s.slot), 3))
    run_pass(b, nxt, f"{cfg} q{q}: the pass behind the accepted drafts")
    for s, start in zip(seqs, starts):
        check_slot_rows(b, s, range(start, s.n), f"{cfg} q{q}: rows after the rewrite")


# ---------------------------------------------------------------------------------------------- 7. Gemma-2's window per row

@gpu
def test_gemma_window_inside_a_run():
    """test_batch.py's window model (mini-gemma with 4352 positions): a run over 4094 .. 4100 - its rows from 4097 on mask keys 0 .. pos - 4097, the
    earlier ones none - beside a run at position 3."""
    import lmrs_amd as L
    cfg = dataclasses.replace(S.CONFIGS["mini-gemma"], name="mini-gemma-window", max_pos=4352)
    img = S.build_image(cfg, S.Q8_0, 29)
    m, b, seqs = prefilled(L, img, cfg, [4094, 3], 29)
    run_pass(b, [(seqs[0], toks_for(cfg, 7, 61), 7), (seqs[1], toks_for(cfg, 2, 62), 2)], "window")
    run_pass(b, [(seqs[1], [9], 1), (seqs[0], [8, 7], 2)], "window, the shallow run first")


# ---------------------------------------------------------------------------------------------- 8. isolation

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_isolation_and_interleaving(L, cfg, q):
    img = S.build_image(cfg, q, seed=183)
    m, b, seqs = prefilled(L, img, cfg, [12, 0, 66, 30], 184)
    own = Seq(img, None)                                       # the context's own sequence
    nl = own.orc.args.n_layers
    assert_bit_equal(m.forward(5, 0), own.feed([5]), "forward before any pass")
    idle = seqs[3]
    before = snapshot(b, idle.slot, range(idle.n + 8), nl)
    run_pass(b, [(seqs[0], toks_for(cfg, 5, 1), 1), (seqs[1], toks_for(cfg, 20, 2), 0), (seqs[2], toks_for(cfg, 1, 3), 1)], "pass 0")
    for x, y in zip(before, snapshot(b, idle.slot, range(idle.n + 8), nl)):
        assert_bit_equal(x, y, "a slot that no run names keeps its rows")
    assert_bit_equal(m.forward(6, 1), own.feed([6]), "forward between passes")
    toks = np.array([7, 8, 9, 10, 11], np.uint32)
    am, _ = m.verify_tokens(toks, own.n)
    assert am.tolist() == [ref_argmax(own.feed([t])) for t in toks], "verify_tokens between passes"
    # lmrs_batch_forward and lmrs_batch_generate_greedy on the same slots, then runs again
    pos = [s.n for s in seqs[:2]]
    am = b.forward([0, 1], [3, 4], pos)
    assert am.tolist() == [ref_argmax(s.feed([t])) for s, t in zip(seqs[:2], (3, 4))]
    out = b.generate_greedy([2], [9], [seqs[2].n], 4)
    t, want = 9, []
    for _ in range(4):
        t = ref_argmax(seqs[2].feed([t])); want.append(t)
    assert out[0].tolist() == want
    run_pass(b, [(s, toks_for(cfg, n, 20 + s.slot), n) for s, n in zip(seqs, (2, 3, 1, 4))], "pass 1")
    for layer in range(nl):
        for p in range(own.n):
            for w in (0, 1):
                assert_bit_equal(m.kv_row(w, layer, p), own.orc.kv_row(w, layer, p), f"the context's own {'kv'[w]} row layer {layer} pos {p}")
    assert_bit_equal(m.forward(3, own.n), own.feed([3]), "forward after everything")


# ---------------------------------------------------------------------------------------------- 9. refusals

@gpu
def test_refusals_come_before_device_work(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=185)
    m, b, seqs = prefilled(L, img, cfg, [6, 0, 0], 186)
    V, T = m.args.vocab_size, m.args.seq_len
    n_good = [0]

    def good():
        run_pass(b, [(seqs[0], [50 + n_good[0] % 7], 1), (seqs[1], [60, 61], n_good[0] % 3)], f"the valid call after refusal {n_good[0]}")
        n_good[0] += 1

    cases = [
        ([], {}, "n_runs = 0 is outside 1 .. 16"),
        ([(0, 0, [1], 1)] * 17, {}, "n_runs = 17 is outside 1 .. 16"),
        ([(0, 6, [1], 1), (1, 0, [], 0)], {}, "run 1: run_len is 0"),
        ([(0, 0, [1] * 200, 0), (1, 0, [1] * 200, 0), (2, 0, [1] * 113, 0)], {}, "more than 512 rows"),
        ([(0, 6, [1], 1), (0, 7, [2], 1)], {}, "slot 0 appears in more than one run"),
        ([(0, 6, [1], 1), (3, 0, [2], 1)], {}, "run 1: slot 3 of 3"),
        ([(0, 6, [1, 2], 3)], {}, "run 0: n_out = 3 exceeds run_len = 2"),
        ([(0, 6, [1, V], 1)], {}, "token 1 out of range"),
        ([(0, 6, [1], 1), (1, T - 2, [1, 2, 3], 1)], {}, "run 1: start_pos \\+ run_len exceeds seq_len"),
        ([(0, 6, [1], 1)], {"k": 257}, "k = 257 is outside 1 .. 256"),
    ]
    for runs, kw, msg in cases:
        with pytest.raises(L.LmrsError, match=msg):
            b.forward_runs(runs, **kw)
        good()
    # (k > vocab_size needs a vocabulary below 256: the rule is topk_check_k's, tested in tests/test_topk.py; here through this call on a small model)
    lib = L.lib()
    one = np.array([1], np.uint32); zero = np.array([0], np.uint32); six = np.array([seqs[0].n], np.uint32); out = np.zeros(8, np.uint32)
    p1, p0, p6, po = one.ctypes.data, zero.ctypes.data, six.ctypes.data, out.ctypes.data

    def call(bh=None, slot=p0, start=p6, ln=p1, no=p1, tok=p1, am=po, k=0, ti=None, tl=None):
        return lib.lmrs_batch_forward_runs(b._h if bh is None else bh, 1, slot, start, ln, no, tok, am, None, k, ti, tl)

    for kw, msg in (({"k": 2}, "k > 0 needs topk_idx and topk_logprob"), ({"k": 2, "ti": po}, "k > 0 needs topk_idx and topk_logprob"),
                    ({"am": None}, "argmax is NULL with 1 output rows"), ({"slot": None}, "NULL argument"), ({"start": None}, "NULL argument"),
                    ({"ln": None}, "NULL argument"), ({"no": None}, "NULL argument"), ({"tok": None}, "NULL argument")):
        assert call(**kw) != 0 and msg in lib.lmrs_last_error().decode(), (kw, lib.lmrs_last_error().decode())
        good()
    assert lib.lmrs_batch_forward_runs(None, 1, p0, p6, p1, p1, p1, po, None, 0, None, None) != 0 and "NULL argument" in lib.lmrs_last_error().decode()
    good()
    # the existing calls keep their own messages
    with pytest.raises(L.LmrsError, match="appears twice"):
        b.forward([0, 0], [1, 2], [6, 7])
    good()


@gpu
def test_k_above_a_small_vocabulary_is_refused(L):
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-v208", vocab_size=208)
    img = S.build_image(cfg, S.Q8_0, seed=187)
    m = L.Transformer(img); b = L.Batch(m, 1); s = Seq(img, 0)
    with pytest.raises(L.LmrsError, match="k = 209 exceeds vocab_size = 208"):
        b.forward_runs([(0, 0, [1, 2], 1)], k=209)
    _, rows, (ti, tl) = run_pass(b, [(s, [1, 2, 3], 2)], "k = vocab_size", k=208)
    assert ti[1].tolist() == rank_row(rows[0][2]).tolist()


# ---------------------------------------------------------------------------------------------- resources, example, ABI presence (no GPU)

def test_new_kernels_have_no_scratch_and_stay_outside_the_hot_table():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    new = {n: r for n, r in rows.items() if re.search(NEW_KERNELS, n)}
    # RoPE + scatter, the row selection, attention over the long table for head sizes 64 / 96 / 128 and Gemma's 256
    assert len(new) == 6, sorted(new)
    assert sum("attention_runs_kernel" in n for n in new) == 4
    for n, r in new.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{n}: scratch {r['scratch']} bytes per lane, spilled VGPRs {r['vgpr_spill']}"
        assert not KR.HOT.match(n), f"{n} must not enter the hot table"
        if "attention_runs_kernel" in n:
            # the body is attention_table_kernel's: so are its registers, LDS and occupancy
            twin = rows[n.replace("attention_runs_kernel", "attention_table_kernel")]
            assert (r["sgpr_spill"], r["waves_per_simd"]) == (twin["sgpr_spill"], twin["waves_per_simd"]) and abs(r["vgpr"] - twin["vgpr"]) <= 16, f"{n}: {r} vs {twin}"
        else:
            assert r["sgpr_spill"] == 0, f"{n}: spilled SGPRs {r['sgpr_spill']}"


def test_batch_admit_example_passes_the_syntax_check():
    src = os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_admit.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "forward_runs" in open(src).read()


def test_entry_point_exists_in_every_layer(L):
    name = "lmrs_batch_forward_runs"
    assert hasattr(L.lib(), name) and name in L.EXPORTS and callable(L.Batch.forward_runs)
    header = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    assert re.search(rf"\bint\s+{name}\(", header) and "transformer.rs:316-384" in header[header.index("ONE weight pass over n_runs"):header.index(f"int {name}(")]
    assert name in open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()


@gpu
def test_batch_admit_program_prints_what_batch_greedy_prints(tmp_path):
    """hostcpp/batch_admit.cpp and hostcpp/batch_greedy.cpp, built and run over the same five prompts (a small tokenizer.bin in the layout of
    tokenizer.rs:24-64 for mini-llama's vocabulary): the continuations are equal, line by line, with the late prompt admitted two tokens a step."""
    import struct
    cfg = S.CONFIGS["mini-llama"]
    S.build_image(cfg, S.Q8_0, seed=189).tofile(tmp_path / "model.lmrs")
    toks = [("<unk>", 0.0), ("<s>", 0.0), ("</s>", 0.0)] + [("<0x%02X>" % b, 0.0) for b in range(256)]
    toks += [(ch, -1.0 - i) for i, ch in enumerate(" abcdefghijklmnopqrstuvwxyz")]
    toks += [(m, 5.0 - 0.1 * i) for i, m in enumerate(["he", "ll", "hell", "hello", " w", "or", "ld", " world", "wor"])]
    toks += [("<fill_%d>" % i, 0.0) for i in range(cfg.vocab_size - len(toks))]
    blob = struct.pack("IIII", len(toks), 16, 1, 2)
    for s_, sc in toks:
        b = s_.encode(); blob += struct.pack("fI", sc, len(b)) + b
    (tmp_path / "tokenizer.bin").write_bytes(blob)
    (tmp_path / "prompts.txt").write_text("hello world\nworld\na quick brown fox\nhello hello hello world\nthe late prompt is the longest of them all\n")
    out = {}
    for prog, extra in (("batch_greedy", []), ("batch_admit", ["--chunk", "2"])):
        exe = str(tmp_path / prog)
        subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "lm.rs_amd", "hostcpp", prog + ".cpp"), "-I", os.path.join(ROOT, "include"),
                        "-L", os.path.join(ROOT, "lm.rs_amd"), "-llmrs_hip", f"-Wl,-rpath,{os.path.join(ROOT, 'lm.rs_amd')}", "-o", exe], check=True)
        r = subprocess.run([exe, "--model", str(tmp_path / "model.lmrs"), "--tokenizer", str(tmp_path / "tokenizer.bin"), "--prompts", str(tmp_path / "prompts.txt"),
                            "--n", "12"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[prog] = [l for l in r.stdout.split("\n") if l.startswith("[")]
    assert len(out["batch_greedy"]) == 5 and out["batch_admit"] == out["batch_greedy"], out
