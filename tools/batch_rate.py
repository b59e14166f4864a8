"""What a multi-sequence decode step yields on a full-size synthetic model, in one process: aggregate tokens per second of lmrs_batch_generate_greedy
over 64 steps at n = 1, 2, 4, 8, 16 rows standing at about 100 positions, against lmrs_generate_greedy over the same 64 steps on the context's own cache
(the single-sequence decode step: the baseline), then n = 16 and the baseline again with the rows at about 1030 positions.  Both calls report device
time (HIP events around their steps): median of 5 after 2 warm-ups, with the minimum and the maximum.  Every row's token ids are compared with the
single-sequence run of the same prompt in the same process.  Last, one lmrs_batch_fork of 1030 positions at full size, timed and checked.
usage: python tools/batch_rate.py [model] [q8_0|q4_0]
       (writes profiles/batch_decode_llama1b.txt for llama-3.2-1b q8_0, profiles/batch_decode_gemma2b_q4.txt for gemma-2-2b q4_0)
       python tools/batch_rate.py --wide [model] [q8_0|q4_0]
--wide: the same protocol on a WIDE batch (lmrs_batch_create_wide) - n = 16, 17, 24, 32, 47, 48, 64 rows at about 100 positions and n = 64 at about 1030 -
and, before it, the time of ONE ragged pass (lmrs_batch_forward_runs, 16 runs on 16 slots at 100 positions, every row's output asked for) of 16 .. 64 rows:
host time of 64 synchronous calls / 64, median of 5 after 2 warm-ups.  That call exists without the wide batch too, so on a build that lacks
lmrs_batch_create_wide the mode prints the pass times and the n = 16 line only: the two trees of an A/B run by turns.  BATCH_RATE_OUT names the file written.
       python tools/batch_rate.py --paged [model] [q8_0|q4_0]
--paged: a PAGED batch (lmrs_batch_create_paged) against the wide batch of the same build, the forms by turns (paged_main below)
       (writes profiles/batch_paged_llama1b.txt, profiles/batch_paged_gemma2b_q4.txt, profiles/batch_paged_phi35.txt)
       python tools/batch_rate.py --kvq [--parent-lib PATH] [model] [q8_0|q4_0]
--kvq: a Q8 paged batch (lmrs_batch_create_paged_q8) against the f32 paged batch of the same build, by turns (kvq_main below)
       (writes profiles/batch_kvq_llama1b.txt, profiles/batch_kvq_gemma2b_q4.txt)
       python tools/batch_rate.py --kvq --kv q4 [--parent-lib PATH] [model] [q8_0|q4_0]
--kv q4: the same protocol with a Q4 paged batch (lmrs_batch_create_paged_q4) as a third pool beside the f32 and the Q8 one; a Q4 line is a MISS where it is
       slower than the Q8 pool's by more than the larger of the two pools' turn spreads
       (writes profiles/batch_kv4_llama1b.txt, profiles/batch_kv4_gemma2b_q4.txt)
       python tools/batch_rate.py --paged-prefill [model] [q8_0|q4_0]
--paged-prefill: lmrs_batch_prefill of 16 .. 512 tokens on a wide batch, on paged batches (block attention over the page table from 16 rows on) and on the
same paged batches with lmrs_batch_debug_prefill_table (every chunk through the table pass: the routing before), and on a Q8 paged batch under the library's
rule and forced to the table pass, the forms by turns (paged_prefill_main below)
       (writes profiles/batch_kvq_prefill_llama1b.txt, profiles/batch_kvq_prefill_gemma2b_q4.txt; the five f32 forms alone were recorded in
       profiles/batch_paged_prefill_*.txt)
       python tools/batch_rate.py --paged-prefill --kv q4 [model] [q8_0|q4_0]
--paged-prefill --kv q4: 320 .. 512 tokens on a Q4 paged batch under the library's rule (block attention over Q4 pages) and forced to the table pass, by turns
beside the f32 and the Q8 paged batch's block attention
       (writes profiles/batch_kv4_prefill_llama1b.txt, profiles/batch_kv4_prefill_gemma2b_q4.txt)
       python tools/batch_rate.py --tree [--parent-lib PATH] [model] [q8_0|q4_0]
--tree: a pass over token trees (lmrs_batch_forward_tree) against lmrs_batch_forward_runs of equal rows, this build's by turns and the parent commit's in
processes of their own, the existing calls against the parent, lmrs_batch_accept_path and the launch lists (tree_main below)
       (writes profiles/batch_tree_llama1b.txt, profiles/batch_tree_gemma2b_q4.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import bench  # noqa: E402
import lmrs_amd  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402

STEPS, ROWS = 64, 16
OUT = {("llama-3.2-1b", S.Q8_0): "batch_decode_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_decode_gemma2b_q4.txt"}


def timed(fn, reps=5, warm=2):
    """fn() -> (ids, device seconds); -> (ids of the last run, median, min, max in microseconds)"""
    for _ in range(warm):
        fn()
    runs = [fn() for _ in range(reps)]
    us = [sec * 1e6 for _, sec in runs]
    return runs[-1][0], statistics.median(us), min(us), max(us)


WIDE_ROWS = (16, 17, 24, 32, 47, 48, 64)


def wide_main(argv):
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    has_wide = hasattr(lmrs_amd.lib(), "lmrs_batch_create_wide")
    rows_max = 64 if has_wide else ROWS
    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    b = lmrs_amd.Batch(m, 64, wide=True) if has_wide else lmrs_amd.Batch(m, ROWS)
    say(f"python tools/batch_rate.py --wide {model} {qname}" + ("" if has_wide else "   (a build without lmrs_batch_create_wide: the shared lines only)"))
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}; LMRS_LIB={os.path.basename(os.environ.get('LMRS_LIB', ''))}")
    for depth in (100, 1030):
        prompts = [S.prompt_tokens(model, depth + 8, 100 + i) for i in range(rows_max)]    # row i: depth tokens in its cache, the next ones fed first
        for i, p in enumerate(prompts):
            b.prefill(i, p[:depth], 0)
        if depth == 100:
            say(f"one ragged pass (lmrs_batch_forward_runs): R rows as 16 runs on 16 slots at {depth} positions, every row's output asked for; host time of {STEPS} "
                f"synchronous calls / {STEPS}, median of 5 after 2 warm-ups (min .. max)")
            for R in WIDE_ROWS:
                lens = [R // 16 + (1 if i < R % 16 else 0) for i in range(16)]
                runs = [(i, depth, [int(t) for t in prompts[i][depth:depth + n]], n) for i, n in enumerate(lens)]

                def calls():
                    t0 = time.perf_counter()
                    for _ in range(STEPS):
                        am = b.forward_runs(runs)
                    return am, time.perf_counter() - t0
                am, us, lo, hi = timed(calls)
                say(f"  R={R:2d}   {us / STEPS:8.1f} us per pass ({lo / STEPS:.1f} .. {hi / STEPS:.1f})   argmax checksum {int(am.astype(np.uint64).sum())}")
        singles = []
        for p in prompts:                                    # the single-sequence ids of every row's prompt, and the baseline's time from row 0's
            m.prefill_tokens(p[:depth], 0)
            singles.append(m.generate_greedy(p[depth:depth + 1], STEPS, depth))
        m.prefill_tokens(prompts[0][:depth], 0)
        _, base, lo, hi = timed(lambda: m.generate_greedy(prompts[0][depth:depth + 1], STEPS, depth, timing=True))
        base_rate = STEPS / base * 1e6
        say(f"rows at {depth} positions: {STEPS} greedy steps per call, device time of the steps (HIP events inside the call); median of 5 after 2 warm-ups (min .. max)")
        say(f"  lmrs_generate_greedy (one sequence)   {base / STEPS:8.1f} us per step ({lo / STEPS:.1f} .. {hi / STEPS:.1f})   {base_rate:9.1f} tok/s")
        for n in (WIDE_ROWS if depth == 100 else (64,)):
            if n > rows_max:
                continue
            slots = list(range(n))
            ids, us, lo, hi = timed(lambda: b.generate_greedy(slots, [int(p[depth]) for p in prompts[:n]], [depth] * n, STEPS, timing=True))
            same = all(ids[i].tolist() == singles[i].tolist() for i in range(n))
            rate = n * STEPS / us * 1e6
            say(f"  lmrs_batch_generate_greedy n={n:2d}       {us / STEPS:8.1f} us per pass ({lo / STEPS:.1f} .. {hi / STEPS:.1f})   {rate:9.1f} tok/s aggregate"
                f"   {rate / base_rate:5.2f}x the baseline   same tokens as the single-sequence runs: {same}")
    path = os.environ.get("BATCH_RATE_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


PAGED_OUT = {("llama-3.2-1b", S.Q8_0): "batch_paged_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_paged_gemma2b_q4.txt", ("phi-3.5", S.Q8_0): "batch_paged_phi35.txt"}


def paged_main(argv):
    """--paged [model] [q8_0|q4_0]: a paged batch (lmrs_batch_create_paged, page_len 64 and 256) against the wide batch of the same build, in one process,
    the forms by turns three times: us per pass of 16 and 64 decode rows at 100 and at 1000 positions (device time of 64 greedy steps a call, median of 3 a
    turn), a fork of 1000 positions into 63 slots (wall time, bytes held), and a 512-token lmrs_batch_prefill (wall time).  --paged phi-3.5 q8_0: the
    full-size case only - the wide batch of 64 slots against a pool for 64 x 1024 positions."""
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    def finish():
        name = PAGED_OUT.get((model, qt))
        path = os.environ.get("BATCH_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
        if path:
            with open(path, "w") as f:
                f.write("\n".join(lines) + "\n")

    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    a = m.args
    say(f"python tools/batch_rate.py --paged {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}")
    pos_bytes = 2 * a.n_layers * a.n_kv_heads * a.head_size * 4                              # K and V of one position, all layers
    if model == "phi-3.5":
        try:
            lmrs_amd.Batch(m, 64, wide=True)
            say("lmrs_batch_create_wide(64): created")
        except lmrs_amd.LmrsError as e:
            say(f"lmrs_batch_create_wide(64): {e}")
        b = lmrs_amd.Batch(m, 64, page_len=256, n_pages=64 * 4)
        say(f"lmrs_batch_create_paged(64, page_len 256, 256 pages = 64 x 1024 positions): created, {257 * 256 * pos_bytes / 1e9:.2f} GB")
        p = S.prompt_tokens(model, 101, 100)
        for i in range(64):
            b.prefill(i, p[:100], 0)
        ids, us, lo, hi = timed(lambda: b.generate_greedy(list(range(64)), [int(p[100])] * 64, [100] * 64, STEPS, timing=True), reps=3, warm=1)
        say(f"  lmrs_batch_generate_greedy n=64 at 100 positions, {STEPS} steps a call: {us / STEPS:8.1f} us per pass ({lo / STEPS:.1f} .. {hi / STEPS:.1f})   "
            f"{64 * STEPS / us * 1e6:9.1f} tok/s aggregate; the 64 rows agree: {all(ids[i].tolist() == ids[0].tolist() for i in range(64))}; pages (page_len, n, free): {b.pages()}")
        return finish()
    forms = [("wide", None), ("paged 64", 64), ("paged 256", 256)]
    say(f"us per pass of lmrs_batch_generate_greedy ({STEPS} greedy steps a call, device time of the steps): the three forms by turns, three turns, median of 3 "
        f"calls after 1 warm-up a turn; per form the median of its turns (fastest .. slowest turn)")
    prompt = S.prompt_tokens(model, 1001, 100)
    for depth in (100, 1000):
        batches = {}
        for name, pl in forms:
            b = lmrs_amd.Batch(m, 64, wide=True) if pl is None else lmrs_amd.Batch(m, 64, page_len=pl, n_pages=64 * (-(-(depth + STEPS + 1) // pl)))
            for i in range(64):
                b.prefill(i, prompt[:depth], 0)
            batches[name] = b
        for n in (16, 64):
            turns, ids = {name: [] for name, _ in forms}, {}
            for _ in range(3):
                for name, _pl in forms:
                    b = batches[name]
                    ids[name], us, _lo, _hi = timed(lambda: b.generate_greedy(list(range(n)), [int(prompt[depth])] * n, [depth] * n, STEPS, timing=True), reps=3, warm=1)
                    turns[name].append(us / STEPS)
            same = all((ids[name] == ids["wide"]).all() for name, _ in forms)
            w = statistics.median(turns["wide"])
            for name, _pl in forms:
                t = turns[name]
                say(f"  {depth:4d} positions, n={n:2d}, {name:9s}  {statistics.median(t):8.1f} us per pass ({min(t):.1f} .. {max(t):.1f})   {statistics.median(t) / w - 1:+6.1%} against wide")
            say(f"      the three forms give the same tokens: {same}")
        if depth == 1000:
            say("lmrs_batch_fork of 1000 positions from slot 0 into slots 1 .. 63 (host wall time of the 63 synchronous calls), and the K/V bytes the 64 slots then hold")
            for name, pl in forms:
                b = batches[name]
                for s in range(1, 64):
                    if pl is not None:
                        b.release(s)
                t0 = time.perf_counter()
                for s in range(1, 64):
                    b.fork(0, s, 1000)
                ms = (time.perf_counter() - t0) * 1e3
                held = 64 * 1000 * pos_bytes if pl is None else (b.pages()[1] - b.pages()[2]) * pl * pos_bytes
                say(f"  {name:9s}  {ms:8.2f} ms   {held / 1e6:9.1f} MB of written or held K/V" + ("" if pl is None else f" ({b.pages()[1] - b.pages()[2]} pages)"))
            say("lmrs_batch_prefill of 512 tokens into slot 1 (host wall time of the synchronous call, median of 5 after 1 warm-up): block attention on every form, "
                "over the page table on a paged batch (--paged-prefill: every length by turns, and the table pass it replaced)")
            for name, pl in forms:
                b = batches[name]

                def call():
                    t0 = time.perf_counter(); b.prefill(1, prompt[:512], 0)
                    return None, time.perf_counter() - t0
                _, us, lo, hi = timed(call, reps=5, warm=1)
                say(f"  {name:9s}  {us / 1e3:8.2f} ms ({lo / 1e3:.2f} .. {hi / 1e3:.2f})")
        for b in batches.values():
            b.close()
    finish()


PREFILL_OUT = {("llama-3.2-1b", S.Q8_0): "batch_kvq_prefill_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_kvq_prefill_gemma2b_q4.txt"}
PREFILL_CASES = [(16, 0), (32, 0), (64, 0), (80, 0), (96, 0), (112, 0), (128, 0), (256, 0), (512, 0), (512, 512)]   # (tokens, start position); 80 .. 112: around the crossover

# --kv q4: from kKv4BlockMin rows on, a 64-query block at a time
KV4_PREFILL_OUT = {("llama-3.2-1b", S.Q8_0): "batch_kv4_prefill_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_kv4_prefill_gemma2b_q4.txt"}
KV4_PREFILL_CASES = [(320, 0), (384, 0), (448, 0), (512, 0)]


def paged_prefill_main(argv):
    """--paged-prefill [model] [q8_0|q4_0]: host wall time of the synchronous lmrs_batch_prefill call into slot 0, in one process, seven forms by turns,
    three turns, median of 5 calls after 1 warm-up a turn: (a) the wide batch; (b) paged batches of page_len 64 and 256 under the library's routing; (c) the
    same two with lmrs_batch_debug_prefill_table(1) - every chunk through the table pass, one workgroup per (head, row); (d) a Q8 paged batch of page_len 64
    under the library's rule (block attention over int8 pages from 256 rows on) and (e) the same forced to the table pass.  Per form and length the median
    of its turns (fastest .. slowest turn), lmrs_batch_prefill_form's answer, and whether the forms of one K/V format leave the same last K row.
    --kv q4 in front of the model: four forms at 320 .. 512 rows - f32, Q8 and Q4 pages of page_len 64 under the library's rule (block attention on all three)
    and the Q4 pages forced to the table pass; a length at which Q4 block attention is not faster than its table pass outside the turns' spread is a MISS."""
    q4 = argv[:2] == ["--kv", "q4"]
    if q4:
        argv = argv[2:]
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    say(f"python tools/batch_rate.py --paged-prefill {'--kv q4 ' if q4 else ''}{model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}")
    forms = [("wide", None, False), ("paged 64", 64, False), ("paged 256", 256, False), ("paged 64 table", 64, True), ("paged 256 table", 256, True),
             ("q8 64", 64, False), ("q8 64 table", 64, True)]
    if q4:
        forms = [("paged 64", 64, False), ("q8 64", 64, False), ("q4 64", 64, False), ("q4 64 table", 64, True)]
    say(f"lmrs_batch_prefill into slot 0, host wall time of the synchronous call: {len(forms)} forms by turns, three turns, median of 5 calls after 1 warm-up a turn; "
        "per form the median of its turns (fastest .. slowest turn); form = lmrs_batch_prefill_form's (chunks, of them block attention)")
    prompt = S.prompt_tokens(model, 1024, 100)
    batches = {}
    for name, pl, table in forms:
        kv = name.split()[0] if name[0] == "q" else "f32"
        b = lmrs_amd.Batch(m, 2, wide=True) if pl is None else lmrs_amd.Batch(m, 2, page_len=pl, n_pages=2 * (1024 // pl), kv=kv)
        if table:
            b.debug_prefill_table(True)
        batches[name] = b
    nl = m.args.n_layers
    first = forms[0][0]                                     # the form the others' times are quoted against
    for n, start in (KV4_PREFILL_CASES if q4 else PREFILL_CASES):
        toks = prompt[start:start + n]
        turns, last = {name: [] for name, _, _ in forms}, {}
        for b in batches.values():
            if start:
                b.prefill(0, prompt[:start], 0)
        for _ in range(3):
            for name, _pl, _t in forms:
                b = batches[name]

                def call():
                    t0 = time.perf_counter(); b.prefill(0, toks, start)
                    return None, time.perf_counter() - t0
                _, us, _lo, _hi = timed(call, reps=5, warm=1)
                turns[name].append(us / 1e3)
        for name, _pl, _t in forms:
            last[name] = batches[name].kv_row(0, 0, nl - 1, start + n - 1).view(np.uint32).copy()
        w = statistics.median(turns[first])
        for name, pl, table in forms:
            t = turns[name]
            note = f"{statistics.median(t) / w:5.2f}x {first}"
            if pl is not None and not table and name + " table" in turns:
                old = turns[name + " table"]
                note += f"   {statistics.median(t) / statistics.median(old):5.2f}x its table pass; slowest turn below the table pass's fastest: {max(t) < min(old)}"
                if name[0] == "q":
                    note += f"; {statistics.median(t) / statistics.median(turns['paged 64']):5.2f}x the f32 pages"
                if name.startswith("q4"):
                    note += f", {statistics.median(t) / statistics.median(turns['q8 64']):5.2f}x the Q8 pages"
                if name[0] == "q" and batches[name].prefill_form(n, start)[1]:
                    # the condition of DESIGN.md 4.4.17 / 4.4.19: faster than the table pass by more than the larger turn-to-turn spread of the two forms
                    gap, spread = statistics.median(old) - statistics.median(t), max(max(t) - min(t), max(old) - min(old))
                    note += f"; gap {gap:.3f} ms against spread {spread:.3f} ms: {'wins' if gap > spread else '** MISS **' if q4 else 'NO WIN'}"
            say(f"  {n:3d} tokens at {start:3d}, {name:15s} form {batches[name].prefill_form(n, start)}  {statistics.median(t):8.3f} ms ({min(t):.3f} .. {max(t):.3f})   {note}")
        # per K/V format the forms' last K row against the format's first form
        head = {}
        same = all((last[name] == last[head.setdefault(name.split()[0] if name[0] == "q" else "f32", name)]).all() for name, _, _ in forms)
        say(f"      the forms of one K/V format leave the same last K row: {same}")
    for b in batches.values():
        b.close()
    name = (KV4_PREFILL_OUT if q4 else PREFILL_OUT).get((model, qt))
    path = os.environ.get("BATCH_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def kvq_child(image_path, kv, traced):
    """--kvq's child, over a binding of its own (the parent commit's library has no Q8 entry points) on the library LMRS_LIB names: 64 slots of a paged pool
    (kv: f32 | q8, page_len 64).  Timed: each slot prefilled, then us per pass of 64 rows at 100 positions, 64 and 16 rows at 1000 (device time of 64 greedy
    steps a call, median of 3 after 1 warm-up) and a 512-token prefill (wall time, median of 5 after 1).  traced (under rocprofv3): slot 0 prefilled to 1000 and
    forked into the others, then one call of 2 steps and one of 8 - the last 8 x n_layers launches of a kernel are its decode launches at 1000 positions."""
    import ctypes as C
    lib = C.CDLL(os.environ.get("LMRS_LIB", lmrs_amd.LIB_PATH))
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.lmrs_last_error.restype = C.c_char_p
    lib.lmrs_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    create = {"f32": "lmrs_batch_create_paged", "q8": "lmrs_batch_create_paged_q8", "q4": "lmrs_batch_create_paged_q4"}[kv]
    create = getattr(lib, create)
    create.argtypes = [vp, u32, u32, u32, C.POINTER(vp)]
    lib.lmrs_batch_prefill.argtypes = [vp, u32, vp, sz, u32]
    lib.lmrs_batch_fork.argtypes = [vp, u32, u32, u32]
    lib.lmrs_batch_generate_greedy.argtypes = [vp, u32, vp, vp, vp, u32, vp, C.POINTER(C.c_double)]
    lib.lmrs_batch_destroy.argtypes = [vp]; lib.lmrs_batch_destroy.restype = None
    lib.lmrs_destroy.argtypes = [vp]; lib.lmrs_destroy.restype = None

    def chk(rc):
        if rc:
            raise RuntimeError(lib.lmrs_last_error().decode())

    img = np.fromfile(image_path, np.uint8)
    prompt = np.ascontiguousarray(np.fromfile(image_path + ".prompt", np.uint32))
    h, used = vp(), sz()
    chk(lib.lmrs_create(img.ctypes.data, img.size, 0, C.byref(h), C.byref(used)))

    def greedy(b, n, depth, steps):
        slot = np.arange(n, dtype=np.uint32); pos = np.full(n, depth, np.uint32); tok = np.full(n, prompt[depth], np.uint32)
        ids = np.zeros((n, steps), np.uint32); sec = C.c_double()
        chk(lib.lmrs_batch_generate_greedy(b, n, slot.ctypes.data, tok.ctypes.data, pos.ctypes.data, steps, ids.ctypes.data, C.byref(sec)))
        return sec.value * 1e6 / steps, int(ids.astype(np.uint64).sum())

    out = []
    for depth, ns in ((1000, (64,)),) if traced else ((100, (64,)), (1000, (64, 16))):
        b = vp()
        chk(create(h, 64, 64, 64 * (-(-(depth + STEPS + 1) // 64)) + 64, C.byref(b)))
        for i in range(64):
            if traced and i:
                chk(lib.lmrs_batch_fork(b, 0, i, depth))
            else:
                chk(lib.lmrs_batch_prefill(b, i, prompt.ctypes.data, depth, 0))
        if traced:
            greedy(b, 64, depth, 2); greedy(b, 64, depth, 8)
        for n in () if traced else ns:
            runs = [greedy(b, n, depth, STEPS) for _ in range(4)][1:]
            out += [statistics.median(u for u, _ in runs), runs[-1][1]]
        if depth == 1000 and not traced:
            ms = []
            for _ in range(6):
                t0 = time.perf_counter(); chk(lib.lmrs_batch_prefill(b, 1, prompt.ctypes.data, 512, 0)); ms.append((time.perf_counter() - t0) * 1e3)
            out.append(statistics.median(ms[1:]))
        lib.lmrs_batch_destroy(b)
    lib.lmrs_destroy(h)
    print("KVQ " + " ".join(f"{x:.2f}" if isinstance(x, float) else str(x) for x in out), flush=True)


def kvq_processes(say, img, model, prompt, parent, q4=False):
    """--kvq's two sections that need processes of their own: the parent commit's library, and the launches alone under a kernel trace"""
    import csv, glob, shutil, subprocess, tempfile  # noqa: E401
    me, L = os.path.abspath(__file__), S.CONFIGS[model].n_layers
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "model.lmrs")
        img.tofile(path); np.ascontiguousarray(prompt, np.uint32).tofile(path + ".prompt")
        say("the f32 pool on the PARENT commit's library against this build's two pools, a process per library, pool and turn, two turns (us per pass as above, "
            "median of 3 calls after 1 warm-up; the 512-token prefill in ms)")
        if not parent or not os.path.exists(parent):
            say("  not run: no parent library given (--parent-lib PATH)")
        else:
            runs = (("parent f32", os.path.abspath(parent), "f32"), ("this f32", lmrs_amd.LIB_PATH, "f32"), ("this q8", lmrs_amd.LIB_PATH, "q8"))
            runs += (("this q4", lmrs_amd.LIB_PATH, "q4"),) if q4 else ()
            res = {k: [] for k, _, _ in runs}
            for turn in range(2):
                for who, lib, kv in runs:
                    r = subprocess.run([sys.executable, me, "--kvq-child", path, kv], env=dict(os.environ, LMRS_LIB=lib), capture_output=True, text=True, timeout=900)
                    got = [l for l in r.stdout.splitlines() if l.startswith("KVQ ")]
                    if r.returncode or not got:
                        say(f"  {who}, turn {turn}: failed: {r.stderr.strip()[-300:]}")
                        continue
                    v = got[0].split()[1:]
                    res[who].append(v)
                    say(f"  turn {turn}  {who:10s}  64 x 100: {v[0]:>8s}   64 x 1000: {v[2]:>8s}   16 x 1000: {v[4]:>8s} us per pass   prefill 512: {v[6]:>6s} ms   token checksums {v[1]} {v[3]} {v[5]}")
            if all(res.values()):
                mean = lambda who, k: statistics.mean(float(v[k]) for v in res[who])
                for k, what in ((0, "64 x 100"), (2, "64 x 1000"), (4, "16 x 1000"), (6, "prefill 512")):
                    p = mean("parent f32", k)
                    spread = max(float(v[k]) for v in res["parent f32"]) - min(float(v[k]) for v in res["parent f32"])
                    say(f"  {what:11s}  parent f32 {p:8.2f} (its turns {spread:.2f} apart)   this f32 {mean('this f32', k):8.2f} ({mean('this f32', k) / p - 1:+.2%})   "
                        f"this q8 {mean('this q8', k):8.2f} ({mean('this q8', k) / p - 1:+.2%}{'  ** A MISS **' if mean('this q8', k) > p + spread else ''})")
                    if q4:                                # against this build's Q8 pool: slower by more than the larger of the two pools' turn spreads is a MISS
                        gap = lambda who: max(float(v[k]) for v in res[who]) - min(float(v[k]) for v in res[who])
                        a8, a4, allow = mean("this q8", k), mean("this q4", k), max(gap("this q8"), gap("this q4"))
                        say(f"  {'':11s}  this q4 {a4:8.2f} ({a4 / p - 1:+.2%} against parent f32, {a4 / a8 - 1:+.2%} against this q8; turns q8 {gap('this q8'):.2f} / q4 {gap('this q4'):.2f} apart)"
                            f"{f'  ** MISS: q4 {a4:.2f} against q8 {a8:.2f} **' if a4 > a8 + allow else ''}")
                say(f"  f32 tokens equal between the libraries: {[res['parent f32'][0][k] for k in (1, 3, 5)] == [res['this f32'][0][k] for k in (1, 3, 5)]}")
        say(f"the launches alone, 64 rows at 1000 - 1007 positions: rocprofv3 --kernel-trace over a process per pool (slot 0 prefilled and forked into 63 slots, a call "
            f"of 2 steps, then one of 8); per kernel the last 8 x {L} launches: median (fastest .. slowest) us")
        if not shutil.which("rocprofv3"):
            say("  not run: rocprofv3 is not on the PATH")
            return
        traced = (("f32", ("paged_scatter_kernel", "paged_attn_kernel")), ("q8", ("kvq_scatter_kernel", "kvq_attn_kernel")))
        for kv, kernels in traced[1:] + (("q4", ("kv4_scatter_kernel", "kv4_attn_kernel")),) if q4 else traced:
            with tempfile.TemporaryDirectory() as tt:
                r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tt, "--", sys.executable, me, "--kvq-child", path, kv, "traced"],
                                   capture_output=True, text=True, timeout=900)
                traces = glob.glob(os.path.join(tt, "**", "*kernel_trace.csv"), recursive=True)
                if r.returncode or not traces:
                    say(f"  {kv}: failed: {r.stderr.strip()[-300:]}")
                    continue
                rows = sorted(csv.DictReader(open(traces[0])), key=lambda x: int(x["Start_Timestamp"]))
                for kern in kernels:
                    us = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in rows if kern in x["Kernel_Name"]][-8 * L:]
                    say(f"  {kern:22s} {len(us):4d} launches  {statistics.median(us):8.2f} ({min(us):.2f} .. {max(us):.2f}) us" if us else f"  {kern}: no launch in the trace")


KVQ_OUT = {("llama-3.2-1b", S.Q8_0): "batch_kvq_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_kvq_gemma2b_q4.txt"}
KV4_OUT = {("llama-3.2-1b", S.Q8_0): "batch_kv4_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_kv4_gemma2b_q4.txt"}
KVQ_MINIS = [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-llama3b", S.Q8_0), ("mini-gemma", S.Q4_0)]


def kvq_main(argv):
    """--kvq [--parent-lib PATH] [model] [q8_0|q4_0]: first, in processes of their own (kvq_processes), the f32 pool on the parent commit's library against this
    build's two pools, and the scatter and attention launches alone under a kernel trace.  Then a Q8 paged batch (lmrs_batch_create_paged_q8) against the f32 paged batch of the same build, page_len 64, in one process, the
    two pools by turns three times: us per pass of 64 decode rows at 100 and at 1000 positions and of 16 rows at 1000 (device time of 64 greedy steps a call,
    median of 3 a turn), a 512-token lmrs_batch_prefill (wall time; the Q8 pool takes the table pass), the pools' bytes for 64 x 1024 positions (also for
    the Phi-3.5 geometry, from its shapes), and - on the four mini models - the logits of the Q8 batch against the f32 paged batch after 130 positions."""
    parent, q4 = os.environ.get("BATCH_RATE_PARENT_LIB"), False
    if argv[:2] == ["--kv", "q4"]:
        q4, argv = True, argv[2:]
    if argv and argv[0] == "--parent-lib":
        parent, argv = argv[1], argv[2:]
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    say(f"python tools/batch_rate.py --kvq {'--kv q4 ' if q4 else ''}--parent-lib <the parent commit's liblmrs_hip.so> {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}")
    kvq_processes(say, img, model, S.prompt_tokens(model, 1001, 100), parent, q4)
    m = lmrs_amd.Transformer(img)
    say("in one process, both pools this build's:")
    forms = [("f32 pages", "f32"), ("q8 pages", "q8")] + ([("q4 pages", "q4")] if q4 else [])
    prompt = S.prompt_tokens(model, 1001, 100)
    say(f"us per pass of lmrs_batch_generate_greedy ({STEPS} greedy steps a call, device time of the steps): the two pools by turns, three turns, median of 3 calls "
        f"after 1 warm-up a turn; per pool the median of its turns (fastest .. slowest turn)")
    for depth, ns in ((100, (64,)), (1000, (64, 16))):
        batches = {}
        for name, kv in forms:
            b = lmrs_amd.Batch(m, 64, page_len=64, n_pages=64 * (-(-(depth + STEPS + 1) // 64)), kv=kv)
            for i in range(64):
                b.prefill(i, prompt[:depth], 0)
            batches[name] = b
        for n in ns:
            turns, ids = {name: [] for name, _ in forms}, {}
            for _ in range(3):
                for name, _kv in forms:
                    b = batches[name]
                    ids[name], us, _lo, _hi = timed(lambda: b.generate_greedy(list(range(n)), [int(prompt[depth])] * n, [depth] * n, STEPS, timing=True), reps=3, warm=1)
                    turns[name].append(us / STEPS)
            w = statistics.median(turns["f32 pages"])
            for name, _kv in forms:
                t = turns[name]
                say(f"  {depth:4d} positions, n={n:2d}, {name:9s}  {statistics.median(t):8.1f} us per pass ({min(t):.1f} .. {max(t):.1f})   {statistics.median(t) / w - 1:+6.1%} against f32 pages")
            say(f"      tokens equal between the pools (not expected: Q8 is another rule): {bool((ids['f32 pages'] == ids['q8 pages']).all())}")
        if depth == 1000:
            say("lmrs_batch_prefill of 512 tokens into slot 1 (host wall time of the synchronous call, median of 5 after 1 warm-up): block attention on f32, on Q8 and on Q4 pages (lmrs_batch_prefill_form's answer beside each)")
            for name, _kv in forms:
                b = batches[name]

                def call():
                    t0 = time.perf_counter(); b.prefill(1, prompt[:512], 0)
                    return None, time.perf_counter() - t0
                _, us, lo, hi = timed(call, reps=5, warm=1)
                say(f"  {name:9s}  {us / 1e3:8.2f} ms ({lo / 1e3:.2f} .. {hi / 1e3:.2f}); lmrs_batch_prefill_form(512): {b.prefill_form(512)}")
        for b in batches.values():
            b.close()
    say("pool bytes for 64 x 1024 positions (1024 pages of 64 and the zero page): kv_format's page_bytes x 1025")
    for name, kv in forms:
        b = lmrs_amd.Batch(m, 64, page_len=64, n_pages=1024, kv=kv)
        say(f"  {name:9s}  {b.kv_format()[2] * 1025 / 1e9:8.3f} GB  ({b.kv_format()[2]} bytes a page)")
        b.close()
    c = S.CONFIGS["phi-3.5"]
    per = 2 * c.n_layers * 64 * c.n_kv_heads * (c.dim // c.n_heads)
    say(f"  phi-3.5 geometry, from its shapes (not created here): f32 {per * 4 * 1025 / 1e9:.3f} GB, q8 {per * 9 // 8 * 1025 / 1e9:.3f} GB, q4 {per * 5 // 8 * 1025 / 1e9:.3f} GB")
    say(f"accuracy (reported, not a gate; synthetic weights): {'Q4' if q4 else 'Q8'} pages against f32 pages on the mini models, 6 slots prefilled to 130 positions, then one step: "
        "largest |logit difference| over the 6 rows, rows whose argmax agrees")
    for cfg, q in KVQ_MINIS:
        mm = lmrs_amd.Transformer(S.build_image(cfg, q, 1234))
        out = {}
        for name, kv in forms:
            b = lmrs_amd.Batch(mm, 6, page_len=64, n_pages=18, kv=kv)
            for i in range(6):
                b.prefill(i, S.prompt_tokens(cfg, 130, 700 + i), 0)
            out[name] = b.forward(list(range(6)), [7 + i for i in range(6)], [130] * 6, logits=True)
            b.close()
        (a0, l0), (a1, l1) = out["f32 pages"], out["q4 pages" if q4 else "q8 pages"]
        say(f"  {cfg:13s} {'Q4 ' if q4 else ''}max |dlogit| {float(np.abs(l0 - l1).max()):.5f} (largest |logit| {float(np.abs(l0).max()):.3f}); argmax agrees in {int((a0 == a1).sum())} of 6 rows")
    name = (KV4_OUT if q4 else KVQ_OUT).get((model, qt))
    path = os.environ.get("BATCH_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


TREE_OUT = {("llama-3.2-1b", S.Q8_0): "batch_tree_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_tree_gemma2b_q4.txt"}
# (slots, rows a slot): 16- and 64-node binary trees on 1 and 16 slots - a call takes 512 rows, so the 64-node trees stand on 8 slots - and one node a slot
TREE_SHAPES = ((1, 16), (16, 16), (1, 64), (8, 64), (1, 1), (16, 1))
TREE_PASSES = 8


def tree_child(image_path, mode):
    """--tree's child, over a binding of its own (the parent commit's library has no tree entry points) on the library LMRS_LIB names.  Per batch kind (wide,
    f32 paged with pages of 64), depth (100, 1000) and shape of TREE_SHAPES: us per pass of lmrs_batch_forward_runs with every row's output asked for and,
    where the library has it, of lmrs_batch_forward_tree over binary trees of as many rows at the same prefix - the two forms by turns, three turns, a turn
    the median of 3 calls of TREE_PASSES passes after 1 warm-up (host time of the synchronous calls).  Then lmrs_batch_forward at 16 and 64 rows, the decode
    step (lmrs_generate_greedy, bench.py's workload; device time) and lmrs_batch_accept_path of a 4-of-16 path on 16 slots.  One line a figure: TREE key
    median min max.  mode "traced" (under rocprofv3): one forward_runs call at 16 slots x 16 rows and 100 positions and one forward of 16 and of 64 rows, wide
    and paged - the calls both libraries have; "traced-tree": one tree pass there instead, and one accept."""
    import ctypes as C
    lib = C.CDLL(os.environ.get("LMRS_LIB", lmrs_amd.LIB_PATH))
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.lmrs_last_error.restype = C.c_char_p
    lib.lmrs_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.lmrs_batch_create_wide.argtypes = [vp, u32, C.POINTER(vp)]
    lib.lmrs_batch_create_paged.argtypes = [vp, u32, u32, u32, C.POINTER(vp)]
    lib.lmrs_batch_prefill.argtypes = [vp, u32, vp, sz, u32]
    lib.lmrs_batch_forward.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    lib.lmrs_batch_forward_runs.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
    lib.lmrs_generate_greedy.argtypes = [vp, vp, sz, u32, u32, vp, C.POINTER(C.c_double)]
    lib.lmrs_batch_destroy.argtypes = [vp]; lib.lmrs_batch_destroy.restype = None
    traced, tree_only = mode != "", mode == "traced-tree"
    has_tree = hasattr(lib, "lmrs_batch_forward_tree")
    if has_tree:
        lib.lmrs_batch_forward_tree.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
        lib.lmrs_batch_accept_path.argtypes = [vp, u32, vp, vp, vp, vp]

    def chk(rc):
        if rc:
            raise RuntimeError(lib.lmrs_last_error().decode())

    def p(a):
        return a.ctypes.data

    img = np.fromfile(image_path, np.uint8)
    prompt = np.ascontiguousarray(np.fromfile(image_path + ".prompt", np.uint32))
    h, used = vp(), sz()
    chk(lib.lmrs_create(p(img), img.size, 0, C.byref(h), C.byref(used)))
    u = lambda x: np.ascontiguousarray(x, np.uint32)

    def turns(forms, passes=TREE_PASSES, n_turns=3):
        """forms: {name: call}; by turns -> {name: (median, min, max) of the turns' medians, us per pass}"""
        got = {k: [] for k in forms}
        for _ in range(1 if traced else n_turns):
            for k, call in forms.items():
                us = []
                for _ in range(1 if traced else 4):
                    t0 = time.perf_counter()
                    for _ in range(1 if traced else passes):
                        call()
                    us.append((time.perf_counter() - t0) * 1e6 / (1 if traced else passes))
                got[k].append(statistics.median(us[0 if traced else 1:]))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}

    def say(key, r):
        print(f"TREE {key} {r[0]:.1f} {r[1]:.1f} {r[2]:.1f}", flush=True)

    for kind in ("wide", "paged"):
        for depth in (100,) if traced else (100, 1000):
            b = vp()
            if kind == "wide":
                chk(lib.lmrs_batch_create_wide(h, 64, C.byref(b)))
            else:
                chk(lib.lmrs_batch_create_paged(h, 64, 64, 64 * (-(-(depth + 65) // 64)), C.byref(b)))
            for i in range(64 if kind == "wide" and depth == 100 else 16):
                chk(lib.lmrs_batch_prefill(b, i, p(prompt), depth, 0))
            for slots, rows in ((16, 16),) if traced else TREE_SHAPES:
                sl, st, n = u(range(slots)), u([depth] * slots), u([rows] * slots)
                tok = u(np.tile(prompt[depth:depth + rows], slots))
                par = u(np.tile([0xFFFFFFFF] + [(j - 1) // 2 for j in range(1, rows)], slots))
                am = np.zeros(slots * rows, np.uint32)
                forms = {} if tree_only else {"runs": lambda: chk(lib.lmrs_batch_forward_runs(b, slots, p(sl), p(st), p(n), p(n), p(tok), p(am), None, 0, None, None))}
                if has_tree and (tree_only or not traced):
                    forms["tree"] = lambda: chk(lib.lmrs_batch_forward_tree(b, slots, p(sl), p(st), p(n), p(par), p(tok), p(am), None, 0, None, None))
                for k, r in turns(forms).items():
                    say(f"{kind}:{slots}x{rows}@{depth}:{k}", r)
            if kind == "wide" and depth == 100:
                for rows in () if tree_only else (16, 64):
                    sl, tok, pos, am = u(range(rows)), u([prompt[depth]] * rows), u([depth] * rows), np.zeros(rows, np.uint32)
                    say(f"forward:{rows}@{depth}", turns({"f": lambda: chk(lib.lmrs_batch_forward(b, rows, p(sl), p(tok), p(pos), p(am), None))})["f"])
                if has_tree and (tree_only or not traced):   # a 16-node tree a slot, then the path 0, 1, 3, 7 -> .. accepted: 4 of 16, rows 3 and 7 move
                    sl, st, n = u(range(16)), u([depth] * 16), u([16] * 16)
                    tok, par = u(np.tile(prompt[depth:depth + 16], 16)), u(np.tile([0xFFFFFFFF] + [(j - 1) // 2 for j in range(1, 16)], 16))
                    am, plen, path = np.zeros(256, np.uint32), u([4] * 16), u([0, 1, 3, 7] * 16)
                    chk(lib.lmrs_batch_forward_tree(b, 16, p(sl), p(st), p(n), p(par), p(tok), p(am), None, 0, None, None))
                    say("accept:16x4of16", turns({"a": lambda: chk(lib.lmrs_batch_accept_path(b, 16, p(sl), p(st), p(plen), p(path)))}, passes=1)["a"])
            lib.lmrs_batch_destroy(b)
    if not traced:
        ids, sec, us = np.zeros(STEPS, np.uint32), C.c_double(), []
        for _ in range(4):
            chk(lib.lmrs_generate_greedy(h, p(prompt), 10, STEPS, 0, p(ids), C.byref(sec)))
            us.append(sec.value * 1e6 / STEPS)
        say("decode:1@10", (statistics.median(us[1:]), min(us[1:]), max(us[1:])))


def tree_main(argv):
    """--tree [--parent-lib PATH] [model] [q8_0|q4_0]: tree_child a process per library by turns (the parent commit's, this build's; two turns), then the
    conditions: (1) a tree pass is no slower than the PARENT's lmrs_batch_forward_runs pass of equal rows by more than the parent's spread over its turns plus
    the cost of the one extra upload (tree against runs at one node a slot, this build); (2) this build's forward_runs, forward at 16 and 64 rows and the
    decode step stay within the parent's spread.  A MISS is printed as a MISS with its size.  Last, under rocprofv3 --kernel-trace in processes of their own: the
    launch lists of the calls both libraries have, compared, and the tree kernels' times (tree_commit_kernel: a 4-of-16 path on 16 slots)."""
    import csv, glob, shutil, subprocess, tempfile  # noqa: E401
    parent = os.environ.get("BATCH_RATE_PARENT_LIB")
    if argv and argv[0] == "--parent-lib":
        parent, argv = argv[1], argv[2:]
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    say(f"python tools/batch_rate.py --tree --parent-lib <the parent commit's liblmrs_hip.so> {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}")
    say(f"us per pass, host time of synchronous calls ({TREE_PASSES} passes a call); in a process the forms by turns, three turns of 3 calls after 1 warm-up; "
        "a process per library by turns, two turns; per figure the mean of the processes' medians (their distance apart)")
    libs = [("this", lmrs_amd.LIB_PATH)] + ([("parent", os.path.abspath(parent))] if parent and os.path.exists(parent) else [])
    if len(libs) == 1:
        say("no parent library given (--parent-lib PATH): the conditions against the parent are not judged")
    me, res = os.path.abspath(__file__), {}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "model.lmrs")
        S.build_image(model, qt, 1234).tofile(path); np.ascontiguousarray(S.prompt_tokens(model, 1100, 100), np.uint32).tofile(path + ".prompt")
        for turn in range(2):
            for who, lib in libs:
                r = subprocess.run([sys.executable, me, "--tree-child", path], env=dict(os.environ, LMRS_LIB=lib), capture_output=True, text=True, timeout=900)
                if r.returncode:
                    say(f"  {who}, turn {turn}: failed: {r.stderr.strip()[-300:]}")
                for l in r.stdout.splitlines():
                    if l.startswith("TREE "):
                        res.setdefault((who, l.split()[1]), []).append(float(l.split()[2]))
        mean = lambda who, k: statistics.mean(res[(who, k)])
        gap = lambda who, k: max(res[(who, k)]) - min(res[(who, k)])
        misses = 0
        say("condition 1 - the tree pass against the parent's forward_runs pass of equal rows (binary trees; kind:slots x rows@prefix):")
        for kind in ("wide", "paged"):
            for depth in (100, 1000):
                for slots, rows in TREE_SHAPES:
                    k = f"{kind}:{slots}x{rows}@{depth}"
                    t, own = mean("this", k + ":tree"), mean("this", k + ":runs")
                    line = f"  {k:18s} tree {t:8.1f} ({gap('this', k + ':tree'):.1f})   this build's runs {own:8.1f} ({t / own - 1:+.1%})"
                    if len(libs) > 1:
                        one = f"{kind}:{1 if slots == 1 else 16}x1@{depth}"          # (the 8-slot shape: the 16-slot upload, the larger table)
                        up = max(0.0, mean("this", one + ":tree") - mean("this", one + ":runs"))
                        pr, allow = mean("parent", k + ":runs"), gap("parent", k + ":runs") + up
                        miss = t > pr + allow
                        misses += miss
                        line += f"   parent's runs {pr:8.1f} ({t / pr - 1:+.1%}; allowed {allow:.1f} = its turns {gap('parent', k + ':runs'):.1f} + upload {up:.1f})"
                        line += f"   ** MISS by {t - pr - allow:.1f} us **" if miss else ""
                    say(line)
        if len(libs) > 1:
            say("condition 2 - existing calls against the parent (a MISS: slower by more than the parent's turns are apart):")
            keys = [f"{kind}:{s}x{r}@{d}:runs" for kind in ("wide", "paged") for d in (100, 1000) for s, r in TREE_SHAPES] + ["forward:16@100", "forward:64@100", "decode:1@10"]
            for k in keys:
                a, pr, g = mean("this", k), mean("parent", k), gap("parent", k)
                misses += a > pr + g
                say(f"  {k:24s} this {a:8.1f}   parent {pr:8.1f} ({a / pr - 1:+.1%}; parent's turns {g:.1f} apart)" + (f"   ** MISS by {a - pr - g:.1f} us **" if a > pr + g else ""))
            say(f"  MISSES in all: {misses}")
        r = res.get(("this", "accept:16x4of16"))
        say(f"lmrs_batch_accept_path, a 4-of-16 path on 16 slots (two rows a slot move), host time of the synchronous call: {statistics.mean(r):.1f} us" if r else "accept: not run")
        say("launch lists under rocprofv3 --kernel-trace, a process each: forward_runs 16 x 16 and forward at 16 and 64 rows on a wide and a paged batch, per library; "
            "then this build's tree pass and accept alone")
        counts = {}
        for who, lib, mode in [(w, l, "traced") for w, l in libs] + [("this, tree", lmrs_amd.LIB_PATH, "traced-tree")] if shutil.which("rocprofv3") else ():
            with tempfile.TemporaryDirectory() as tt:
                r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tt, "--", sys.executable, me, "--tree-child", path, mode],
                                   env=dict(os.environ, LMRS_LIB=lib), capture_output=True, text=True, timeout=900)
                traces = glob.glob(os.path.join(tt, "**", "*kernel_trace.csv"), recursive=True)
                if r.returncode or not traces:
                    say(f"  {who}: failed: {r.stderr.strip()[-300:]}")
                    continue
                rows = list(csv.DictReader(open(traces[0])))
                counts[who] = {}
                for x in rows:
                    name = x["Kernel_Name"].split("(")[0]
                    counts[who][name] = counts[who].get(name, 0) + 1
                say(f"  {who}: {sum(counts[who].values())} launches of {len(counts[who])} kernels")
                for kern in ("tree_scatter_kernel", "tree_attn_kernel", "tree_commit_kernel") if mode == "traced-tree" else ():
                    us = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in rows if kern in x["Kernel_Name"]]
                    say(f"    {kern:20s} {len(us):3d} launches  median {statistics.median(us):8.2f} us ({min(us):.2f} .. {max(us):.2f})" if us else f"    {kern}: no launch")
        if not shutil.which("rocprofv3"):
            say("  not run: rocprofv3 is not on the PATH")
        if "this" in counts and "parent" in counts:
            diff = {k: (counts["this"].get(k, 0), counts["parent"].get(k, 0)) for k in set(counts["this"]) | set(counts["parent"]) if counts["this"].get(k, 0) != counts["parent"].get(k, 0)}
            say(f"  launch lists of the existing calls identical between the libraries: {not diff}" + (f"   (this, parent): {diff}" if diff else ""))
    name = TREE_OUT.get((model, qt))
    out = os.environ.get("BATCH_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--tree-child":
        return tree_child(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "")
    if len(sys.argv) > 1 and sys.argv[1] == "--tree":
        return tree_main(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--paged-prefill":
        return paged_prefill_main(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--wide":
        return wide_main(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--kvq-child":
        return kvq_child(sys.argv[2], sys.argv[3], len(sys.argv) > 4)
    if len(sys.argv) > 1 and sys.argv[1] == "--kvq":
        return kvq_main(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--paged":
        return paged_main(sys.argv[2:])
    model = sys.argv[1] if len(sys.argv) > 1 else "llama-3.2-1b"
    qname = sys.argv[2] if len(sys.argv) > 2 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    b = lmrs_amd.Batch(m, ROWS)
    say(f"python tools/batch_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}")
    say(f"{STEPS} greedy steps per call, device time of the steps (HIP events inside the call); median of 5 after 2 warm-ups (min .. max)")
    first_win = None
    for depth in (100, 1030):
        prompts = [S.prompt_tokens(model, depth + 1, 100 + i) for i in range(ROWS)]        # row i: depth tokens in its cache, the next one fed first
        for i, p in enumerate(prompts):
            b.prefill(i, p[:depth], 0)
        singles = []
        for p in prompts:                                    # the single-sequence ids of every row's prompt, and the baseline's time from row 0's
            m.prefill_tokens(p[:depth], 0)
            singles.append(m.generate_greedy(p[depth:], STEPS, depth))
        m.prefill_tokens(prompts[0][:depth], 0)
        _, base, lo, hi = timed(lambda: m.generate_greedy(prompts[0][depth:], STEPS, depth, timing=True))
        base_rate = STEPS / base * 1e6
        say(f"rows at {depth} positions")
        say(f"  lmrs_generate_greedy (one sequence)   {base / STEPS:8.1f} us per step ({lo / STEPS:.1f} .. {hi / STEPS:.1f})   {base_rate:9.1f} tok/s")
        for n in ((1, 2, 4, 8, 16) if depth == 100 else (16,)):
            slots = list(range(n))
            ids, us, lo, hi = timed(lambda: b.generate_greedy(slots, [int(p[depth]) for p in prompts[:n]], [depth] * n, STEPS, timing=True))
            same = all(ids[i].tolist() == singles[i].tolist() for i in range(n))
            rate = n * STEPS / us * 1e6
            if depth == 100 and first_win is None and rate > base_rate:
                first_win = n
            say(f"  lmrs_batch_generate_greedy n={n:2d}       {us / STEPS:8.1f} us per pass ({lo / STEPS:.1f} .. {hi / STEPS:.1f})   {rate:9.1f} tok/s aggregate"
                f"   {rate / base_rate:5.2f}x the baseline   same tokens as the single-sequence runs: {same}")
        if depth == 100:
            say(f"  the batch first beats the baseline at n = {first_win}")
    # lmrs_batch_fork at full size (its V copy's pitch is seq_len x kv_dim x 4 bytes): slot 0's 1030 rows into slot 1 and from the context's own cache
    # into slot 2, the copied rows compared, and slot 1 continued as slot 0's prompt is
    depth, nl = 1030, m.args.n_layers
    t0 = time.perf_counter(); b.fork(0, 1, depth); fork_ms = (time.perf_counter() - t0) * 1e3
    m.prefill_tokens(prompts[0][:depth], 0)
    b.fork(lmrs_amd.BATCH_CTX, 2, depth)
    rows_equal = all((b.kv_row(dst, w, l, p).view(np.uint32) == b.kv_row(0, w, l, p).view(np.uint32)).all()
                     for dst in (1, 2) for w in (0, 1) for l in (0, nl // 2, nl - 1) for p in (0, 517, depth - 1))
    ids = b.generate_greedy([2, 1], [int(prompts[0][depth])] * 2, [depth] * 2, STEPS)
    same = ids[0].tolist() == ids[1].tolist() == singles[0].tolist()
    bytes_moved = 2 * nl * depth * m.args.n_kv_heads * m.args.head_size * 4
    say(f"lmrs_batch_fork of {depth} positions ({bytes_moved / 1e6:.1f} MB of K and V rows, host wall time of the synchronous call): {fork_ms:.2f} ms; "
        f"copied rows bit-equal: {rows_equal}; a forked slot continues with the single-sequence tokens: {same}")
    name = OUT.get((model, qt))
    if name:
        path = os.environ.get("BATCH_RATE_OUT") or os.path.join(ROOT, "profiles", name)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
