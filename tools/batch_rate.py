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
       python tools/batch_rate.py --paged-prefill [model] [q8_0|q4_0]
--paged-prefill: lmrs_batch_prefill of 16 .. 512 tokens on a wide batch, on paged batches (block attention over the page table from 16 rows on) and on the
same paged batches with lmrs_batch_debug_prefill_table (every chunk through the table pass: the routing before), the forms by turns (paged_prefill_main below)
       (writes profiles/batch_paged_prefill_llama1b.txt, profiles/batch_paged_prefill_gemma2b_q4.txt)"""
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


PREFILL_OUT = {("llama-3.2-1b", S.Q8_0): "batch_paged_prefill_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_paged_prefill_gemma2b_q4.txt"}
PREFILL_CASES = [(16, 0), (32, 0), (64, 0), (80, 0), (96, 0), (112, 0), (128, 0), (256, 0), (512, 0), (512, 512)]   # (tokens, start position); 80 .. 112: around the crossover


def paged_prefill_main(argv):
    """--paged-prefill [model] [q8_0|q4_0]: host wall time of the synchronous lmrs_batch_prefill call into slot 0, in one process, five forms by turns,
    three turns, median of 5 calls after 1 warm-up a turn: (a) the wide batch; (b) paged batches of page_len 64 and 256 under the library's routing; (c) the
    same two with lmrs_batch_debug_prefill_table(1) - every chunk through the table pass, one workgroup per (head, row).  Per form and length the median of
    its turns (fastest .. slowest turn), lmrs_batch_prefill_form's answer, and whether the forms leave the same last K row."""
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    say(f"python tools/batch_rate.py --paged-prefill {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}")
    say("lmrs_batch_prefill into slot 0, host wall time of the synchronous call: five forms by turns, three turns, median of 5 calls after 1 warm-up a turn; "
        "per form the median of its turns (fastest .. slowest turn); form = lmrs_batch_prefill_form's (chunks, of them block attention)")
    forms = [("wide", None, False), ("paged 64", 64, False), ("paged 256", 256, False), ("paged 64 table", 64, True), ("paged 256 table", 256, True)]
    prompt = S.prompt_tokens(model, 1024, 100)
    batches = {}
    for name, pl, table in forms:
        b = lmrs_amd.Batch(m, 2, wide=True) if pl is None else lmrs_amd.Batch(m, 2, page_len=pl, n_pages=2 * (1024 // pl))
        if table:
            b.debug_prefill_table(True)
        batches[name] = b
    nl = m.args.n_layers
    for n, start in PREFILL_CASES:
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
        w = statistics.median(turns["wide"])
        for name, pl, table in forms:
            t = turns[name]
            note = f"{statistics.median(t) / w:5.2f}x wide"
            if pl is not None and not table:
                old = turns[name + " table"]
                note += f"   {statistics.median(t) / statistics.median(old):5.2f}x its table pass; slowest turn below the table pass's fastest: {max(t) < min(old)}"
            say(f"  {n:3d} tokens at {start:3d}, {name:15s} form {batches[name].prefill_form(n, start)}  {statistics.median(t):8.3f} ms ({min(t):.3f} .. {max(t):.3f})   {note}")
        say(f"      the five forms leave the same last K row: {all((last[name] == last['wide']).all() for name, _, _ in forms)}")
    for b in batches.values():
        b.close()
    name = PREFILL_OUT.get((model, qt))
    path = os.environ.get("BATCH_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--paged-prefill":
        return paged_prefill_main(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--wide":
        return wide_main(sys.argv[2:])
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
