"""What a SAMPLED multi-sequence decode step costs on a full-size synthetic model, in one process: lmrs_batch_forward_sample (the pass, then Sampler::sample
per row on the device) against the existing-calls route - lmrs_batch_forward with logits, then lmrs_sampler_sample per row on the host - at n = 1, 2, 4, 8, 16
rows standing at 100 positions, for a sample_mult sampler (0.8, 1.0), a peaked top-p (temperature 0.02, top_p 0.9), the default flags' top-p (0.7, 0.9: flat
on synthetic weights, every row sorted on the device) and, beside them, lmrs_batch_forward without logits (greedy: the pass alone).  Host wall time per step
from call to return - the host's finishing is part of the feature: 8 steps a run, each row fed its own token, median of 5 runs after 2 warm-ups (min .. max);
every run starts from fresh samplers, and the tokens of every timed configuration are compared with the existing-calls route's.  Last, the device time of
the sampling kernels alone with both chains at full length, as cycles per term.
--wide: the same question for lmrs_batch_forward_runs_sample on a WIDE batch at 16, 32, 47, 48 and 64 rows - runs of one token, against lmrs_batch_forward
with logits and lmrs_sampler_sample per row, code that call does not touch - and, for the flat rows' common sort, lmrs_batch_forward_sample (one sort and one
synchronise per flat row) against the new call at 16 flat top-p rows, the two by turns in the same process.
usage: python tools/sample_rate.py [--wide] [model] [q8_0|q4_0]
       (writes profiles/batch_sample_llama1b.txt for llama-3.2-1b q8_0, profiles/batch_sample_gemma2b_q4.txt for gemma-2-2b q4_0; with --wide
       profiles/batch_sample_wide_llama1b.txt and profiles/batch_sample_wide_gemma2b_q4.txt)"""
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

STEPS, ROWS, DEPTH = 8, 16, 100
OUT = {("llama-3.2-1b", S.Q8_0): "batch_sample_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_sample_gemma2b_q4.txt"}
KINDS = [("sample_mult (0.8, 1.0)", 0.8, 1.0), ("peaked top-p (0.02, 0.9)", 0.02, 0.9), ("flat top-p (0.7, 0.9)", 0.7, 0.9)]


WIDE_ROWS = (16, 32, 47, 48, 64)


def main_wide(model, qname, qt):
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    b = lmrs_amd.Batch(m, 64, wide=True)
    V = m.args.vocab_size
    say(f"python tools/sample_rate.py --wide {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234), vocabulary {V}; kernel_source_hash {bench.kernel_source_hash()}")
    say(f"a wide batch, rows at {DEPTH} positions; host wall time per step, call to return; {STEPS} steps a run, median of 5 runs after 2 warm-ups (min .. max)")
    prompts = [S.prompt_tokens(model, DEPTH + 1, 100 + i) for i in range(64)]
    for i, p in enumerate(prompts):
        b.prefill(i, p[:DEPTH], 0)

    def run(n, step):
        slots, toks, ids, t = list(range(n)), [int(p[DEPTH]) for p in prompts[:n]], [], 0.0
        for j in range(STEPS):
            pos = [DEPTH + j] * n
            t0 = time.perf_counter()
            toks = step(slots, toks, pos)
            t += time.perf_counter() - t0
            ids.append(list(map(int, toks)))
        return ids, t / STEPS * 1e6

    def stats(runs):
        us = [u for _, u in runs]
        return runs[-1][0], statistics.median(us), min(us), max(us)

    def timed(n, make_step):
        return stats([run(n, make_step()) for _ in range(7)][2:])

    def samplers(n, temp, top_p):
        return [lmrs_amd.Sampler(V, temp, top_p, 7 + i) for i in range(n)]

    def new_route(n, temp, top_p):
        sm = samplers(n, temp, top_p)
        return lambda s, t, p: b.forward_runs_sample([(s[i], p[i], [t[i]], sm[i]) for i in range(n)])

    def old_route(n, temp, top_p):
        sm = samplers(n, temp, top_p)

        def step(s, t, p):
            _, lg = b.forward(s, t, p, logits=True)
            return [sm[i].sample(lg[i]) for i in range(n)]
        return step

    verdict = {}
    for n in WIDE_ROWS:
        say(f"n = {n}")
        _, g, lo, hi = timed(n, lambda: (lambda s, t, p: b.forward(s, t, p)))
        say(f"  lmrs_batch_forward, no logits (greedy)                 {g:9.1f} us per step ({lo:.1f} .. {hi:.1f})")
        for name, temp, top_p in KINDS:
            ids_old, old, olo, ohi = timed(n, lambda: old_route(n, temp, top_p))
            ids_new, new, nlo, nhi = timed(n, lambda: new_route(n, temp, top_p))
            verdict[(n, name)] = (old / new, old - new > ohi - olo)
            say(f"  {name:26s} lmrs_batch_forward_runs_sample {new:9.1f} us per step ({nlo:.1f} .. {nhi:.1f})   existing calls {old:9.1f} ({olo:.1f} .. {ohi:.1f})"
                f"   {old / new:5.2f}x   sampler's own cost {new - g:8.1f} us   same tokens: {ids_new == ids_old}")
    say("conditions")
    for n in (32, 64):
        for name, _, _ in KINDS:
            ratio, clear = verdict[(n, name)]
            say(f"  n = {n} {name}: faster than the existing calls by more than their spread: {clear} ({ratio:.2f}x)")
    # the common sort of the flat rows, A/B without a switch: the two calls by turns, one run each a turn
    name, temp, top_p = KINDS[2]
    say(f"the flat rows' sort, n = 16 {name}, by turns in this process: lmrs_batch_forward_sample (a sort and a synchronise per flat row) / "
        "lmrs_batch_forward_runs_sample (one sort, one synchronise)")

    def serial_route():
        sm = samplers(16, temp, top_p)
        return lambda s, t, p: b.forward_sample(s, t, p, sm)
    a_runs, b_runs = [], []
    for _ in range(7):
        a_runs.append(run(16, serial_route()))
        b_runs.append(run(16, new_route(16, temp, top_p)))
    ids_a, a, alo, ahi = stats(a_runs[2:])
    ids_b, bb, blo, bhi = stats(b_runs[2:])
    say(f"  lmrs_batch_forward_sample      {a:9.1f} us per step ({alo:.1f} .. {ahi:.1f})")
    say(f"  lmrs_batch_forward_runs_sample {bb:9.1f} us per step ({blo:.1f} .. {bhi:.1f})   {a / bb:5.2f}x   same tokens: {ids_a == ids_b}")
    say(f"  the common sort is faster by more than the spread of lmrs_batch_forward_sample's runs: {a - bb > ahi - alo}")
    name = {("llama-3.2-1b", S.Q8_0): "batch_sample_wide_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_sample_wide_gemma2b_q4.txt"}.get((model, qt))
    if name:
        path = os.environ.get("SAMPLE_RATE_OUT") or os.path.join(ROOT, "profiles", name)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    wide = "--wide" in sys.argv
    if wide:
        sys.argv.remove("--wide")
    model = sys.argv[1] if len(sys.argv) > 1 else "llama-3.2-1b"
    qname = sys.argv[2] if len(sys.argv) > 2 else "q8_0"
    if wide:
        return main_wide(model, qname, S.Q4_0 if qname == "q4_0" else S.Q8_0)
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    b = lmrs_amd.Batch(m, ROWS)
    V = m.args.vocab_size
    say(f"python tools/sample_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234), vocabulary {V}; kernel_source_hash {bench.kernel_source_hash()}")
    say(f"rows at {DEPTH} positions; host wall time per step, call to return; {STEPS} steps a run, median of 5 runs after 2 warm-ups (min .. max)")
    prompts = [S.prompt_tokens(model, DEPTH + 1, 100 + i) for i in range(ROWS)]
    for i, p in enumerate(prompts):
        b.prefill(i, p[:DEPTH], 0)

    def run(n, step):
        """STEPS steps of `step(toks, pos) -> next` from the prompts' ends -> (the ids [STEPS, n], microseconds per step)"""
        slots, toks, ids, t = list(range(n)), [int(p[DEPTH]) for p in prompts[:n]], [], 0.0
        for j in range(STEPS):
            pos = [DEPTH + j] * n
            t0 = time.perf_counter()
            toks = step(slots, toks, pos)
            t += time.perf_counter() - t0
            ids.append(list(map(int, toks)))
        return ids, t / STEPS * 1e6

    def timed(n, make_step):
        runs = [run(n, make_step()) for _ in range(7)][2:]
        us = [u for _, u in runs]
        return runs[-1][0], statistics.median(us), min(us), max(us)

    verdict = {}
    for n in (1, 2, 4, 8, 16):
        say(f"n = {n}")
        _, g, lo, hi = timed(n, lambda: (lambda s, t, p: b.forward(s, t, p)))
        say(f"  lmrs_batch_forward, no logits (greedy)            {g:9.1f} us per step ({lo:.1f} .. {hi:.1f})")
        for name, temp, top_p in KINDS:
            def new_route():
                sm = [lmrs_amd.Sampler(V, temp, top_p, 7 + i) for i in range(n)]
                return lambda s, t, p: b.forward_sample(s, t, p, sm)

            def old_route():
                sm = [lmrs_amd.Sampler(V, temp, top_p, 7 + i) for i in range(n)]

                def step(s, t, p):
                    _, lg = b.forward(s, t, p, logits=True)
                    return [sm[i].sample(lg[i]) for i in range(n)]
                return step
            ids_old, old, olo, ohi = timed(n, old_route)
            ids_new, new, nlo, nhi = timed(n, new_route)
            verdict[(n, name)] = old / new
            say(f"  {name:26s} lmrs_batch_forward_sample {new:9.1f} us per step ({nlo:.1f} .. {nhi:.1f})   existing calls {old:9.1f} ({olo:.1f} .. {ohi:.1f})"
                f"   {old / new:5.2f}x   sampler's own cost {new - g:8.1f} us   same tokens: {ids_new == ids_old}")
    say("conditions")
    for n in (16, 4):
        for name, _, _ in KINDS[:2]:
            say(f"  n = {n:2d} {name}: faster than the existing calls: {verdict[(n, name)] > 1.0} ({verdict[(n, name)]:.2f}x)")
    say(f"  n = 16 {KINDS[2][0]}: not slower than the existing calls: {verdict[(16, KINDS[2][0])] >= 1.0} ({verdict[(16, KINDS[2][0])]:.2f}x)")
    say("the sampling kernels alone, both chains over all of the vocabulary (lmrs_bench_sample_rows: HIP events on every dispatch, mean of 5 runs)")
    names = ["scale + maxima", "exponentials", "sum chain", "division + candidate counts", "cdf chain", "ordered candidates (no top-p row: nothing to do)"]
    for rows in (1, 16):
        us, mhz = lmrs_amd.bench_sample_rows(rows, V, 5)
        say(f"  {rows:2d} rows: " + "; ".join(f"{nm} {u:.1f} us" for nm, u in zip(names, us)))
        say(f"           sum chain {us[2] * mhz / V:.2f} cycles per term, cdf chain {us[4] * mhz / V:.2f} (nominal clock {mhz:.0f} MHz; tools/ubench/addlat.hip: 4.0 for an isolated chain)")
    name = OUT.get((model, qt))
    if name:
        path = os.environ.get("SAMPLE_RATE_OUT") or os.path.join(ROOT, "profiles", name)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
