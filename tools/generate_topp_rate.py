"""What lmrs_batch_generate_topp costs on a full-size synthetic model: a wide batch, 16 and 64 rows standing at 100 positions, 128 tokens a row, every row
a top-p sampler of its own - peaked (temperature 0.02, top_p 0.9) or the default flags' (0.7, 0.9: flat on synthetic weights).  The yardstick is the only
other way to run such rows: one lmrs_batch_forward_runs_sample call per step.  The two run by turns in the same process, each from fresh samplers, host
wall time from call to return - the loop's upload and download of the candidate vectors included - median of 5 runs after 2 warm-ups (min .. max); the
tokens and the samplers' vectors of the two routes are compared in every run.  Beside them the loop with sample_mult rows (0.8, 1.0), and the device time
of the new launches alone from HIP events on their own dispatches (lmrs_bench_topp_rows: the launches over rows of n0 candidates each).
usage: python tools/generate_topp_rate.py [model] [q8_0|q4_0]
       (writes profiles/batch_generate_topp_llama1b.txt for llama-3.2-1b q8_0, profiles/batch_generate_topp_gemma2b_q4.txt for gemma-2-2b q4_0;
       GENERATE_TOPP_RATE_OUT names another file)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402

DEPTH, ROWS, STEPS = 100, 64, 128
KINDS = [("peaked top-p (0.02, 0.9)", 0.02, 0.9), ("flat top-p (0.7, 0.9)", 0.7, 0.9)]
OUT = {("llama-3.2-1b", S.Q8_0): "batch_generate_topp_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_generate_topp_gemma2b_q4.txt"}


def main():
    argv = sys.argv[1:]
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    import bench
    import lmrs_amd as L
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    V = S.CONFIGS[model].vocab_size
    say(f"python tools/generate_topp_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234), vocabulary {V}; kernel_source_hash {bench.kernel_source_hash()}")
    say(f"a wide batch, rows at {DEPTH} positions, {STEPS} tokens a row; host wall time, call to return, median of 5 runs after 2 warm-ups (min .. max), the routes by turns")
    m = L.Transformer(img); b = L.Batch(m, ROWS, wide=True)
    rng = np.random.default_rng(33)
    prompts = [rng.integers(0, V, DEPTH + 1).astype(np.uint32) for _ in range(ROWS)]
    for i, p in enumerate(prompts):
        b.prefill(i, p[:DEPTH], 0)
    first = [int(p[DEPTH]) for p in prompts]
    misses = []
    for name, temp, top_p in KINDS:
        for n in (16, ROWS):
            slots, pos = list(range(n)), [DEPTH] * n
            us = {"per step": [], "loop": []}
            same = True
            for run in range(7):
                sa = [L.Sampler(V, temp, top_p, 7 + i) for i in range(n)]
                t0 = time.perf_counter()
                tok, outs = list(first[:n]), []
                for j in range(STEPS):
                    tok = b.forward_runs_sample([(i, DEPTH + j, [tok[i]], sa[i]) for i in range(n)]).tolist()
                    outs.append(tok)
                t1 = time.perf_counter()
                sb = [L.Sampler(V, temp, top_p, 7 + i) for i in range(n)]
                t2 = time.perf_counter()
                got = b.generate_topp(slots, first[:n], pos, STEPS, samplers=sb, check_every=STEPS)
                t3 = time.perf_counter()
                same = same and np.array(outs).T.tolist() == [t.tolist() for t in got[0]] and all(x.candidates()[0].tobytes() == y.candidates()[0].tobytes() for x, y in zip(sa, sb))
                if run >= 2:
                    us["per step"].append((t1 - t0) * 1e6 / STEPS); us["loop"].append((t3 - t2) * 1e6 / STEPS)
            (ms, ls, hs), (ml, ll, hl) = [(statistics.median(v), min(v), max(v)) for v in (us["per step"], us["loop"])]
            ok = ml <= ms
            if not ok:
                misses.append(f"{name}, {n} rows")
            say(f"    {name}, {n:2d} rows: lmrs_batch_forward_runs_sample per step {ms:9.1f} us ({ls:.1f} .. {hs:.1f})   lmrs_batch_generate_topp {ml:9.1f} ({ll:.1f} .. {hl:.1f})"
                f"   {ml - ms:+9.1f} us per step   no larger: {ok}   same tokens and vectors: {same}")
    say("the condition (the loop's time per step no larger than the per-call route's in every case): " + ("met" if not misses else "MISSED for " + "; ".join(misses)))
    # the loop with sample_mult rows beside it, and the upload / download alone
    for n in (16, ROWS):
        sm = [L.Sampler(V, 0.8, 1.0, 7 + i) for i in range(n)]
        us = []
        for run in range(5):
            t0 = time.perf_counter()
            b.generate(list(range(n)), first[:n], [DEPTH] * n, STEPS, samplers=sm, check_every=STEPS)
            if run >= 2:
                us.append((time.perf_counter() - t0) * 1e6 / STEPS)
        say(f"    sample_mult (0.8, 1.0), {n:2d} rows: lmrs_batch_generate {statistics.median(us):9.1f} us per step ({min(us):.1f} .. {max(us):.1f})")
    for n in (16, ROWS):
        # one step of n top-p rows from used samplers: the call's time less a pass is dominated by the vectors' way up and down
        ss = [L.Sampler(V, 0.7, 0.9, 7 + i) for i in range(n)]
        b.generate_topp(list(range(n)), first[:n], [DEPTH] * n, 1, samplers=ss)
        us1, us0 = [], []
        for run in range(5):
            t0 = time.perf_counter(); b.generate_topp(list(range(n)), first[:n], [DEPTH] * n, 1, samplers=ss); us1.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter(); b.generate(list(range(n)), first[:n], [DEPTH] * n, 1); us0.append((time.perf_counter() - t0) * 1e6)
        say(f"    one-step calls, {n:2d} rows: lmrs_batch_generate_topp with used flat samplers {statistics.median(us1):9.1f} us, lmrs_batch_generate (argmax) {statistics.median(us0):9.1f} us:"
            f" the vectors up and down, the sampling launches and one sort, merge and draw cost {statistics.median(us1) - statistics.median(us0):9.1f} us a call"
            f" ({n} x {V * 8} bytes each way); the merge reads and writes {n} x 2 x {V * 8} bytes a step")
    # the new launches alone
    say("the new launches alone (HIP events on each dispatch, summed; rows of n0 candidates each over used vectors), us per step:")
    for n in (16, ROWS):
        for n0 in (8, V // 2, V - V // 8):
            us, launches = L.bench_topp_rows(n, V, n0)
            say(f"    {n:2d} rows, n0 {n0:6d}: {us:9.1f} us in {launches} launches")
    b.close(); m.close()
    name = OUT.get((model, qt))
    path = os.environ.get("GENERATE_TOPP_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
