"""What lmrs_batch_generate costs and buys on a full-size synthetic model, one process per model: a wide batch, every row at 100 positions.  Host wall
time, call to return, median of 5 runs after 2 warm-ups (min .. max), the forms of a section taken by turns; every timed form's tokens are compared with
the per-step route's in the same run.
  a. the loop's overhead: no stops, argmax rows, 16 and 64 rows, 64 steps - us per pass of lmrs_batch_generate (check_every 8, and 64 = the budget) and of
     lmrs_batch_generate_greedy, the PARENT commit's library against this one by turns (--parent-lib PATH, or GENERATE_RATE_PARENT_LIB; without it the
     section runs this library only and says so), six child processes per library, by turns, over a binding of their own: every library's own
     process-to-process distribution stands in the file, and the condition is judged against it;
  b. what stopping buys: 64 rows whose ends are spread evenly between 8 and 128 tokens - tokens per second of useful output for check_every 1 .. 32,
     against (i) lmrs_batch_generate_greedy to 128 steps truncated on the host and (ii) one lmrs_batch_forward per step with the end test and the row
     removal in Python.  A row ends on a stop token of its own free-running sequence where that sequence offers one, on its budget elsewhere
     (the file says how many of each);
  c. the sampled loop: 16 and 64 sample_mult rows (0.8, 1.0), us per step against one lmrs_batch_forward_runs_sample per step;
  d. log-probabilities: us per step with and without out_logprobs, argmax rows and sample_mult rows (whose samplers then work on a copy of the logits);
  e. the boundary launch alone, beside the advance launches of lmrs_batch_generate_greedy: a rocprofv3 --kernel-trace --stats run of its own (a child
     process; skipped where rocprofv3 is missing) over 16 steps of each loop at 16 and 64 rows.
usage: python tools/generate_rate.py [--parent-lib PATH] [model] [q8_0|q4_0]
       (writes profiles/batch_generate_llama1b.txt for llama-3.2-1b q8_0, profiles/batch_generate_gemma2b_q4.txt for gemma-2-2b q4_0; GENERATE_RATE_OUT
       names another file)"""
import csv
import ctypes as C
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402

DEPTH, ROWS, STEPS, LONG = 100, 64, 64, 128
TURNS = 6                                                                              # processes per library in section a
OUT = {("llama-3.2-1b", S.Q8_0): "batch_generate_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_generate_gemma2b_q4.txt"}


def med(us):
    return statistics.median(us), min(us), max(us)


def prompts_of(V):
    rng = np.random.default_rng(33)
    return [rng.integers(0, V, DEPTH + 1).astype(np.uint32) for _ in range(ROWS)]


def overhead_child(image_path, V):
    """section a's child: the loops on the library LMRS_LIB names, over a binding of its own (the parent's library has no lmrs_batch_generate)"""
    lib = C.CDLL(os.environ.get("LMRS_LIB", os.path.join(ROOT, "lm.rs_amd", "liblmrs_hip.so")))
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.lmrs_last_error.restype = C.c_char_p
    lib.lmrs_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.lmrs_batch_create_wide.argtypes = [vp, u32, C.POINTER(vp)]
    lib.lmrs_batch_prefill.argtypes = [vp, u32, vp, sz, u32]
    lib.lmrs_batch_generate_greedy.argtypes = [vp, u32, vp, vp, vp, u32, vp, C.POINTER(C.c_double)]
    lib.lmrs_batch_destroy.argtypes = [vp]; lib.lmrs_batch_destroy.restype = None
    lib.lmrs_destroy.argtypes = [vp]; lib.lmrs_destroy.restype = None
    new = hasattr(lib, "lmrs_batch_generate")
    if new:
        lib.lmrs_batch_generate.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, C.POINTER(C.c_double)]

    def chk(rc):
        if rc:
            raise RuntimeError(lib.lmrs_last_error().decode())

    img = np.fromfile(image_path, np.uint8)
    h, used, b = vp(), sz(), vp()
    chk(lib.lmrs_create(img.ctypes.data, img.size, 0, C.byref(h), C.byref(used)))
    chk(lib.lmrs_batch_create_wide(h, ROWS, C.byref(b)))
    prompts = prompts_of(V)
    for i, p in enumerate(prompts):
        t = np.ascontiguousarray(p[:DEPTH])
        chk(lib.lmrs_batch_prefill(b, i, t.ctypes.data, t.size, 0))
    out = []
    for n in (16, ROWS):
        slot = np.arange(n, dtype=np.uint32); pos = np.full(n, DEPTH, np.uint32); budget = np.full(n, STEPS, np.uint32)
        tok = np.array([int(p[DEPTH]) for p in prompts[:n]], np.uint32)
        ids = np.zeros((n, STEPS), np.uint32); n_out = np.zeros(n, np.uint32); fin = np.zeros(n, np.uint32)
        forms = [("greedy", lambda: lib.lmrs_batch_generate_greedy(b, n, slot.ctypes.data, tok.ctypes.data, pos.ctypes.data, STEPS, ids.ctypes.data, None))]
        for ce in (8, STEPS) if new else ():
            forms.append((f"generate/{ce}", lambda ce=ce: lib.lmrs_batch_generate(b, n, slot.ctypes.data, tok.ctypes.data, pos.ctypes.data, budget.ctypes.data, None, None, None, ce,
                                                                                  ids.ctypes.data, None, n_out.ctypes.data, fin.ctypes.data, None, None)))
        us, sums = {k: [] for k, _ in forms}, {}
        for k in range(7):
            for name, call in forms:
                t0 = time.perf_counter()
                chk(call())
                dt = time.perf_counter() - t0
                sums[name] = int(ids.astype(np.uint64).sum())
                if k >= 2:
                    us[name].append(dt * 1e6 / STEPS)
        for name, _ in forms:
            out.append(f"{n}:{name}:" + ":".join(f"{x:.2f}" for x in med(us[name])) + f":{sums[name]}")
    lib.lmrs_batch_destroy(b); lib.lmrs_destroy(h)
    print("OVERHEAD " + " ".join(out), flush=True)


def traced_child(image_path):
    """section e's child (under rocprofv3): 16 steps of the greedy loop and of lmrs_batch_generate (argmax rows; then with samplers and log-probabilities)"""
    import lmrs_amd
    m = lmrs_amd.Transformer(np.fromfile(image_path, np.uint8))
    b = lmrs_amd.Batch(m, ROWS, wide=True)
    prompts = prompts_of(m.args.vocab_size)
    for i, p in enumerate(prompts):
        b.prefill(i, p[:DEPTH], 0)
    for n in (16, ROWS):
        s, t, p = list(range(n)), [int(x[DEPTH]) for x in prompts[:n]], [DEPTH] * n
        b.generate_greedy(s, t, p, 16)
        b.generate(s, t, p, 16, check_every=16)
    sm = [lmrs_amd.Sampler(m.args.vocab_size, 0.8, 1.0, 7 + i) for i in range(ROWS)]
    b.generate(list(range(ROWS)), [int(x[DEPTH]) for x in prompts], [DEPTH] * ROWS, 16, samplers=sm, check_every=16, logprobs=True)
    b.close(); m.close()


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--overhead-child":
        return overhead_child(argv[1], int(argv[2]))
    if argv and argv[0] == "--traced-child":
        return traced_child(argv[1])
    parent = os.environ.get("GENERATE_RATE_PARENT_LIB")
    if argv and argv[0] == "--parent-lib":
        parent, argv = argv[1], argv[2:]
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    import bench
    import lmrs_amd
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    V = S.CONFIGS[model].vocab_size
    say(f"python tools/generate_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234), vocabulary {V}; kernel_source_hash {bench.kernel_source_hash()}")
    say(f"a wide batch, rows at {DEPTH} positions; host wall time, call to return, median of 5 runs after 2 warm-ups (min .. max), forms by turns")
    say(f"a. the loop's overhead: argmax rows, no stops, {STEPS} steps; us per pass; a process per library and turn")
    have_parent = bool(parent and os.path.exists(parent))
    if not have_parent:
        say("    no parent library given (--parent-lib PATH): this library only")
    with tempfile.NamedTemporaryFile(suffix=".lmrs") as f:
        img.tofile(f.name)
        res = {}
        for turn in range(TURNS):
            for who, path in ((("parent", os.path.abspath(parent)),) if have_parent else ()) + (("this", lmrs_amd.LIB_PATH),):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--overhead-child", f.name, str(V)], env=dict(os.environ, LMRS_LIB=path),
                                   capture_output=True, text=True, timeout=900)
                got = [l for l in r.stdout.splitlines() if l.startswith("OVERHEAD ")]
                if r.returncode or not got:
                    say(f"    {who}, turn {turn}: failed: {r.stderr.strip()[-300:]}")
                    continue
                for item in got[0].split()[1:]:
                    n, name, m_, lo, hi, chk = item.split(":")
                    res.setdefault((int(n), who, name), []).append((float(m_), float(lo), float(hi), chk))
                    say(f"    turn {turn}  {who:6s}  {int(n):2d} rows  {name:12s} {float(m_):9.2f} us per pass ({lo} .. {hi})   token checksum {chk}")
        say("e. the boundary launch alone: rocprofv3 --kernel-trace --stats over a process of its own; us per launch, median (min .. max)")
        boundary = None
        if not shutil.which("rocprofv3"):
            say("    not run: rocprofv3 is not on the PATH")
        else:
            with tempfile.TemporaryDirectory() as td:
                r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--traced-child", f.name],
                                   capture_output=True, text=True, timeout=900)
                traces = glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True)
                if r.returncode or not traces:
                    say(f"    failed: {r.stderr.strip()[-300:]}")
                else:
                    rows = list(csv.DictReader(open(traces[0])))
                    for kern in ("table_advance_kernel", "runs_advance_kernel", "gen_advance_kernel", "gen_logprobs_kernel"):
                        us = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in rows if kern in x["Kernel_Name"]]
                        say(f"    {kern:22s} {len(us):3d} launches" + (f"   {statistics.median(us):6.2f} us ({min(us):.2f} .. {max(us):.2f})" if us else ""))
                        if kern == "gen_advance_kernel" and us:
                            boundary = statistics.median(us)
        say(f"a, summed up: every process's median per form; a library's figure = the median over its {TURNS} processes, its process-to-process spread = their range.  The condition: "
            "lmrs_batch_generate <= the parent's lmrs_batch_generate_greedy + the parent's own process-to-process spread + the boundary launch (e)")

        def over(key):
            v = [x[0] for x in res.get(key, [])]
            return (statistics.median(v), min(v), max(v), v) if v else None

        for n in (16, ROWS):
            this_g, par_g = over((n, "this", "greedy")), over((n, "parent", "greedy"))
            for who, g in (("parent", par_g), ("this", this_g)):
                if g:
                    say(f"    {n} rows  {who:6s} lmrs_batch_generate_greedy  median {g[0]:.2f} us per pass, processes {g[1]:.2f} .. {g[2]:.2f} (spread {g[2] - g[1]:.2f}): "
                        + " ".join(f"{x:.1f}" for x in g[3]))
            if this_g and par_g:
                lo, hi = max(this_g[1], par_g[1]), min(this_g[2], par_g[2])
                say(f"    {n} rows  the unchanged greedy loop, this library against the parent's: {this_g[0] - par_g[0]:+.2f} us on the medians; the two libraries' ranges of processes "
                    + (f"overlap ({lo:.2f} .. {hi:.2f})" if lo <= hi else f"do NOT overlap (a gap of {lo - hi:.2f} us)"))
            for ce in (8, STEPS):
                g = over((n, "this", f"generate/{ce}"))
                if not g:
                    continue
                own = [x[0] - y[0] for x, y in zip(res[(n, "this", f"generate/{ce}")], res[(n, "this", "greedy")])]
                same = {x[3] for x in res[(n, "this", f"generate/{ce}")]} == {x[3] for x in res[(n, "this", "greedy")]}
                line = (f"    {n} rows  lmrs_batch_generate check_every {ce:2d}: median {g[0]:.2f} us per pass, processes {g[1]:.2f} .. {g[2]:.2f}; beside this library's greedy loop in "
                        f"the same process {statistics.median(own):+.2f} us ({min(own):+.2f} .. {max(own):+.2f})")
                if par_g:
                    bound = par_g[2] - par_g[1] + (boundary or 0.0)
                    line += (f"; on the parent's greedy loop {g[0] - par_g[0]:+.2f} us ({(g[0] / par_g[0] - 1) * 100:+.3f} %), the bound {par_g[2] - par_g[1]:.2f} + "
                             f"{boundary or 0.0:.2f} = {bound:.2f} us: condition met: {g[0] - par_g[0] <= bound}")
                say(line + f"; same tokens as the greedy loop: {same}")
    m = lmrs_amd.Transformer(img)
    b = lmrs_amd.Batch(m, ROWS, wide=True)
    prompts = prompts_of(V)
    for i, p in enumerate(prompts):
        b.prefill(i, p[:DEPTH], 0)
    slots = list(range(ROWS))
    first = [int(p[DEPTH]) for p in prompts]
    pos = [DEPTH] * ROWS

    def timed(forms, per, runs=7):
        """forms: name -> call returning something comparable; by turns -> name -> (result, median, lo, hi) in us per `per`"""
        us, last = {k: [] for k in forms}, {}
        for k in range(runs):
            for name, call in forms.items():
                t0 = time.perf_counter()
                last[name] = call()
                dt = time.perf_counter() - t0
                if k >= 2:
                    us[name].append(dt * 1e6 / per)
        return {k: (last[k],) + med(us[k]) for k in forms}

    # ---- b
    ends = [int(round(8 + (LONG - 8) * i / (ROWS - 1))) for i in range(ROWS)]
    useful = sum(ends)
    # a row ends on a stop token where the free-running sequence allows it - the token of its last wanted step, when that step is its first occurrence -
    # and on its budget elsewhere (a model that repeats itself offers no such token)
    free = b.generate_greedy(slots, first, pos, LONG)
    stops, budgets = [], []
    for i in range(ROWS):
        t = int(free[i, ends[i] - 1])
        by_stop = free[i].tolist().index(t) == ends[i] - 1
        stops.append([t] if by_stop else []); budgets.append(LONG if by_stop else ends[i])
    n_stop = sum(1 for x in stops if x)
    say(f"b. what stopping buys: {ROWS} rows whose ends are spread evenly over 8 .. {LONG} tokens ({useful} useful tokens; {n_stop} rows end on a stop token taken from their "
        f"own free-running sequence, {ROWS - n_stop} on their budget); useful tokens per second of host wall time")

    def truncated():
        out = b.generate_greedy(slots, first, pos, LONG)
        return [out[i, :ends[i]].tolist() for i in range(ROWS)]

    def per_step():
        live, tok, outs = list(range(ROWS)), list(first), [[] for _ in range(ROWS)]
        j = 0
        while live:
            am = b.forward([slots[i] for i in live], [tok[i] for i in live], [DEPTH + j] * len(live))
            nxt = []
            for k, i in enumerate(live):
                outs[i].append(int(am[k])); tok[i] = int(am[k])
                if tok[i] not in stops[i] and len(outs[i]) < budgets[i]:
                    nxt.append(i)
            live, j = nxt, j + 1
        return outs

    def loop(ce):
        return lambda: [t.tolist() for t in b.generate(slots, first, pos, budgets, stop=stops, check_every=ce)[0]]

    forms = {"greedy loop to 128, truncated": truncated, "one lmrs_batch_forward per step": per_step}
    forms.update({f"lmrs_batch_generate check_every {ce:2d}": loop(ce) for ce in (1, 2, 4, 8, 16, 32)})
    got = timed(forms, 1)
    want = got["one lmrs_batch_forward per step"][0]
    for name, (ids, us, lo, hi) in got.items():
        say(f"    {name:36s} {us / 1e3:9.2f} ms ({lo / 1e3:.2f} .. {hi / 1e3:.2f})   {useful * 1e6 / us:9.0f} tok/s ({useful * 1e6 / hi:.0f} .. {useful * 1e6 / lo:.0f})"
            f"   same tokens as the per-step route: {ids == want}")
    sweep = {ce: got[f"lmrs_batch_generate check_every {ce:2d}"] for ce in (1, 2, 4, 8, 16, 32)}
    best = min(sweep, key=lambda ce: sweep[ce][1])
    spread = max(sweep[best][3] - sweep[best][2], sweep[8][3] - sweep[8][2])
    import inspect
    dflt = inspect.signature(lmrs_amd.Batch.generate).parameters["check_every"].default
    say(f"    the sweep's best: check_every {best}; check_every 8 is {(sweep[8][1] - sweep[best][1]) / 1e3:+.2f} ms ({(sweep[8][1] / sweep[best][1] - 1) * 100:+.2f} %) off it, the two forms' "
        f"own spread {spread / 1e3:.2f} ms: within it: {sweep[8][1] - sweep[best][1] <= spread}; Batch.generate's default, check_every {dflt}, is "
        f"{(sweep[dflt][1] / sweep[best][1] - 1) * 100 if dflt in sweep else float('nan'):+.2f} % off it")
    assert [len(x) for x in want] == ends, "a row did not end where it was wanted"
    # ---- c
    say("c. the sampled loop: sample_mult rows (0.8, 1.0), 32 steps; us per step")
    for n in (16, ROWS):
        sm = [lmrs_amd.Sampler(V, 0.8, 1.0, 7 + i) for i in range(n)]

        def stepwise(n=n, sm=sm):
            tok, outs = list(first[:n]), []
            for j in range(32):
                tok = b.forward_runs_sample([(i, DEPTH + j, [tok[i]], sm[i]) for i in range(n)]).tolist()
                outs.append(tok)
            return np.array(outs).T.tolist()
        got = timed({"per step": stepwise, "loop": lambda n=n, sm=sm: [t.tolist() for t in b.generate(slots[:n], first[:n], pos[:n], 32, samplers=sm, check_every=32)[0]]}, 32)
        (ids_s, us_s, lo_s, hi_s), (ids_l, us_l, lo_l, hi_l) = got["per step"], got["loop"]
        say(f"    {n:2d} rows: lmrs_batch_forward_runs_sample per step {us_s:9.1f} us ({lo_s:.1f} .. {hi_s:.1f})   lmrs_batch_generate {us_l:9.1f} ({lo_l:.1f} .. {hi_l:.1f})"
            f"   {us_l - us_s:+8.1f} us per step   same tokens: {ids_s == ids_l}")
    # ---- d
    say(f"d. log-probabilities: {ROWS} rows, 32 steps, check_every 32; us per step with and without out_logprobs")
    sm = [lmrs_amd.Sampler(V, 0.8, 1.0, 7 + i) for i in range(ROWS)]
    for what, samplers in (("argmax rows", None), ("sample_mult rows (the samplers work on a copy of the logits)", sm)):
        got = timed({"without": lambda s=samplers: [t.tolist() for t in b.generate(slots, first, pos, 32, samplers=s, check_every=32)[0]],
                     "with": lambda s=samplers: [t.tolist() for t in b.generate(slots, first, pos, 32, samplers=s, check_every=32, logprobs=True)[0]]}, 32)
        (ids0, us0, lo0, hi0), (ids1, us1, lo1, hi1) = got["without"], got["with"]
        say(f"    {what}: without {us0:9.1f} us ({lo0:.1f} .. {hi0:.1f})   with {us1:9.1f} ({lo1:.1f} .. {hi1:.1f})   {us1 - us0:+7.1f} us per step   same tokens: {ids0 == ids1}")
    b.close(); m.close()
    name = OUT.get((model, qt))
    path = os.environ.get("GENERATE_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
