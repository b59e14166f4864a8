"""What the per-slot token record and the penalties over it (lmrs_batch_set_penalties) cost on a full-size synthetic model, one process per model: a wide
batch of 64 slots, every row's record drawn from a 300-token alphabet.
  1. unchanged when unused: lmrs_batch_generate_greedy of 64 rows on a batch that never set penalties, at 100 and 1000 positions, the parent commit's
     library against this one by turns (--parent-lib PATH, or PENALTY_RATE_PARENT_LIB; without it the section says so) - device time of 64 steps a call
     (HIP events inside the call), median of 5 calls after 2 warm-ups, a child process per library and turn, over a binding of its own of old entry points;
  2. cost when used: the same call on this build - no record, the record alone, all 64 rows under "all" (1.7, 0.5, 0.25, out_from 3) - by turns at 100
     and 1000 positions, median of 5 turns after 2 warm-ups; the turns' own differences are the record launch and the penalty launch per step, beside
     DESIGN.md section 3.5's launch model - 2.4 us + bytes / 6.3 TB/s; tok/s of the 64-step loops with and without penalties;
  3. the two launches alone, from a rocprofv3 --kernel-trace --stats run of its own (a child process; skipped where rocprofv3 is missing) at 100, 1000
     and 2047 positions;
  4. against the host route the penalties replace: lmrs_batch_forward_runs with logits, the rule in numpy per row, lmrs_sampler_sample per row on the host -
     for a sample_mult sampler (0.8, 1.0), a peaked top-p (0.02, 0.9) and the default flags' top-p (0.7, 0.9); host wall time per step, call to return, 8
     steps a run, median of 5 runs after 2 warm-ups, the tokens of the two routes compared.
usage: python tools/penalty_rate.py [--parent-lib PATH] [model] [q8_0|q4_0]
       (writes profiles/batch_penalty_llama1b.txt for llama-3.2-1b q8_0, profiles/batch_penalty_gemma2b_q4.txt for gemma-2-2b q4_0; PENALTY_RATE_OUT names
       another file)"""
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

STEPS, ROWS, GREEDY_STEPS, ALPHABET = 8, 64, 64, 300
DEPTHS, DEEP = (100, 1000), 2047
ALL = dict(repetition=1.7, presence=0.5, frequency=0.25, out_from=3)
OUT = {("llama-3.2-1b", S.Q8_0): "batch_penalty_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_penalty_gemma2b_q4.txt"}
KINDS = [("sample_mult (0.8, 1.0)", 0.8, 1.0), ("peaked top-p (0.02, 0.9)", 0.02, 0.9), ("flat top-p (0.7, 0.9)", 0.7, 0.9)]
LAUNCH_US, HBM_BYTES_PER_US = 2.4, 6.3e6
NONE = 0xFFFFFFFF


def med(us):
    return statistics.median(us), min(us), max(us)


def prompts_of(V, depth):
    """row i's depth + 1 tokens over an alphabet of its own model-wide: records with repeats"""
    rng = np.random.default_rng(21)
    alpha = rng.choice(V, ALPHABET, replace=False).astype(np.uint32)
    return [alpha[rng.integers(0, ALPHABET, depth + 1)] for _ in range(ROWS)]


def unused_passes(image_path):
    """measurement 1's child: the greedy loop at each depth on the library LMRS_LIB names, over a binding of its own -> one line of numbers on stdout"""
    path = os.environ.get("LMRS_LIB", os.path.join(ROOT, "lm.rs_amd", "liblmrs_hip.so"))
    lib = C.CDLL(path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.lmrs_last_error.restype = C.c_char_p
    lib.lmrs_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.lmrs_batch_create_wide.argtypes = [vp, u32, C.POINTER(vp)]
    lib.lmrs_batch_prefill.argtypes = [vp, u32, vp, sz, u32]
    lib.lmrs_batch_generate_greedy.argtypes = [vp, u32, vp, vp, vp, u32, vp, C.POINTER(C.c_double)]
    lib.lmrs_batch_destroy.argtypes = [vp]; lib.lmrs_batch_destroy.restype = None
    lib.lmrs_destroy.argtypes = [vp]; lib.lmrs_destroy.restype = None

    def chk(rc):
        if rc:
            raise RuntimeError(lib.lmrs_last_error().decode())

    img = np.fromfile(image_path, np.uint8)
    V = int(sys.argv[3])
    h, used, b = vp(), sz(), vp()
    chk(lib.lmrs_create(img.ctypes.data, img.size, 0, C.byref(h), C.byref(used)))
    chk(lib.lmrs_batch_create_wide(h, ROWS, C.byref(b)))
    out = []
    for depth in DEPTHS:
        prompts = prompts_of(V, depth)
        for i, p in enumerate(prompts):
            t = np.ascontiguousarray(p[:depth], np.uint32)
            chk(lib.lmrs_batch_prefill(b, i, t.ctypes.data, t.size, 0))
        slot = np.arange(ROWS, dtype=np.uint32); pos = np.full(ROWS, depth, np.uint32)
        tok = np.array([int(p[depth]) for p in prompts], np.uint32); ids = np.zeros((ROWS, GREEDY_STEPS), np.uint32); sec = C.c_double()
        us = []
        for k in range(7):
            chk(lib.lmrs_batch_generate_greedy(b, ROWS, slot.ctypes.data, tok.ctypes.data, pos.ctypes.data, GREEDY_STEPS, ids.ctypes.data, C.byref(sec)))
            if k >= 2:
                us.append(sec.value * 1e6 / GREEDY_STEPS)
        out += [*med(us), int(ids.astype(np.uint64).sum())]
    lib.lmrs_batch_destroy(b); lib.lmrs_destroy(h)
    print("UNUSED " + " ".join(f"{x:.2f}" if isinstance(x, float) else str(x) for x in out), flush=True)


def traced_passes(image_path):
    """measurement 3's child (under rocprofv3): 8 penalised greedy steps of 64 rows at each depth"""
    import lmrs_amd
    img = np.fromfile(image_path, np.uint8)
    m = lmrs_amd.Transformer(img)
    b = lmrs_amd.Batch(m, ROWS, wide=True)
    b.set_penalties(list(range(ROWS)), **ALL)
    for depth in DEPTHS + (DEEP,):
        prompts = prompts_of(m.args.vocab_size, depth)
        for i, p in enumerate(prompts):
            b.prefill(i, p[:depth], 0)
        b.generate_greedy(list(range(ROWS)), [int(p[depth]) for p in prompts], [depth] * ROWS, 1)
    b.close(); m.close()


def host_penalised(row, hist, par):
    """the rule over a record (positions 0 .. p, no NONE among them here), vectorised: np.float32 arrays, one operation at a time"""
    h = np.asarray(hist, np.int64)
    t_all = np.unique(h)
    t_out, c_out = np.unique(h[par["out_from"]:], return_counts=True)
    rep, pres, freq = np.float32(par["repetition"]), np.float32(par["presence"]), np.float32(par["frequency"])
    l = row[t_all]
    row[t_all] = np.where(l > 0, l / rep, l * rep)
    row[t_out] = (row[t_out] - freq * c_out.astype(np.float32)) - pres
    return row


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--unused-passes":
        return unused_passes(argv[1])
    if argv and argv[0] == "--traced-passes":
        return traced_passes(argv[1])
    parent = os.environ.get("PENALTY_RATE_PARENT_LIB")
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
    slots = list(range(ROWS))
    say(f"python tools/penalty_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234), vocabulary {V}; kernel_source_hash {bench.kernel_source_hash()}")
    say(f"a wide batch, {ROWS} rows, every row's record drawn from {ALPHABET} tokens; penalties: {ALL}")
    with tempfile.NamedTemporaryFile(suffix=".lmrs") as f:
        img.tofile(f.name)
        say(f"1. unused: lmrs_batch_generate_greedy, {ROWS} rows, device time of {GREEDY_STEPS} steps a call, median of 5 after 2 warm-ups (min .. max), the parent commit's library and "
            "this one by turns, a process per library and turn")
        if not parent or not os.path.exists(parent):
            say("    not run: no parent library given (--parent-lib PATH)")
        else:
            res = {"parent": [], "this": []}
            for turn in range(2):
                for who, path in (("parent", os.path.abspath(parent)), ("this", lmrs_amd.LIB_PATH)):
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--unused-passes", f.name, str(V)], env=dict(os.environ, LMRS_LIB=path),
                                       capture_output=True, text=True, timeout=900)
                    got = [l for l in r.stdout.splitlines() if l.startswith("UNUSED ")]
                    if r.returncode or not got:
                        say(f"    {who}, turn {turn}: failed: {r.stderr.strip()[-300:]}")
                        continue
                    v = got[0].split()[1:]
                    res[who].append(v)
                    say(f"    turn {turn}  {who:6s}  " + "   ".join(f"{d} positions {float(v[4 * k]):8.2f} us per step ({v[4 * k + 1]} .. {v[4 * k + 2]})" for k, d in enumerate(DEPTHS))
                        + f"   token checksums {v[3]} {v[7]}")
            if res["parent"] and res["this"]:
                for k, d in enumerate(DEPTHS):
                    p = [float(v[4 * k]) for v in res["parent"]]; t = [float(v[4 * k]) for v in res["this"]]
                    spread = max(max(float(v[4 * k + 2]) - float(v[4 * k + 1]) for v in res["parent"]), max(p) - min(p))
                    say(f"    {d} positions: parent {statistics.mean(p):.2f}, this {statistics.mean(t):.2f} us per step ({(statistics.mean(t) / statistics.mean(p) - 1) * 100:+.3f} %); "
                        f"the parent's own run-to-run spread {spread:.2f} us ({spread / statistics.mean(p) * 100:.3f} %); within it: "
                        f"{abs(statistics.mean(t) - statistics.mean(p)) <= spread}; same tokens: {res['parent'][0][4 * k + 3] == res['this'][0][4 * k + 3]}")
        say("3. the two launches alone: rocprofv3 --kernel-trace --stats over a process of its own, one penalised 64-row step at each depth")
        if not shutil.which("rocprofv3"):
            say("    not run: rocprofv3 is not on the PATH")
        else:
            with tempfile.TemporaryDirectory() as td:
                r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--traced-passes", f.name],
                                   capture_output=True, text=True, timeout=900)
                traces = glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True)
                if r.returncode or not traces:
                    say(f"    failed: {r.stderr.strip()[-300:]}")
                else:
                    rows = list(csv.DictReader(open(traces[0])))
                    for kern in ("penalty_rows_kernel", "record_rows_kernel"):
                        us = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in rows if kern in x["Kernel_Name"]]
                        say(f"    {kern}: {len(us)} launches, in order (prefills' record launches apart, the steps' at {', '.join(map(str, DEPTHS + (DEEP,)))} positions): "
                            + " ".join(f"{u:.2f}" for u in us[-3:]) + " us" + (f"   (all: min {min(us):.2f}, max {max(us):.2f} us)" if us else ""))
    m = lmrs_amd.Transformer(img)
    say(f"2. used: device time per step of lmrs_batch_generate_greedy, {ROWS} rows, {GREEDY_STEPS} steps a call; a batch with no record, one with the record alone and one with all rows "
        "penalised, by turns, median of 5 turns after 2 warm-ups (min .. max)")
    for depth in DEPTHS:
        prompts = prompts_of(V, depth)
        first = [int(p[depth]) for p in prompts]
        # two batches (64 caches of Gemma-2-2B are 112 GB): one that never has a record, one whose penalties are cleared and set turn by turn
        plain, rec = lmrs_amd.Batch(m, ROWS, wide=True), lmrs_amd.Batch(m, ROWS, wide=True)
        bs = {"no record": plain, "record": rec, "penalised": rec}
        rec.set_history(0)
        for b in (plain, rec):
            for i, p in enumerate(prompts):
                b.prefill(i, p[:depth], 0)
        per, ids = {k: [] for k in bs}, {}
        for k in range(7):
            for what, b in bs.items():
                if b is rec:
                    rec.set_penalties(slots, **ALL) if what == "penalised" else rec.clear_penalties()
                ids[what], sec = b.generate_greedy(slots, first, [depth] * ROWS, GREEDY_STEPS, timing=True)
                if k >= 2:
                    per[what].append(sec * 1e6 / GREEDY_STEPS)
        base, blo, bhi = med(per["no record"])
        say(f"  {depth} positions")
        say(f"    no record    {base:9.2f} us per step ({blo:.2f} .. {bhi:.2f})   {ROWS * 1e6 / base:9.0f} tok/s")
        n_keys = depth + GREEDY_STEPS // 2                                              # the mean record length over the loop
        for what, ref, nbytes, name in (("record", "no record", ROWS * 16, "the record in the loop"), ("penalised", "record", ROWS * (n_keys * 4 + ALPHABET * 8), "the penalties in the loop")):
            us, lo, hi = med(per[what])
            d, dl, dh = med([x - y for x, y in zip(per[what], per[ref])])               # the turns' own differences
            model_us = LAUNCH_US + nbytes / HBM_BYTES_PER_US
            say(f"    {what:12s} {us:9.2f} us per step ({lo:.2f} .. {hi:.2f})   {ROWS * 1e6 / us:9.0f} tok/s   {name}: {d:+6.2f} us per step ({dl:+.2f} .. {dh:+.2f}), {d / base * 100:.2f} % of the "
                f"step   model: 2.4 us + {nbytes} bytes / 6.3 TB/s = {model_us:.2f} us   same tokens as the batch without a record: {np.array_equal(ids[what], ids['no record'])}")
        plain.close(); rec.close()
    say(f"4. against the host route, {DEPTHS[0]} positions: host wall time per step, call to return; {STEPS} steps a run, median of 5 runs after 2 warm-ups (min .. max)")
    depth = DEPTHS[0]
    prompts = prompts_of(V, depth)
    first = [int(p[depth]) for p in prompts]
    dev_b, host_b = lmrs_amd.Batch(m, ROWS, wide=True), lmrs_amd.Batch(m, ROWS, wide=True)
    dev_b.set_penalties(slots, **ALL)
    for b in (dev_b, host_b):
        for i, p in enumerate(prompts):
            b.prefill(i, p[:depth], 0)

    def run(step):
        toks, ids, t = list(first), [], 0.0
        hist = [p[:depth].tolist() for p in prompts]
        for j in range(STEPS):
            pos = [depth + j] * ROWS
            t0 = time.perf_counter()
            toks = step(toks, pos, hist)
            t += time.perf_counter() - t0
            ids.append(list(map(int, toks)))
        return ids, t / STEPS * 1e6

    def timed(make_step):
        runs = [run(make_step()) for _ in range(7)][2:]
        return (runs[-1][0],) + med([u for _, u in runs])

    def samplers(temp, top_p):
        return [lmrs_amd.Sampler(V, temp, top_p, 7 + i) for i in range(ROWS)]

    def device_route(b, temp, top_p):
        sm = samplers(temp, top_p)
        return lambda t, p, hist: b.forward_runs_sample([(i, p[i], [t[i]], sm[i]) for i in range(ROWS)])

    def host_route(temp, top_p):
        sm = samplers(temp, top_p)

        def step(t, p, hist):
            _, lg = host_b.forward_runs([(i, p[i], [t[i]], 1) for i in range(ROWS)], logits=True)
            nxt = []
            for i in range(ROWS):
                hist[i].append(int(t[i]))                                              # the caller keeps the record itself
                nxt.append(sm[i].sample(host_penalised(lg[i], hist[i], ALL)))
            return nxt
        return step

    for name, temp, top_p in KINDS:
        _, plain, plo, phi = timed(lambda: device_route(host_b, temp, top_p))
        ids_dev, dev, dlo, dhi = timed(lambda: device_route(dev_b, temp, top_p))
        ids_host, host, hlo, hhi = timed(lambda: host_route(temp, top_p))
        say(f"  {name}")
        say(f"    unpenalised  lmrs_batch_forward_runs_sample {plain:9.1f} us per step ({plo:.1f} .. {phi:.1f})")
        say(f"    penalised    lmrs_batch_forward_runs_sample {dev:9.1f} us per step ({dlo:.1f} .. {dhi:.1f})   {dev - plain:+8.1f} us on the unpenalised step"
            f"   logits to host + numpy penalties + host sampler {host:9.1f} ({hlo:.1f} .. {hhi:.1f})   {host / dev:6.2f}x   same tokens: {ids_dev == ids_host}")
    dev_b.close(); host_b.close(); m.close()
    name = OUT.get((model, qt))
    path = os.environ.get("PENALTY_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
