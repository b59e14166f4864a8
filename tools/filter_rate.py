"""What the per-slot candidate filters (lmrs_batch_set_filters: top_k and min_gap) cost on a full-size synthetic model, one process per model: a wide batch
of 64 slots at 100 positions.
  1. unchanged when unused: lmrs_batch_generate_greedy of 16 and 64 rows on a batch that never set a filter, the parent commit's library against this one by
     turns (--parent-lib PATH, or FILTER_RATE_PARENT_LIB; without it the section says so) - device time of 32 steps a call (HIP events inside the call),
     median of 5 calls after 2 warm-ups, a child process per library and turn over a binding of its own of old entry points; and the two libraries' launch
     lists of one 64-row call (rocprofv3 --kernel-trace, a child each), compared name by name;
  2. the launch alone: filter_rows_kernel over 64 rows of the model's vocabulary (lmrs_op_filter_rows, rows of normal logits; and rows of ONE value, where
     the select runs every round) under top_k = 40, min_gap alone, both, and top_k = 70 000 on the equal rows - from a rocprofv3 --kernel-trace run of its
     own (skipped where rocprofv3 is missing), beside the step time of section 1;
  3. against the route callers have today, top_k = 40: lmrs_batch_forward_runs_sample on filtered slots against lmrs_batch_forward_runs with logits, the rule
     in numpy per row and lmrs_sampler_sample per row on the host - for a sample_mult sampler (0.8, 1.0), a peaked top-p (0.02, 0.9) and a flat top-p
     (1.0, 0.9); host wall time per step, call to return, 8 steps a run, median of 5 runs after 2 warm-ups, the tokens of the two routes compared; and the
     flat top-p rows with and without the filter in lmrs_batch_forward_runs_sample and in lmrs_batch_generate_topp (16 steps a call).
  (4., the headline - python bench.py on both commits - is run by hand; DESIGN.md section 4.4.16 quotes it.)
usage: python tools/filter_rate.py [--parent-lib PATH] [model] [q8_0|q4_0]
       (writes profiles/batch_filter_llama1b.txt for llama-3.2-1b q8_0, profiles/batch_filter_gemma2b_q4.txt for gemma-2-2b q4_0; FILTER_RATE_OUT names
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402

STEPS, ROWS, GREEDY_STEPS, LOOP_STEPS, DEPTH, TOP_K = 8, 64, 32, 16, 100, 40
WIDTHS = (16, 64)
OUT = {("llama-3.2-1b", S.Q8_0): "batch_filter_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_filter_gemma2b_q4.txt"}
KINDS = [("sample_mult (0.8, 1.0)", 0.8, 1.0), ("peaked top-p (0.02, 0.9)", 0.02, 0.9), ("flat top-p (1.0, 0.9)", 1.0, 0.9)]
FORMS = [("top_k = 40", 40, np.inf, False), ("min_gap = 2.0", 0, 2.0, False), ("top_k = 40 and min_gap = 2.0", 40, 2.0, False),
         ("top_k = 40, rows of one value", 40, np.inf, True), ("top_k = 70000, rows of one value", 70000, np.inf, True)]


def med(us):
    return statistics.median(us), min(us), max(us)


def prompts_of(V):
    rng = np.random.default_rng(21)
    return [rng.integers(0, V, DEPTH + 1).astype(np.uint32) for _ in range(ROWS)]


def unused_passes(image_path):
    """measurement 1's child: the greedy loop at 16 and 64 rows on the library LMRS_LIB names, over a binding of its own -> one line of numbers on stdout.
    FILTER_RATE_ONE_CALL: one 64-row call of 2 steps only (the launch lists' child)"""
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
    one = bool(os.environ.get("FILTER_RATE_ONE_CALL"))
    h, used, b = vp(), sz(), vp()
    chk(lib.lmrs_create(img.ctypes.data, img.size, 0, C.byref(h), C.byref(used)))
    chk(lib.lmrs_batch_create_wide(h, ROWS, C.byref(b)))
    prompts = prompts_of(V)
    for i, p in enumerate(prompts):
        t = np.ascontiguousarray(p[:DEPTH], np.uint32)
        chk(lib.lmrs_batch_prefill(b, i, t.ctypes.data, t.size, 0))
    out = []
    for n in ((ROWS,) if one else WIDTHS):
        slot = np.arange(n, dtype=np.uint32); pos = np.full(n, DEPTH, np.uint32)
        steps = 2 if one else GREEDY_STEPS
        tok = np.array([int(p[DEPTH]) for p in prompts[:n]], np.uint32); ids = np.zeros((n, steps), np.uint32); sec = C.c_double()
        us = []
        for k in range(1 if one else 7):
            chk(lib.lmrs_batch_generate_greedy(b, n, slot.ctypes.data, tok.ctypes.data, pos.ctypes.data, steps, ids.ctypes.data, C.byref(sec)))
            if k >= 2 or one:
                us.append(sec.value * 1e6 / steps)
        out += [*med(us), int(ids.astype(np.uint64).sum())]
    lib.lmrs_batch_destroy(b); lib.lmrs_destroy(h)
    print("UNUSED " + " ".join(f"{x:.2f}" if isinstance(x, float) else str(x) for x in out), flush=True)


def traced_launches(V):
    """measurement 2's child (under rocprofv3): the kernel alone, each form three times"""
    import lmrs_amd
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((ROWS, V)) * 3).astype(np.float32)
    flat = np.full((ROWS, V), np.float32(1.25))
    for _, k, gap, ties in FORMS:
        for _ in range(3):
            lmrs_amd.filter_rows(flat if ties else rows, k, gap)


def kernel_trace(cmd, env=None):
    """-> the rows of rocprofv3's kernel trace of `cmd`, in start order (None: it failed)"""
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", td, "--"] + cmd, capture_output=True, text=True, timeout=900, env=env)
        traces = glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode or not traces:
            return None, r.stderr.strip()[-300:]
        rows = list(csv.DictReader(open(traces[0])))
        rows.sort(key=lambda x: int(x["Start_Timestamp"]))
        return rows, ""


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--unused-passes":
        return unused_passes(argv[1])
    if argv and argv[0] == "--traced-launches":
        return traced_launches(int(argv[1]))
    parent = os.environ.get("FILTER_RATE_PARENT_LIB")
    if argv and argv[0] == "--parent-lib":
        parent, argv = argv[1], argv[2:]
    model = argv[0] if argv else "llama-3.2-1b"
    qname = argv[1] if len(argv) > 1 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    import bench
    import lmrs_amd
    from filter_rules import filtered
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    V = S.CONFIGS[model].vocab_size
    slots = list(range(ROWS))
    me = os.path.abspath(__file__)
    say(f"python tools/filter_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234), vocabulary {V}; kernel_source_hash {bench.kernel_source_hash()}")
    say(f"a wide batch, {ROWS} rows at {DEPTH} positions")
    step_us = {}
    with tempfile.NamedTemporaryFile(suffix=".lmrs") as f:
        img.tofile(f.name)
        say(f"1. unused: lmrs_batch_generate_greedy, device time of {GREEDY_STEPS} steps a call, median of 5 after 2 warm-ups (min .. max), the parent commit's library and this one "
            "by turns, a process per library and turn")
        if not parent or not os.path.exists(parent):
            say("    not run: no parent library given (--parent-lib PATH)")
        else:
            libs = (("parent", os.path.abspath(parent)), ("this", lmrs_amd.LIB_PATH))
            res = {"parent": [], "this": []}
            for turn in range(2):
                for who, path in libs:
                    r = subprocess.run([sys.executable, me, "--unused-passes", f.name, str(V)], env=dict(os.environ, LMRS_LIB=path), capture_output=True, text=True, timeout=900)
                    got = [l for l in r.stdout.splitlines() if l.startswith("UNUSED ")]
                    if r.returncode or not got:
                        say(f"    {who}, turn {turn}: failed: {r.stderr.strip()[-300:]}")
                        continue
                    v = got[0].split()[1:]
                    res[who].append(v)
                    say(f"    turn {turn}  {who:6s}  " + "   ".join(f"{n} rows {float(v[4 * k]):8.2f} us per step ({v[4 * k + 1]} .. {v[4 * k + 2]})" for k, n in enumerate(WIDTHS))
                        + f"   token checksums {v[3]} {v[7]}")
            if res["parent"] and res["this"]:
                for k, n in enumerate(WIDTHS):
                    p = [float(v[4 * k]) for v in res["parent"]]; t = [float(v[4 * k]) for v in res["this"]]
                    step_us[n] = statistics.mean(t)
                    spread = max(max(float(v[4 * k + 2]) - float(v[4 * k + 1]) for v in res["parent"]), max(p) - min(p))
                    inside = abs(statistics.mean(t) - statistics.mean(p)) <= spread
                    say(f"    {n} rows: parent {statistics.mean(p):.2f}, this {statistics.mean(t):.2f} us per step ({(statistics.mean(t) / statistics.mean(p) - 1) * 100:+.3f} %); "
                        f"the parent's own spread across its calls and turns {spread:.2f} us ({spread / statistics.mean(p) * 100:.3f} %); within it: {inside}"
                        f"{'' if inside else '  ** A MISS **'}; same tokens: {res['parent'][0][4 * k + 3] == res['this'][0][4 * k + 3]}")
            if not shutil.which("rocprofv3"):
                say("    launch lists: not compared: rocprofv3 is not on the PATH")
            else:
                names = {}
                for who, path in libs:
                    rows, err = kernel_trace([sys.executable, me, "--unused-passes", f.name, str(V)], env=dict(os.environ, LMRS_LIB=path, FILTER_RATE_ONE_CALL="1"))
                    names[who] = None if rows is None else [x["Kernel_Name"] for x in rows]
                    if rows is None:
                        say(f"    launch lists: {who}: failed: {err}")
                if names.get("parent") and names.get("this"):
                    say(f"    launch lists of a process that prefills {ROWS} slots and runs one {ROWS}-row call of 2 steps: parent {len(names['parent'])} launches, this {len(names['this'])}; "
                        f"identical, name by name: {names['parent'] == names['this']}; filter_rows_kernel among them: {any('filter_rows' in x for x in names['this'])}")
    say(f"2. the launch alone: filter_rows_kernel over {ROWS} rows of {V} logits (lmrs_op_filter_rows), rocprofv3 --kernel-trace over a process of its own, three launches a form")
    if not shutil.which("rocprofv3"):
        say("    not run: rocprofv3 is not on the PATH")
    else:
        rows, err = kernel_trace([sys.executable, me, "--traced-launches", str(V)])
        if rows is None:
            say(f"    failed: {err}")
        else:
            us = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in rows if "filter_rows_kernel" in x["Kernel_Name"]]
            for i, (name, _, _, _) in enumerate(FORMS):
                mine = us[3 * i:3 * i + 3]
                if len(mine) == 3:
                    share = f"   {min(mine) / step_us[ROWS] * 100:.2f} % of the {ROWS}-row step of section 1" if ROWS in step_us else ""
                    say(f"    {name:36s} {' '.join(f'{u:8.2f}' for u in mine)} us{share}")
    m = lmrs_amd.Transformer(img)
    prompts = prompts_of(V)
    first = [int(p[DEPTH]) for p in prompts]
    dev_b, host_b = lmrs_amd.Batch(m, ROWS, wide=True), lmrs_amd.Batch(m, ROWS, wide=True)
    dev_b.set_filters(slots, top_k=TOP_K)
    for b in (dev_b, host_b):
        for i, p in enumerate(prompts):
            b.prefill(i, p[:DEPTH], 0)
    say(f"3. against the host route, top_k = {TOP_K}: host wall time per step, call to return; {STEPS} steps a run, median of 5 runs after 2 warm-ups (min .. max)")

    def run(step):
        toks, ids, t = list(first), [], 0.0
        for j in range(STEPS):
            pos = [DEPTH + j] * ROWS
            t0 = time.perf_counter()
            toks = step(toks, pos)
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
        return lambda t, p: b.forward_runs_sample([(i, p[i], [t[i]], sm[i]) for i in range(ROWS)])

    def host_route(temp, top_p):
        sm = samplers(temp, top_p)

        def step(t, p):
            _, lg = host_b.forward_runs([(i, p[i], [t[i]], 1) for i in range(ROWS)], logits=True)
            return [sm[i].sample(filtered(lg[i], TOP_K)) for i in range(ROWS)]
        return step

    for name, temp, top_p in KINDS:
        _, plain, plo, phi = timed(lambda: device_route(host_b, temp, top_p))
        ids_dev, dev, dlo, dhi = timed(lambda: device_route(dev_b, temp, top_p))
        ids_host, host, hlo, hhi = timed(lambda: host_route(temp, top_p))
        say(f"  {name}")
        say(f"    unfiltered  lmrs_batch_forward_runs_sample {plain:9.1f} us per step ({plo:.1f} .. {phi:.1f})")
        say(f"    top_k = {TOP_K}  lmrs_batch_forward_runs_sample {dev:9.1f} us per step ({dlo:.1f} .. {dhi:.1f})   {dev - plain:+8.1f} us on the unfiltered step"
            f"   logits to host + numpy filter + host sampler {host:9.1f} ({hlo:.1f} .. {hhi:.1f})   {host / dev:6.2f}x   same tokens: {ids_dev == ids_host}")
    say(f"  flat top-p (1.0, 0.9) in lmrs_batch_generate_topp: {ROWS} rows, {LOOP_STEPS} steps a call, check_every {LOOP_STEPS}; host wall time per step, median of 5 calls after 2 warm-ups")
    for what, b in (("unfiltered", host_b), (f"top_k = {TOP_K}", dev_b)):
        us = []
        for k in range(7):
            sm = samplers(1.0, 0.9)
            t0 = time.perf_counter()
            b.generate_topp(slots, first, [DEPTH] * ROWS, [LOOP_STEPS] * ROWS, samplers=sm, check_every=LOOP_STEPS)
            if k >= 2:
                us.append((time.perf_counter() - t0) * 1e6 / LOOP_STEPS)
        u, lo, hi = med(us)
        say(f"    {what:12s} {u:9.1f} us per step ({lo:.1f} .. {hi:.1f})   {ROWS * 1e6 / u:9.0f} tok/s")
    dev_b.close(); host_b.close(); m.close()
    name = OUT.get((model, qt))
    path = os.environ.get("FILTER_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
