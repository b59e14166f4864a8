"""What allowed-token masks (lmrs_batch_set_masks) cost on a full-size synthetic model, one process per model: a wide batch of 64 slots, rows at 100 positions.
  1. a 64-row lmrs_batch_forward_runs_sample step with EVERY row masked - a ban-list of 100 tokens, then an allow-list of 100 tokens, a list of its own
     per row - against the same step unmasked, for a sample_mult sampler (0.8, 1.0), a peaked top-p (0.02, 0.9) and the default flags' top-p (0.7, 0.9);
  2. the same masked step through the only route the library had: lmrs_batch_forward_runs with logits, the mask applied in numpy (an index assignment per
     row), lmrs_sampler_sample per row on the host - same session, same samplers' seeds, the tokens of the two routes compared;
     (1 and 2: host wall time per step, call to return, 8 steps a run, every row fed its own token, median of 5 runs after 2 warm-ups, min .. max)
  3. the mask launch's own device time per slab: lmrs_batch_generate_greedy of 64 rows reports the device time of its steps (HIP events inside the call); the
     unmasked run, the ban-lists and the allow-lists by turns, 32 steps a call, median of 5 turns after 2 warm-ups; the difference per step is the launch (64
     rows are one slab of the logits block), beside DESIGN.md section 3.5's launch model - 2.4 us + bytes written / 6.3 TB/s;
  4. unmasked passes, the parent commit's library against this one by turns (--parent-lib PATH, or MASK_RATE_PARENT_LIB; without it the section says so):
     lmrs_batch_generate_greedy at n = 16 and n = 64 on a wide batch, tools/batch_rate.py --wide's two lines - device time of 64 steps a call, median of 5
     after 2 warm-ups - a child process per library and turn, over a binding of its own of five old entry points, so it runs on either library.
usage: python tools/mask_rate.py [--parent-lib PATH] [model] [q8_0|q4_0]
       (writes profiles/batch_mask_llama1b.txt for llama-3.2-1b q8_0, profiles/batch_mask_gemma2b_q4.txt for gemma-2-2b q4_0; MASK_RATE_OUT names another file)"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402

STEPS, ROWS, DEPTH, LIST, GREEDY_STEPS, AB_STEPS = 8, 64, 100, 100, 32, 64
OUT = {("llama-3.2-1b", S.Q8_0): "batch_mask_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_mask_gemma2b_q4.txt"}
KINDS = [("sample_mult (0.8, 1.0)", 0.8, 1.0), ("peaked top-p (0.02, 0.9)", 0.02, 0.9), ("flat top-p (0.7, 0.9)", 0.7, 0.9)]
LAUNCH_US, HBM_BYTES_PER_US = 2.4, 6.3e6


def med(us):
    return statistics.median(us), min(us), max(us)


def unmasked_passes(image_path):
    """measurement 4's child: the two greedy lines on the library LMRS_LIB names, over a binding of its own -> one line of numbers on stdout"""
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
    model = sys.argv[3]
    h, used, b = vp(), sz(), vp()
    chk(lib.lmrs_create(img.ctypes.data, img.size, 0, C.byref(h), C.byref(used)))
    chk(lib.lmrs_batch_create_wide(h, ROWS, C.byref(b)))
    prompts = [S.prompt_tokens(model, DEPTH + 1, 100 + i) for i in range(ROWS)]
    for i, p in enumerate(prompts):
        t = np.ascontiguousarray(p[:DEPTH], np.uint32)
        chk(lib.lmrs_batch_prefill(b, i, t.ctypes.data, t.size, 0))
    out = []
    for n in (16, ROWS):
        slot = np.arange(n, dtype=np.uint32); pos = np.full(n, DEPTH, np.uint32)
        tok = np.array([int(p[DEPTH]) for p in prompts[:n]], np.uint32); ids = np.zeros((n, AB_STEPS), np.uint32); sec = C.c_double()
        us = []
        for k in range(7):
            chk(lib.lmrs_batch_generate_greedy(b, n, slot.ctypes.data, tok.ctypes.data, pos.ctypes.data, AB_STEPS, ids.ctypes.data, C.byref(sec)))
            if k >= 2:
                us.append(sec.value * 1e6 / AB_STEPS)
        out += [*med(us), int(ids.astype(np.uint64).sum())]
    lib.lmrs_batch_destroy(b); lib.lmrs_destroy(h)
    print("UNMASKED " + " ".join(f"{x:.2f}" if isinstance(x, float) else str(x) for x in out), flush=True)


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--unmasked-passes":
        return unmasked_passes(argv[1])
    parent = os.environ.get("MASK_RATE_PARENT_LIB")
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
    m = lmrs_amd.Transformer(img)
    b = lmrs_amd.Batch(m, ROWS, wide=True)
    V = m.args.vocab_size
    say(f"python tools/mask_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234), vocabulary {V}; kernel_source_hash {bench.kernel_source_hash()}")
    say(f"a wide batch, {ROWS} rows at {DEPTH} positions, every row masked with a list of its own ({LIST} tokens)")
    prompts = [S.prompt_tokens(model, DEPTH + 1, 100 + i) for i in range(ROWS)]
    for i, p in enumerate(prompts):
        b.prefill(i, p[:DEPTH], 0)
    first = [int(p[DEPTH]) for p in prompts]
    slots = list(range(ROWS))
    rng = np.random.default_rng(11)
    lists = [np.sort(rng.choice(V, LIST, replace=False)) for _ in range(ROWS)]
    ninf = np.float32(-np.inf)

    def bool_masks(allow):
        mk = np.zeros((ROWS, V), np.bool_) if allow else np.ones((ROWS, V), np.bool_)
        for i, idx in enumerate(lists):
            mk[i, idx] = allow
        return mk
    packed = {"ban-list": lmrs_amd.pack_mask(bool_masks(False)), "allow-list": lmrs_amd.pack_mask(bool_masks(True))}

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

    def device_route(temp, top_p):
        sm = samplers(temp, top_p)
        return lambda t, p: b.forward_runs_sample([(i, p[i], [t[i]], sm[i]) for i in range(ROWS)])

    def host_route(temp, top_p, allow):
        sm = samplers(temp, top_p)

        def step(t, p):
            _, lg = b.forward_runs([(i, p[i], [t[i]], 1) for i in range(ROWS)], logits=True)
            nxt = []
            for i in range(ROWS):
                if allow:
                    row = np.full(V, ninf, np.float32); row[lists[i]] = lg[i, lists[i]]
                else:
                    row = lg[i]; row[lists[i]] = ninf
                nxt.append(sm[i].sample(row))
            return nxt
        return step

    say("1, 2. host wall time per step, call to return; 8 steps a run, median of 5 runs after 2 warm-ups (min .. max)")
    beats, extra = [], {}
    for name, temp, top_p in KINDS:
        b.clear_masks()
        _, plain, plo, phi = timed(lambda: device_route(temp, top_p))
        say(f"  {name}")
        say(f"    unmasked     lmrs_batch_forward_runs_sample {plain:9.1f} us per step ({plo:.1f} .. {phi:.1f})")
        for what, allow in (("ban-list", False), ("allow-list", True)):
            b.set_masks(slots, packed[what])
            ids_dev, dev, dlo, dhi = timed(lambda: device_route(temp, top_p))
            b.clear_masks()
            ids_host, host, hlo, hhi = timed(lambda: host_route(temp, top_p, allow))
            beats.append((name, what, host / dev, host - dev > hhi - hlo))
            extra[(name, what)] = (dev - plain, max(dhi - dlo, phi - plo))
            say(f"    {what:12s} lmrs_batch_forward_runs_sample {dev:9.1f} us per step ({dlo:.1f} .. {dhi:.1f})   {dev - plain:+8.1f} us on the unmasked step"
                f"   logits to host + numpy mask + host sampler {host:9.1f} ({hlo:.1f} .. {hhi:.1f})   {host / dev:6.2f}x   same tokens: {ids_dev == ids_host}")
    say(f"3. the mask launch alone: device time per step of lmrs_batch_generate_greedy, {ROWS} rows, {GREEDY_STEPS} steps a call; unmasked, ban-lists and allow-lists by "
        "turns, median of 5 turns after 2 warm-ups (min .. max)")
    per = {"unmasked": [], "ban-list": [], "allow-list": []}
    ids = {}
    for k in range(7):
        for what in per:
            b.clear_masks() if what == "unmasked" else b.set_masks(slots, packed[what])
            ids[what], sec = b.generate_greedy(slots, first, [DEPTH] * ROWS, GREEDY_STEPS, timing=True)
            if k >= 2:
                per[what].append(sec * 1e6 / GREEDY_STEPS)
    b.clear_masks()
    base, blo, bhi = med(per["unmasked"])
    say(f"    unmasked     {base:9.2f} us per step ({blo:.2f} .. {bhi:.2f})")
    launch = {}
    for what, nbytes in (("ban-list", ROWS * LIST * 4), ("allow-list", ROWS * (V - LIST) * 4)):
        us, lo, hi = med(per[what])
        diffs = [x - y for x, y in zip(per[what], per["unmasked"])]                     # the turns' own differences
        d, dl, dh = med(diffs)
        model_us = LAUNCH_US + nbytes / HBM_BYTES_PER_US
        launch[what] = (d, model_us, max(hi - lo, bhi - blo))
        say(f"    {what:12s} {us:9.2f} us per step ({lo:.2f} .. {hi:.2f})   the launch: {d:+6.2f} us per slab ({dl:+.2f} .. {dh:+.2f})   model: 2.4 us + {nbytes} bytes / 6.3 TB/s"
            f" = {model_us:.2f} us   the masks changed the tokens: {not np.array_equal(ids[what], ids['unmasked'])}")
    say(f"4. unmasked passes, the parent commit's library and this one by turns: lmrs_batch_generate_greedy on a wide batch at {DEPTH} positions, device time of {AB_STEPS} steps a call, "
        "median of 5 after 2 warm-ups (min .. max), a process per library and turn")
    b.close(); m.close()
    if not parent or not os.path.exists(parent):
        say("    not run: no parent library given (--parent-lib PATH)")
    else:
        with tempfile.NamedTemporaryFile(suffix=".lmrs") as f:
            img.tofile(f.name)
            res = {"parent": [], "this": []}
            for turn in range(2):
                for who, path in (("parent", os.path.abspath(parent)), ("this", lmrs_amd.LIB_PATH)):
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--unmasked-passes", f.name, model], env=dict(os.environ, LMRS_LIB=path),
                                       capture_output=True, text=True, timeout=600)
                    got = [l for l in r.stdout.splitlines() if l.startswith("UNMASKED ")]
                    if r.returncode or not got:
                        say(f"    {who}, turn {turn}: failed: {r.stderr.strip()[-300:]}")
                        continue
                    v = got[0].split()[1:]
                    res[who].append(v)
                    say(f"    turn {turn}  {who:6s}  n=16 {float(v[0]):8.2f} us per pass ({v[1]} .. {v[2]})   n=64 {float(v[4]):8.2f} us per pass ({v[5]} .. {v[6]})   token checksums {v[3]} {v[7]}")
        if res["parent"] and res["this"]:
            for n, k in ((16, 0), (64, 4)):
                p = [float(v[k]) for v in res["parent"]]; t = [float(v[k]) for v in res["this"]]
                spread = max(max(float(v[k + 2]) - float(v[k + 1]) for v in res["parent"]), max(p) - min(p))
                say(f"    n={n}: parent {statistics.mean(p):.2f}, this {statistics.mean(t):.2f} us per pass; the parent's own run-to-run spread {spread:.2f} us; "
                    f"within it: {abs(statistics.mean(t) - statistics.mean(p)) <= spread}; same tokens: {res['parent'][0][k + 3] == res['this'][0][k + 3]}")
    say("conditions")
    for name, what, ratio, clear in beats:
        say(f"  {name}, {what}: the device route beats the host route by more than the host route's spread: {clear} ({ratio:.2f}x)")
    for what, (d, model_us, spread) in launch.items():
        say(f"  {what}: the launch costs {d:.2f} us against the model's {model_us:.2f} us; more than the model by more than the measured spread ({spread:.2f} us): {d - model_us > spread}")
    for (name, what), (d, spread) in extra.items():
        say(f"  {name}, {what}: the masked step costs {d:+.1f} us on the unmasked step against the model's {launch[what][1]:.1f} us (wall-time spread {spread:.1f} us): "
            f"above the model by more than the spread: {d - launch[what][1] > spread}")
    name = OUT.get((model, qt))
    path = os.environ.get("MASK_RATE_OUT") or (os.path.join(ROOT, "profiles", name) if name else None)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
