"""What embedding rows in a batch cost, in one process per model: host wall time of synchronous calls, median of 5 after 2 warm-ups with the minimum and
the maximum, the results of the two routes compared in the same run.
  (a) admitting one image of 320 embedding rows into a slot: lmrs_batch_prefill_embeddings with residual NULL, against the route the token-only batch
      API leaves - lmrs_fill_kv_cache on the context's own cache (which downloads the residual rows) + lmrs_batch_fork(LMRS_BATCH_CTX -> slot, 320);
  (b) a step of 15 decode rows at 100 positions with a 64-row image chunk beside them in ONE lmrs_batch_forward_runs_embed pass, against
      lmrs_fill_kv_cache(64) + lmrs_batch_fork + lmrs_batch_forward(15) as three calls;
  (c) lmrs_batch_forward_runs on a token-only pass of 16 and of 64 rows (16 runs on 16 slots at 100 positions, every output asked for): time of 64
      calls / 64.  This line goes through a binding of its own over five old entry points, so it runs on a library built before the embedding calls
      existed as well (LMRS_LIB names it): the two builds of an A/B run by turns.
The rows are random (normal * 0.5): the layers never look at where a row came from.  phi-3.5 is the full-size synthetic model with 2048 positions
(a slot's K/V cache is 1.6 GB then, 16 slots 26 GB).
usage: python tools/batch_embed_rate.py [phi-3.5|mini-phi-long]
       python tools/batch_embed_rate.py --token-passes [phi-3.5|mini-phi-long]        (line (c) only)
BATCH_EMBED_OUT names a file the lines are appended to (profiles/batch_embed_phi.txt holds both models and both builds of (c))."""
import ctypes as C
import dataclasses
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402

CALLS, DEPTH, IMAGE, CHUNK = 64, 100, 320, 64
lines = []


def say(s=""):
    print(s, flush=True); lines.append(s)


def timed(fn, reps=5, warm=2, before=lambda: None):
    """fn() -> result; before() runs untimed ahead of every call -> (the last result, median, min, max in microseconds of host wall time)"""
    us = []
    for i in range(warm + reps):
        before()
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e6
        if i >= warm:
            us.append(dt)
    return r, statistics.median(us), min(us), max(us)


def model_image(name):
    cfg = S.CONFIGS[name]
    if name == "phi-3.5":
        cfg = dataclasses.replace(cfg, max_pos=2048)
    return cfg, S.build_image(cfg, S.Q8_0, 1234)


def token_passes(cfg, img):
    """line (c), over a binding of its own"""
    path = os.environ.get("LMRS_LIB", os.path.join(ROOT, "lm.rs_amd", "liblmrs_hip.so"))
    lib = C.CDLL(path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.lmrs_last_error.restype = C.c_char_p
    lib.lmrs_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.lmrs_batch_create.argtypes = [vp, u32, C.POINTER(vp)]
    lib.lmrs_batch_prefill.argtypes = [vp, u32, vp, sz, u32]
    lib.lmrs_batch_forward_runs.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
    lib.lmrs_batch_destroy.argtypes = [vp]; lib.lmrs_batch_destroy.restype = None
    lib.lmrs_destroy.argtypes = [vp]; lib.lmrs_destroy.restype = None

    def chk(rc):
        if rc:
            raise RuntimeError(lib.lmrs_last_error().decode())

    h, used, b = vp(), sz(), vp()
    chk(lib.lmrs_create(img.ctypes.data, img.size, 0, C.byref(h), C.byref(used)))
    chk(lib.lmrs_batch_create(h, 16, C.byref(b)))
    prompts = [S.prompt_tokens(cfg, DEPTH + 8, 100 + i) for i in range(16)]
    for i, p in enumerate(prompts):
        t = np.ascontiguousarray(p[:DEPTH], np.uint32)
        chk(lib.lmrs_batch_prefill(b, i, t.ctypes.data, t.size, 0))
    say(f"(c) lmrs_batch_forward_runs, token runs only: R rows as 16 runs on 16 slots at {DEPTH} positions, every output asked for; {CALLS} synchronous calls / {CALLS}"
        f"   [library: {os.path.basename(path)}]")
    for R in (16, 64):
        n = R // 16
        slot = np.arange(16, dtype=np.uint32); start = np.full(16, DEPTH, np.uint32); ln = np.full(16, n, np.uint32); no = ln.copy()
        tok = np.ascontiguousarray(np.concatenate([p[DEPTH:DEPTH + n] for p in prompts]), np.uint32)
        am = np.zeros(R, np.uint32)

        def calls():
            for _ in range(CALLS):
                chk(lib.lmrs_batch_forward_runs(b, 16, slot.ctypes.data, start.ctypes.data, ln.ctypes.data, no.ctypes.data, tok.ctypes.data, am.ctypes.data,
                                                None, 0, None, None))
            return am
        am, us, lo, hi = timed(calls)
        say(f"  R={R:2d}   {us / CALLS:8.1f} us per pass ({lo / CALLS:.1f} .. {hi / CALLS:.1f})   argmax checksum {int(am.astype(np.uint64).sum())}")
    lib.lmrs_batch_destroy(b); lib.lmrs_destroy(h)


def main():
    argv = sys.argv[1:]
    only_c = bool(argv) and argv[0] == "--token-passes"
    name = (argv[1:] if only_c else argv) or ["phi-3.5"]
    cfg, img = model_image(name[0])
    say(f"python tools/batch_embed_rate.py {' '.join(argv)}")
    say(f"{cfg.name} Q8_0, {cfg.max_pos} positions, synthetic weights (tools/synth_lmrs.py seed 1234); host wall time, median of 5 after 2 warm-ups (min .. max)")
    if not only_c:
        import lmrs_amd
        m = lmrs_amd.Transformer(img)
        b = lmrs_amd.Batch(m, 16)
        dim, nl = m.args.dim, m.args.n_layers
        rng = np.random.default_rng(7)
        image = np.ascontiguousarray(rng.standard_normal((IMAGE, dim)).astype(np.float32) * np.float32(0.5))

        def rows_equal(x, y, positions):
            return all((b.kv_row(x, w, l, p).view(np.uint32) == b.kv_row(y, w, l, p).view(np.uint32)).all() for w in (0, 1) for l in (0, nl - 1) for p in positions)

        # (a)
        _, new, lo, hi = timed(lambda: b.prefill_embeddings(0, image, 0))
        scratch = [None]

        def old_a():
            m.fill_kv_cache(scratch[0], 0); b.fork(lmrs_amd.BATCH_CTX, 1, IMAGE)
        _, old, lo2, hi2 = timed(old_a, before=lambda: scratch.__setitem__(0, image.reshape(-1).copy()))
        am = b.forward([0, 1], [5, 5], [IMAGE, IMAGE])
        same = rows_equal(0, 1, (0, IMAGE // 2, IMAGE - 1)) and int(am[0]) == int(am[1])
        say(f"(a) one image of {IMAGE} embedding rows into a slot")
        say(f"  lmrs_batch_prefill_embeddings (residual NULL)              {new / 1e3:8.3f} ms ({lo / 1e3:.3f} .. {hi / 1e3:.3f})")
        say(f"  lmrs_fill_kv_cache + lmrs_batch_fork(LMRS_BATCH_CTX -> slot) {old / 1e3:8.3f} ms ({lo2 / 1e3:.3f} .. {hi2 / 1e3:.3f})   "
            f"{old / new:5.2f}x; K/V rows bit-equal and the same next token: {same}")
        # (b): slots 0 .. 14 at DEPTH positions, the chunk on slot 15 from position 0
        prompts = [S.prompt_tokens(cfg, DEPTH + 1, 100 + i) for i in range(15)]
        for i, p in enumerate(prompts):
            b.prefill(i, p[:DEPTH], 0)
        chunk = np.ascontiguousarray(image[:CHUNK])
        runs = [(i, DEPTH, [int(p[DEPTH])], 1) for i, p in enumerate(prompts)] + [(15, 0, chunk, 0)]
        am_new, new, lo, hi = timed(lambda: b.forward_runs(runs))
        keep = [b.kv_row(15, w, nl - 1, CHUNK - 1).copy() for w in (0, 1)]

        def old_b():
            m.fill_kv_cache(scratch[0], 0); b.fork(lmrs_amd.BATCH_CTX, 15, CHUNK)
            return b.forward(list(range(15)), [int(p[DEPTH]) for p in prompts], [DEPTH] * 15)
        am_old, old, lo2, hi2 = timed(old_b, before=lambda: scratch.__setitem__(0, chunk.reshape(-1).copy()))
        same = am_new.tolist() == am_old.tolist() and all((b.kv_row(15, w, nl - 1, CHUNK - 1).view(np.uint32) == keep[w].view(np.uint32)).all() for w in (0, 1))
        say(f"(b) 15 decode rows at {DEPTH} positions and a {CHUNK}-row image chunk")
        say(f"  ONE lmrs_batch_forward_runs_embed pass                                  {new / 1e3:8.3f} ms ({lo / 1e3:.3f} .. {hi / 1e3:.3f})")
        say(f"  lmrs_fill_kv_cache({CHUNK}) + lmrs_batch_fork + lmrs_batch_forward(15): three calls {old / 1e3:8.3f} ms ({lo2 / 1e3:.3f} .. {hi2 / 1e3:.3f})   "
            f"{old / new:5.2f}x; the 15 tokens equal and the chunk's last K/V row bit-equal: {same}")
        b.close(); m.close()
    token_passes(cfg, img)
    say()
    path = os.environ.get("BATCH_EMBED_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
