"""What a short token pass costs on a full-size synthetic model, in one process: lmrs_verify_tokens (the skinny weight-streaming GEMMs) at n = 2, 4, 8, 16
against lmrs_score_tokens at the same n (the batched pass on the direct MFMA kernels: the baseline, unchanged by the skinny form) and against one decode
step (lmrs_forward_argmax), then lmrs_generate_speculative against lmrs_generate_greedy for 256 new tokens on two prompts, with the acceptance counts.
Every call is synchronous (it ends with the context's stream idle), so a HIP event recorded on the null stream before and after it brackets the call's
device work and its host round trip: median of 30 calls after 5 warm-ups, with the minimum and the maximum.  The decode step is also given as
lmrs_generate_greedy's device time per step (steps back to back, no host round trip between them).
usage: python tools/verify_rate.py [model] [q8_0|q4_0]        (writes profiles/verify_rate_<model>.txt when run for llama-3.2-1b q8_0)"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import bench  # noqa: E402
import lmrs_amd  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402

hip = ctypes.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]


def _ok(rc):
    if rc:
        raise RuntimeError(f"HIP error {rc}")


E0, E1 = ctypes.c_void_p(), ctypes.c_void_p()


def timed(fn, reps=30, warm=5):
    """-> (median, min, max) in microseconds"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        _ok(hip.hipEventRecord(E0, None)); fn(); _ok(hip.hipEventRecord(E1, None)); _ok(hip.hipEventSynchronize(E1))
        ms = ctypes.c_float(); _ok(hip.hipEventElapsedTime(ctypes.byref(ms), E0, E1)); out.append(ms.value * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "llama-3.2-1b"
    qname = sys.argv[2] if len(sys.argv) > 2 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    _ok(hip.hipEventCreate(ctypes.byref(E0))); _ok(hip.hipEventCreate(ctypes.byref(E1)))
    say(f"python tools/verify_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}")
    say("HIP events on the null stream around each synchronous call; us: median of 30 after 5 warm-ups (min .. max)")
    start = 64
    m.prefill_tokens(S.prompt_tokens(model, start, 3), 0)
    toks = S.prompt_tokens(model, 16, 7)
    step = timed(lambda: m.forward_argmax(int(toks[0]), start))
    say(f"  one decode step (lmrs_forward_argmax at position {start}, host round trip included): {step[0]:8.1f} us ({step[1]:.1f} .. {step[2]:.1f})")
    pr = S.prompt_tokens(model, 16, 9)
    _, sec = m.generate_greedy(pr, 256, 0, timing=True)
    _, sec = m.generate_greedy(pr, 256, 0, timing=True)
    in_loop = sec / (16 + 255) * 1e6
    say(f"  one decode step inside lmrs_generate_greedy (16 + 255 steps, device time / steps):   {in_loop:8.1f} us")
    m.prefill_tokens(S.prompt_tokens(model, start, 3), 0)
    for n in (2, 4, 8, 16):
        v = timed(lambda: m.verify_tokens(toks[:n], start))
        s = timed(lambda: m.score(toks[:n], start))
        same = m.verify_tokens(toks[:n], start)[0].tolist() == m.score(toks[:n], start)[1].tolist()
        say(f"  n={n:2d}  verify_tokens {v[0]:8.1f} us ({v[1]:.1f} .. {v[2]:.1f})   score_tokens {s[0]:8.1f} us ({s[1]:.1f} .. {s[2]:.1f})   "
            f"score / verify {s[0] / v[0]:5.2f}x   verify = {v[0] / step[0]:5.2f} synchronous steps = {v[0] / in_loop:5.2f} in-loop steps   same argmax: {same}")
    say("generate, 256 new tokens (HIP events around the whole call, median of 5 after 1 warm-up); max_draft 7, ngram_max 3")
    block = S.prompt_tokens(model, 8, 11)
    for name, prompt in (("8-token block x 8", np.tile(block, 8).astype(np.uint32)), ("64 random tokens", S.prompt_tokens(model, 64, 13))):
        want = m.generate_greedy(prompt, 256)
        got, st = m.generate_speculative(prompt, 256)
        g = timed(lambda: m.generate_greedy(prompt, 256), reps=5, warm=1)
        sp = timed(lambda: m.generate_speculative(prompt, 256), reps=5, warm=1)
        distinct = len(set(want.tolist()))
        say(f"  prompt: {name}: greedy {g[0] / 1e3:8.2f} ms ({g[1] / 1e3:.2f} .. {g[2] / 1e3:.2f})   speculative {sp[0] / 1e3:8.2f} ms ({sp[1] / 1e3:.2f} .. {sp[2] / 1e3:.2f})"
            f"   greedy / speculative {g[0] / sp[0]:5.2f}x   same tokens: {got.tolist() == want.tolist()}")
        say(f"      verify passes {int(st[0])}, drafted {int(st[1])}, accepted {int(st[2])}, plain decode steps {int(st[3])}; "
            f"distinct tokens among the 256 greedy ones: {distinct}")
    if model == "llama-3.2-1b" and qt == S.Q8_0:
        path = os.environ.get("VERIFY_RATE_OUT") or os.path.join(ROOT, "profiles", "verify_rate_llama1b.txt")      # (VERIFY_RATE_OUT: another place, e.g. for an A/B build)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
