"""What the ragged batch pass (lmrs_batch_forward_runs) costs against the calls it replaces, on a full-size synthetic model, in one process.
  admission   16 prompts x 32 tokens in ONE forward_runs call (n_out = 1: every prompt's first new token) against 16 lmrs_batch_prefill calls (31 tokens
              each) plus one lmrs_batch_forward over the 16 last tokens; the same with 4 prompts x 128 tokens
  mixed step  12 decode rows plus one 4-row draft run against lmrs_batch_forward with the 12 rows (the cost of adding the draft run); 15 decode rows plus a
              64-token prompt chunk against the 15-row step followed by a 64-token lmrs_batch_prefill
Time: HIP events recorded on the null stream before and after each side (every library call ends with a host synchronise, so the device is idle at both
records): the device's clock from the first enqueue to the last synchronise, the same for both sides.  Median of 5 after 2 warm-ups, with minimum and
maximum.  Every timed configuration's token ids are compared with the same sequence run alone on the context's own cache.
usage: python tools/runs_rate.py [model] [q8_0|q4_0]
       (writes profiles/batch_runs_llama1b.txt for llama-3.2-1b q8_0, profiles/batch_runs_gemma2b_q4.txt for gemma-2-2b q4_0)"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import lmrs_amd  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402

OUT = {("llama-3.2-1b", S.Q8_0): "batch_runs_llama1b.txt", ("gemma-2-2b", S.Q4_0): "batch_runs_gemma2b_q4.txt"}
DEPTH = 100                                                   # where the decode rows of the mixed steps stand


class DeviceClock:
    """two HIP events on the null stream around a call that synchronises with the host before it returns"""

    def __init__(self):
        self.hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
        self.ev = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.ev:
            self.ok(self.hip.hipEventCreate(ctypes.byref(e)))

    @staticmethod
    def ok(rc):
        if rc:
            raise RuntimeError(f"HIP error {rc}")

    def us(self, fn):
        self.ok(self.hip.hipEventRecord(self.ev[0], None))
        out = fn()
        self.ok(self.hip.hipEventRecord(self.ev[1], None))
        self.ok(self.hip.hipEventSynchronize(self.ev[1]))
        ms = ctypes.c_float()
        self.ok(self.hip.hipEventElapsedTime(ctypes.byref(ms), self.ev[0], self.ev[1]))
        return out, ms.value * 1e3


def timed(clock, fn, reps=5, warm=2):
    """-> (result of the last run, median, min, max in microseconds)"""
    for _ in range(warm):
        fn()
    runs = [clock.us(fn) for _ in range(reps)]
    us = [t for _, t in runs]
    return runs[-1][0], statistics.median(us), min(us), max(us)


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "llama-3.2-1b"
    qname = sys.argv[2] if len(sys.argv) > 2 else "q8_0"
    qt = S.Q4_0 if qname == "q4_0" else S.Q8_0
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    img = S.build_image(model, qt, 1234)
    m = lmrs_amd.Transformer(img)
    b = lmrs_amd.Batch(m, 16)
    clock = DeviceClock()
    say(f"python tools/runs_rate.py {model} {qname}")
    say(f"{model} {qname.upper()}, synthetic weights (tools/synth_lmrs.py seed 1234); kernel_source_hash {bench.kernel_source_hash()}")
    say("HIP events on the null stream around each side (every call ends with a host synchronise); median of 5 after 2 warm-ups (min .. max)")

    def pair(name, new, old, want):
        """the two sides of one comparison; both must give `want`, the single-context token ids"""
        a, ua, la, ha = timed(clock, new)
        o, uo, lo, ho = timed(clock, old)
        same = [int(x) for x in a] == [int(x) for x in o] == [int(x) for x in want]
        assert same, f"{name}: token ids differ from the single-context run: {list(a)} / {list(o)} / {list(want)}"
        say(f"  {name}")
        say(f"    forward_runs   {ua:9.1f} us ({la:.1f} .. {ha:.1f})")
        say(f"    existing calls {uo:9.1f} us ({lo:.1f} .. {ho:.1f})   existing / forward_runs = {uo / ua:5.2f}x   same tokens as the single-context runs: {same}")

    def alone(prompt):
        """the first new token behind `prompt`, on the context's own cache"""
        return int(m.generate_greedy(prompt, 1, 0)[0])

    say("admission: every prompt's first new token")
    for n, length in ((16, 32), (4, 128)):
        prompts = [S.prompt_tokens(model, length, 300 + i) for i in range(n)]
        want = [alone(p) for p in prompts]
        slots = list(range(n))

        def new():
            return b.forward_runs([(i, 0, p, 1) for i, p in enumerate(prompts)])

        def old():
            for i, p in enumerate(prompts):
                b.prefill(i, p[:-1], 0)
            return b.forward(slots, [int(p[-1]) for p in prompts], [length - 1] * n)

        pair(f"{n} prompts x {length} tokens: one call against {n} lmrs_batch_prefill + one lmrs_batch_forward", new, old, want)

    say(f"mixed steps, decode rows at {DEPTH} positions")
    prompts = [S.prompt_tokens(model, DEPTH + 4, 400 + i) for i in range(16)]
    for i, p in enumerate(prompts):
        b.prefill(i, p[:DEPTH], 0)
    want = [alone(p[:DEPTH + 1]) for p in prompts]
    # the draft run: slot 12 feeds 4 tokens from DEPTH on; its rows against lmrs_verify_tokens alone
    m.prefill_tokens(prompts[12][:DEPTH], 0)
    draft_want = [int(t) for t in m.verify_tokens(prompts[12][DEPTH:DEPTH + 4], DEPTH)[0]]
    rows12 = [(i, DEPTH, [int(prompts[i][DEPTH])], 1) for i in range(12)]
    got, u_mix, lo, hi = timed(clock, lambda: b.forward_runs(rows12 + [(12, DEPTH, prompts[12][DEPTH:DEPTH + 4], 4)]))
    base, u_base, blo, bhi = timed(clock, lambda: b.forward(list(range(12)), [int(prompts[i][DEPTH]) for i in range(12)], [DEPTH] * 12))
    same = [int(x) for x in got] == want[:12] + draft_want and [int(x) for x in base] == want[:12]
    assert same, "12 decode rows + a draft run: token ids differ from the single-context runs"
    say("  12 decode rows + one 4-row draft run (16 rows) against lmrs_batch_forward with the 12 rows")
    say(f"    forward_runs   {u_mix:9.1f} us ({lo:.1f} .. {hi:.1f})")
    say(f"    12-row step    {u_base:9.1f} us ({blo:.1f} .. {bhi:.1f})   the draft run adds {u_mix - u_base:.1f} us ({u_mix / u_base:5.2f}x)   same tokens: {same}")
    chunk = S.prompt_tokens(model, 65, 500)
    rows15 = [(i, DEPTH, [int(prompts[i][DEPTH])], 1) for i in range(15)]

    def old15():
        am = b.forward(list(range(15)), [int(prompts[i][DEPTH]) for i in range(15)], [DEPTH] * 15)
        b.prefill(15, chunk[:64], 0)
        return am

    pair("15 decode rows + a 64-token prompt chunk (79 rows) against the 15-row step, then a 64-token lmrs_batch_prefill",
         lambda: b.forward_runs(rows15 + [(15, 0, chunk[:64], 0)]), old15, want[:15])
    # the chunk's K/V rows serve the prompt's next token as the single-context run has it
    assert int(b.forward([15], [int(chunk[64])], [64])[0]) == alone(chunk), "the admitted chunk's rows differ from the single-context run"
    name = OUT.get((model, qt))
    if name:
        path = os.environ.get("RUNS_RATE_OUT") or os.path.join(ROOT, "profiles", name)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
