"""Wall-clock cost of lmrs_prefill_tokens (a prompt from token ids: K/V rows only, no logits) on a full-size synthetic model: the batched pass
(a context created with LMRS_TOKENS_BATCH_MIN=2, so that every run length below takes it) against the token path (a context created with
LMRS_NO_BATCHED_PREFILL=1: one decode step per token, the classifier's result ignored).  Best of three calls after one warm-up, host wall
clock around the whole call, and the spread (max - min) of the three.  "crossover": the smallest measured n at which the batched pass wins by
more than the larger of the two spreads - the run length from which the library batches by default (tokens_batch_min, lmrs_api.hip).
usage: python tools/prompt_rate.py [model] [q8_0|q4_0]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import lmrs_amd  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402


def timed(fn, reps=3):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append((time.perf_counter() - t0) * 1e3)
    return min(out), max(out) - min(out)


def create(img, **env):
    os.environ.update(env)                                 # (switches are read at create)
    try:
        return lmrs_amd.Transformer(img)
    finally:
        for k in env:
            del os.environ[k]


model = sys.argv[1] if len(sys.argv) > 1 else "llama-3.2-1b"
qt = S.Q4_0 if len(sys.argv) > 2 and sys.argv[2] == "q4_0" else S.Q8_0
img = S.build_image(model, qt, 1234)
default = lmrs_amd.Transformer(img)
batched = create(img, LMRS_TOKENS_BATCH_MIN="2")
token = create(img, LMRS_NO_BATCHED_PREFILL="1")
toks = S.prompt_tokens(model, 512, 7)
nl = default.args.n_layers
print(f"{model} {'Q4_0' if qt == S.Q4_0 else 'Q8_0'}: prefill_tokens wall clock (ms), best of 3 (spread of the 3)")
crossover = None
for n in (4, 8, 16, 32, 64, 128, 512):
    assert batched.tokens_path(n) and not token.tokens_path(n)
    tb, sb = timed(lambda: batched.prefill_tokens(toks[:n], 0))
    tt, st = timed(lambda: token.prefill_tokens(toks[:n], 0))
    td, _ = timed(lambda: default.prefill_tokens(toks[:n], 0))
    same = all(np.array_equal(a.kv_row(w, l, p).view(np.uint32), token.kv_row(w, l, p).view(np.uint32))
               for a in (batched, default) for w in (0, 1) for l in (0, nl - 1) for p in sorted({0, n // 2, n - 1}))
    if crossover is None and tt - tb > max(sb, st):
        crossover = n
    print(f"  n={n:4d}  batched {tb:8.3f} ms ({sb:6.3f})   token by token {tt:8.3f} ms ({st:6.3f})   ratio {tt / tb:6.2f}x"
          f"   default context: {'batched' if default.tokens_path(n) else 'token  '} {td:8.3f} ms   same K/V bits: {same}")
print(f"  crossover: batched wins by more than the spread from n = {crossover}")
