"""Wall-clock rate of lmrs_score_tokens (the log-probability of every next token of a sequence) on a full-size synthetic Llama-3.2-1B Q8_0:
the batched path (forward_layer and the classifier over the token batch on the int8 matrix cores) against the token-by-token path (a second
context created with LMRS_NO_BATCHED_PREFILL=1: one decode step per token), and lmrs_forward_tokens at 512 tokens (all logits to the host).
Best of three calls after one warm-up, host wall clock around the whole call.
--topk K[,K...]: instead, what the k first candidates of every position cost (lmrs_score_tokens_topk) - 512 tokens on the batched path, plain
score and score_topk(K) by turns, three repetitions of the best-of-three each, and a decode step with the logits copied (forward) against one
with the selection on the device (forward_topk).
usage: python tools/score_rate.py [model] [q8_0|q4_0] [--topk K[,K...]]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import lmrs_amd  # noqa: E402
from tools import synth_lmrs as S  # noqa: E402


def best_ms(fn, reps=3):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return min(out) * 1e3


argv = sys.argv[1:]
topk = []
if "--topk" in argv:
    i = argv.index("--topk")
    topk = [int(k) for k in argv[i + 1].split(",")]
    del argv[i:i + 2]
model = argv[0] if len(argv) > 0 else "llama-3.2-1b"
qt = S.Q4_0 if len(argv) > 1 and argv[1] == "q4_0" else S.Q8_0
img = S.build_image(model, qt, 1234)
batched = lmrs_amd.Transformer(img)
if topk:
    toks = S.prompt_tokens(model, 512, 7)
    print(f"{model} {'Q4_0' if qt == S.Q4_0 else 'Q8_0'}: 512 tokens, wall clock (ms), best of 3 calls, three repetitions")
    plain = batched.score(toks, 0)
    for rep in range(3):
        line = f"  rep {rep}: score {best_ms(lambda: batched.score(toks, 0)):7.3f}"
        for k in topk:
            line += f"   score_topk({k}) {best_ms(lambda: batched.score_topk(toks, k, 0)):7.3f}"
        print(line)
    for k in topk:
        r = batched.score_topk(toks, k, 0)
        same = np.array_equal(r[0].view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(r[1], plain[1]) and r[2] == plain[2]
        print(f"  k={k}: logprobs / argmax / sum are score()'s bits: {same}   rank 0 is the argmax: {np.array_equal(r[3][:, 0], r[1])}"
              f"   top-1 {np.mean(r[5] == 0):.4f} top-{k} {np.mean(r[5] < k):.4f} mean target rank {np.mean(r[5]):.1f}")
    steps = 200
    def decode(step):
        t0 = time.perf_counter()
        for i in range(steps):
            step(int(toks[i]), i)
        return (time.perf_counter() - t0) / steps * 1e6
    decode(lambda t, p: batched.forward(t, p))
    line = f"  decode, us/token over {steps} steps: forward {decode(lambda t, p: batched.forward(t, p)):7.1f}   forward_argmax {decode(batched.forward_argmax):7.1f}"
    for k in topk:
        decode(lambda t, p: batched.forward_topk(t, p, k))
        line += f"   forward_topk({k}) {decode(lambda t, p: batched.forward_topk(t, p, k)):7.1f}"
    print(line)
    sys.exit(0)
os.environ["LMRS_NO_BATCHED_PREFILL"] = "1"              # (read at create)
token = lmrs_amd.Transformer(img)
del os.environ["LMRS_NO_BATCHED_PREFILL"]
toks = S.prompt_tokens(model, 1024, 7)
print(f"{model} {'Q4_0' if qt == S.Q4_0 else 'Q8_0'}: score_tokens wall clock (ms), best of 3")
for n in (16, 128, 512, 1024):
    tb = best_ms(lambda: batched.score(toks[:n], 0))
    tt = best_ms(lambda: token.score(toks[:n], 0))
    rb, rt = batched.score(toks[:n], 0), token.score(toks[:n], 0)
    same = np.array_equal(rb[0].view(np.uint32), rt[0].view(np.uint32)) and np.array_equal(rb[1], rt[1]) and rb[2] == rt[2]
    print(f"  n={n:5d}  batched {tb:8.2f} ms ({tb / n * 1e3:7.1f} us/token)   token by token {tt:8.2f} ms ({tt / n * 1e3:7.1f} us/token)"
          f"   ratio {tt / tb:5.1f}x   same bits: {same}   ppl {np.exp(-rb[2] / (n - 1)):.3f}")
tf = best_ms(lambda: batched.forward_tokens(toks[:512], 0))
print(f"  forward_tokens n=512: {tf:.2f} ms (including the {512 * batched.args.vocab_size * 4 / 1e6:.0f} MB of logits to host memory)")
