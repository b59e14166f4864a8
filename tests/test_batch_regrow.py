"""The sets of a batch that grow on demand (lm.rs_amd/csrc/lmrs_api.hip: alloc_all over the owners of lmrs_buf.h), each used at more than one size on ONE
wide batch: lmrs_batch_forward_runs_sample's sampling set (2 sampled runs: 16 rows; 33: made anew for 48; 2 again), the top-k buffers (k = 2, then 8, then 2
again in the larger ones) and the flat rows' sort buffers (two flat top-p rows, then five).  The reference of every call is a FRESH batch on the same context
with freshly made samplers of the same seeds: every token, index and log-probability of the reused batch equals the fresh batch's, bit for bit.  Every run
starts at position 0, so no call reads what an earlier one left in a slot.  Deterministic; no allocation is made to fail."""
import numpy as np
import pytest

import oracle_lib as O
from test_batch_sample import SORT_MIN, n0_of
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
CFG = "mini-llama"                                                                    # vocabulary 4096 = the sort threshold: (3.0, 0.999) keeps all of it
PEAKED = [(0.0, 0.9), (0.8, 1.0), (1.5, 0.0), (0.05, 0.5)]                            # argmax, sample_mult twice, a top-p row of a handful of candidates
FLAT = (3.0, 0.999)                                                                   # tests/test_batch_runs_sample.py's flat top-p kind


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


@gpu
def test_a_reused_batch_equals_a_fresh_one_at_every_size(L):
    img = S.build_image(CFG, S.Q8_0, seed=311)
    m = L.Transformer(img)
    V = m.args.vocab_size
    reused = L.Batch(m, 64, wide=True)
    assert reused.width == 64

    def both(call, what):
        got = call(reused)
        fresh = L.Batch(m, 64, wide=True)
        try:
            want = call(fresh)
        finally:
            fresh.close()
        got, want = (x if isinstance(x, tuple) else (x,) for x in (got, want))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.dtype == w.dtype, what
            assert (g.view(np.uint32) == w.view(np.uint32)).all(), f"{what}: the reused batch {g.tolist()} vs a fresh one {w.tolist()}"
        return got

    def sampled(spec, seed):
        """spec = [(slot, tokens, kind)]: the call with samplers made here, by seed"""
        def call(b):
            samplers = [L.Sampler(V, k[0], k[1], seed + i) for i, (_, _, k) in enumerate(spec)]
            return b.forward_runs_sample([(slot, 0, toks, s) for (slot, toks, _), s in zip(spec, samplers)])
        return call

    def runs(n, seed, kinds):
        return [(i, S.prompt_tokens(CFG, 1 + (i * 7 + seed) % 3, seed + i), kinds[i % len(kinds)]) for i in range(n)]

    # ---- the sampling set: 16 rows, made anew for 48, then 2 runs in the larger set
    both(sampled(runs(2, 4000, [PEAKED[3], PEAKED[1]]), 5000), "2 sampled runs")
    both(sampled(runs(33, 4100, PEAKED), 5100), "33 sampled runs")
    both(sampled(runs(2, 4200, [PEAKED[3], PEAKED[1]]), 5200), "2 sampled runs after 33")

    # ---- top-k: k = 2, then 8 (the buffers grow), then 2 in the buffers made for 8
    def topk(k, seed):
        spec = [(3 * i, 0, S.prompt_tokens(CFG, 2 + i, seed + i), 1 + i % 2) for i in range(5)]
        return lambda b: b.forward_runs(spec, k=k)
    for k, seed in ((2, 4300), (8, 4400), (2, 4500)):
        am, ti, tl = both(topk(k, seed), f"forward_runs, k = {k}")
        assert am.shape == (7,) and ti.shape == (7, k) and tl.shape == (7, k)

    # ---- the flat rows' sort: two flat rows, then five, each beside rows that cross as they are.  What a row was is read off the ORACLE's probabilities
    orc = O.Oracle(img)
    for n_flat, seed in ((2, 4600), (5, 4700)):
        spec = [(2 * i, [(seed + 37 * i) % V], FLAT if i < n_flat else PEAKED[1 + i % 3]) for i in range(n_flat + 3)]
        flat = 0
        for i, (_, toks, kind) in enumerate(spec):
            if 0.0 < kind[1] < 1.0:
                probs = orc.forward(toks[0], 0).copy()
                O.Sampler(V, kind[0], kind[1], seed + i).sample(probs)                # (in place: the probabilities now)
                flat += n0_of(probs, kind[1]) >= SORT_MIN
        assert flat == n_flat, f"{flat} flat rows where {n_flat} were meant: choose other kinds"
        both(sampled(spec, seed), f"{n_flat} flat top-p rows")
