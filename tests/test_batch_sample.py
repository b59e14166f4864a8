"""lmrs_batch_forward_sample (include/lmrs_hip.h): lmrs_batch_forward's pass with a sampler per row, sampled on the device.  The reference is one CPU
oracle PER SEQUENCE running the sequential forward (transformer.rs:316-384) followed by the oracle's Sampler::sample (sampler.rs:109-129), one
persistent Sampler per sequence on each side: every token is compared token for token, every K/V row bit for bit.  No tolerances."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from tools import synth_lmrs as S

gpu = pytest.mark.gpu

# (temperature, top_p): argmax, sample_mult, sample_mult (top_p 0), the default flags' top-p, a peaked top-p, a flat top-p
KINDS = [(0.0, 0.9), (0.8, 1.0), (1.5, 0.0), (0.7, 0.9), (0.05, 0.5), (3.0, 0.999)]
SORT_MIN = 4096                                                                      # LMRS_TOPP_DEVICE_SORT_MIN's default: candidates from which a row is sorted on the device


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


class Seq:
    """one sequence: its slot, its own oracle, its sampler on either side, the tokens fed so far"""

    def __init__(self, L, img, slot, kind, seed):
        self.slot, self.orc, self.n, self.kind = slot, O.Oracle(img), 0, kind
        V = self.orc.args.vocab_size
        self.dev, self.ref = L.Sampler(V, kind[0], kind[1], seed), O.Sampler(V, kind[0], kind[1], seed)

    def feed(self, toks):
        lg = None
        for t in toks:
            lg = self.orc.forward(int(t), self.n).copy()
            self.n += 1
        return lg

    def want(self, tok):
        """the oracle's forward + Sampler::sample at the sequence's end -> (token, the probabilities - or logits at temperature 0)"""
        lg = self.feed([tok])
        return self.ref.sample(lg), lg


def check_slot_rows(b, s, positions, what):
    for layer in range(s.orc.args.n_layers):
        for p in positions:
            for which in (0, 1):
                assert_bit_equal(b.kv_row(s.slot, which, layer, p), s.orc.kv_row(which, layer, p), f"{what}: slot {s.slot} {'kv'[which]} layer {layer} pos {p}")


def make(L, img, cfg, lengths, kinds, seed=1000, n_slots=None):
    m = L.Transformer(img)
    b = L.Batch(m, n_slots or len(lengths))
    seqs = []
    for i, n in enumerate(lengths):
        s = Seq(L, img, i, kinds[i % len(kinds)], seed + i)
        if n:
            toks = S.prompt_tokens(cfg, n, 50 + i)
            assert b.prefill(i, toks, 0) == n
            s.feed(toks)
        seqs.append(s)
    return m, b, seqs


def sampled_step(b, seqs, toks, what, kv=True):
    """one forward_sample over `seqs` (in that order) feeding toks[i] at each sequence's end, judged against the oracles -> the tokens"""
    pos = [s.n for s in seqs]
    got = b.forward_sample([s.slot for s in seqs], toks, pos, [s.dev for s in seqs])
    want = []
    for i, s in enumerate(seqs):
        w, _ = s.want(toks[i])
        want.append(w)
        if kv:
            check_slot_rows(b, s, [pos[i]], what)
    assert got.tolist() == want, f"{what}: tokens {got.tolist()} vs the oracle's {want} (kinds {[s.kind for s in seqs]})"
    return got


# ---------------------------------------------------------------------------------------------- 1. mixed samplers in one pass

DEPTHS = [0, 1, 2, 7, 63, 64, 65, 1, 2, 3, 1, 2, 3, 1, 2, 3]                          # 220 prefilled tokens + 8 x 16 + 1 + 3 steps: under 400 oracle tokens


@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_mixed_samplers_in_one_pass(L, cfg, q):
    img = S.build_image(cfg, q, seed=81)
    m, b, seqs = make(L, img, cfg, DEPTHS, KINDS)
    V = seqs[0].orc.args.vocab_size
    toks = [(13 * i + 3) % V for i in range(16)]
    for k in range(8):
        toks = sampled_step(b, seqs, toks, f"{cfg} q{q} step {k}").tolist()          # each row is fed its own sampled token
    sampled_step(b, [seqs[5]], [toks[5]], f"{cfg} q{q} n = 1")
    sub = [seqs[11], seqs[3], seqs[4]]                                                # shuffled slot order: top-p, top-p, mult behind rows the others left
    sampled_step(b, sub, [toks[11], toks[3], toks[4]], f"{cfg} q{q} 3-row subset")


# ---------------------------------------------------------------------------------------------- 2. the stale vector across calls

@gpu
def test_the_stale_candidate_vector_across_calls(L):
    """sample_topp sorts its WHOLE persistent vector, entries of earlier calls included (sampler.rs:81): 30 calls on one sampler per row"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=82)
    m, b, seqs = make(L, img, cfg, [0, 0, 0, 0], [(0.7, 0.9), (1.0, 0.3)])
    rng = np.random.default_rng(5)
    for k in range(30):
        sampled_step(b, seqs, rng.integers(0, 4096, 4).tolist(), f"stale vector step {k}", kv=k in (0, 29))


# ---------------------------------------------------------------------------------------------- 3. both candidate routes in one call

def n0_of(probs, top_p):
    cutoff = (np.float32(1.0) - np.float32(top_p)) / np.float32(probs.size - 1)
    return int((probs >= cutoff).sum())


@gpu
def test_both_candidate_routes_in_one_call(L):
    """vocabulary 40 000: a flat row (>= 4096 candidates: sorted on the device) beside a peaked one (its pairs cross as they are), and a third row whose
    one sampler meets both kinds over the run - its temperature is chosen from the ORACLE's probabilities of the tokens it will be fed"""
    cfg = "mini-llama-v40k"
    img = S.build_image(cfg, S.Q8_0, seed=83)
    V, steps = 40000, 10
    fixed = S.prompt_tokens(cfg, steps, 9).tolist()                                   # the third row's inputs: not fed back, so its logits are known in advance
    orc = O.Oracle(img)
    rows = [orc.forward(t, i).copy() for i, t in enumerate(fixed)]
    temp3 = None
    for T in (0.3, 0.25, 0.2, 0.17, 0.15, 0.13, 0.11, 0.1, 0.09, 0.08, 0.07, 0.06, 0.05, 0.04):
        ns = []
        for r in rows:
            lg = r.copy(); O.Sampler(V, T, 0.9, 1).sample(lg); ns.append(n0_of(lg, 0.9))
        if min(ns) < SORT_MIN <= max(ns):
            temp3 = T
            break
    assert temp3 is not None, "no temperature at which the third row's candidates straddle the sort threshold: choose other tokens"
    m, b, seqs = make(L, img, cfg, [0, 0, 0], [(0.7, 0.9), (0.02, 0.9), (temp3, 0.9)])
    toks = [5, 6, fixed[0]]
    seen = [set(), set(), set()]
    for k in range(steps):
        pos = [s.n for s in seqs]
        got = b.forward_sample([0, 1, 2], toks, pos, [s.dev for s in seqs])
        for i, s in enumerate(seqs):
            w, probs = s.want(toks[i])
            seen[i].add(n0_of(probs, 0.9) >= SORT_MIN)
            assert int(got[i]) == w, f"v40k step {k} row {i} {s.kind}: {got[i]} vs {w}"
        check_slot_rows(b, seqs[k % 3], [pos[k % 3]], f"v40k step {k}")
        toks = [int(got[0]), int(got[1]), fixed[k + 1] if k + 1 < steps else 0]
    # the inputs are what the test is about: the device-sort route, the plain route, and one sampler that took both
    assert True in seen[0] and False in seen[1] and seen[2] == {True, False}, seen


# ---------------------------------------------------------------------------------------------- 4. interleaving

@gpu
def test_interleaving_with_the_other_calls(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=84)
    m, b, seqs = make(L, img, cfg, [3, 0, 9, 1], KINDS[1:])
    own, own_dev, own_ref, n_own = O.Oracle(img), L.Sampler(4096, 0.7, 0.9, 77), O.Sampler(4096, 0.7, 0.9, 77), 0
    toks = [11, 12, 13, 14]
    toks = sampled_step(b, seqs, toks, "before").tolist()
    # the context's own forward_sample (its cache is a sequence of its own)
    for t in (21, 22):
        lg = own.forward(t, n_own).copy()
        assert m.forward_sample(t, n_own, own_dev) == own_ref.sample(lg), "the context's forward_sample"
        n_own += 1
    toks = sampled_step(b, seqs, toks, "after forward_sample").tolist()
    # Batch.forward with logits on two of the slots
    pos = [seqs[0].n, seqs[2].n]
    am, lg = b.forward([0, 2], [31, 32], pos, logits=True)
    for i, s in enumerate((seqs[0], seqs[2])):
        want = s.feed([31 + i])
        assert_bit_equal(lg[i], want, f"batch forward row {i}"); assert int(am[i]) == ref_argmax(want)
    toks = sampled_step(b, seqs, toks, "after forward").tolist()
    # generate_greedy of 3 steps on slot 1
    out = b.generate_greedy([1], [41], [seqs[1].n], 3)
    t = 41
    for j in range(3):
        t2 = ref_argmax(seqs[1].feed([t]))
        assert int(out[0, j]) == t2, f"generate_greedy step {j}"
        t = t2
    toks = sampled_step(b, seqs, toks, "after generate_greedy").tolist()
    # forward_runs: a 5-token run on slot 3, one decode row on slot 0
    run = [51, 52, 53, 54, 55]
    am = b.forward_runs([(3, seqs[3].n, run, 1), (0, seqs[0].n, [56], 1)])
    assert int(am[0]) == ref_argmax(seqs[3].feed(run)) and int(am[1]) == ref_argmax(seqs[0].feed([56])), "forward_runs"
    toks = sampled_step(b, seqs, toks, "after forward_runs").tolist()
    sampled_step(b, seqs, toks, "last")
    lg = own.forward(23, n_own).copy()
    assert m.forward_sample(23, n_own, own_dev) == own_ref.sample(lg), "the context's forward_sample at the end"


# ---------------------------------------------------------------------------------------------- 5. errors

@gpu
def test_errors_come_before_device_work_and_leave_everything_usable(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=85)
    m, b, seqs = make(L, img, cfg, [2, 0, 1], [(0.7, 0.9), (0.8, 1.0), (0.0, 0.9)], n_slots=3)
    lib = L.lib()
    other_vocab = L.Sampler(4100, 0.7, 0.9, 1)
    state = {"toks": [1, 2, 3]}

    def valid(what):
        state["toks"] = sampled_step(b, seqs, state["toks"], what).tolist()

    u32 = lambda *v: np.array(v, np.uint32)
    hs = lambda *s: (ctypes.c_void_p * len(s))(*[None if x is None else x._h for x in s])
    S3 = [s.dev for s in seqs]
    nxt = np.zeros(16, np.uint32)

    def call(n=3, slot=u32(0, 1, 2), tok=u32(1, 2, 3), pos=None, samplers=S3, nx=nxt, batch=b._h):
        pos = u32(*[s.n for s in seqs][:max(n, 1)]) if pos is None else pos
        arr = hs(*samplers) if samplers is not None else None
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        return lib.lmrs_batch_forward_sample(batch, n, p(slot), p(tok), p(pos), ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, p(nx))

    valid("first")
    cases = [
        (dict(batch=None), "NULL argument"),
        (dict(slot=None), "NULL array"), (dict(tok=None), "NULL array"), (dict(samplers=None), "NULL array"), (dict(nx=None), "NULL array"),
        (dict(n=0), "n = 0 is outside 1 .. 16"), (dict(n=17), "n = 17 is outside 1 .. 16"),
        (dict(slot=u32(0, 3, 2)), "row 1: slot 3 of 3"),
        (dict(slot=u32(0, 1, 1)), "slot 1 appears twice"),
        (dict(tok=u32(1, 4096, 3)), "token 1 out of range"),
        (dict(pos=u32(0, 256, 0)), "row 1: pos + 1 positions exceeds seq_len"),
        (dict(samplers=[S3[0], None, S3[2]]), "row 1: the sampler is NULL"),
        (dict(samplers=[S3[0], other_vocab, S3[2]]), "row 1: the sampler was made for another vocabulary size"),
        (dict(samplers=[S3[0], S3[1], S3[0]]), "row 2: the top-p sampler of row 0 appears twice"),
    ]
    for kw, msg in cases:
        assert call(**kw) != 0, kw
        assert msg in lib.lmrs_last_error().decode(), (kw, lib.lmrs_last_error().decode())
        valid(f"after {msg!r}")
    # stateless samplers may be shared: the argmax sampler in two rows, then the sample_mult sampler (the third row: slot 2 with sequence 0's top-p sampler)
    for k in (2, 1):
        pos = [s.n for s in seqs]
        got = b.forward_sample([0, 1, 2], [7, 8, 9], pos, [S3[k], S3[k], S3[0]])
        want = []
        for i, s in enumerate(seqs):
            lg = s.feed([7 + i])
            want.append(seqs[0].ref.sample(lg) if i == 2 else O.Sampler(4096, *seqs[k].kind, 1000 + k).sample(lg))
        assert got.tolist() == want, f"the sampler {seqs[k].kind} shared by two rows"
    valid("last")


@gpu
def test_a_top_p_row_without_a_candidate_fails_with_its_row(L):
    """top_p so small that (1 - top_p) / (n - 1) exceeds every probability of a flat row: the reference panics, the call names the row"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=86)
    m = L.Transformer(img); b = L.Batch(m, 2)
    ok, none = L.Sampler(4096, 0.8, 1.0, 1), L.Sampler(4096, 1e6, 1e-6, 2)              # p = 1 / 4096 each, the cutoff 1 / 4095
    with pytest.raises(L.LmrsError, match=r"row 1: sample_topp: no candidate above the cutoff"):
        b.forward_sample([0, 1], [5, 6], [0, 0], [ok, none])
    orc = O.Oracle(img)
    lg = orc.forward(5, 0).copy()
    assert int(b.forward_sample([0], [5], [0], [ok])[0]) == O.Sampler(4096, 0.8, 1.0, 1).sample(lg)
