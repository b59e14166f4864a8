"""lmrs_batch_forward_runs_sample (include/lmrs_hip.h): lmrs_batch_forward_runs' pass with a sampler per run - the last row of every run sampled on the
device, up to the batch's width of rows, the flat top-p rows of a call sorted together.  The reference is one CPU oracle PER SEQUENCE running the
sequential forward (transformer.rs:316-384) followed by the oracle's Sampler::sample (sampler.rs:109-129), one persistent Sampler per sequence on each
side (tests/test_batch_sample.py's Seq): every token is compared token for token, every K/V row bit for bit.  No tolerances.
Not covered here: the refusal of more outputs than the logits block holds rows - the block holds 512 MiB, so 64 outputs overflow it only from a
vocabulary of two million entries on."""
import ctypes
import dataclasses

import numpy as np
import pytest

import oracle_lib as O
from parity_rules import assert_bit_equal, ref_argmax
from test_batch_sample import KINDS, SORT_MIN, Seq, check_slot_rows, n0_of
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
HERE = object()                                                                       # an argument of the raw call left to its default


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def is_topp(kind):
    return kind[0] != 0.0 and 0.0 < kind[1] < 1.0


def make(L, img, cfg, lengths, kinds, seed, wide=True, n_slots=None):
    """slot i prefilled with lengths[i] tokens, one oracle and one sampler pair per slot"""
    m = L.Transformer(img)
    b = L.Batch(m, n_slots or len(lengths), wide=wide)
    seqs = []
    for i, n in enumerate(lengths):
        s = Seq(L, img, i, kinds[i % len(kinds)], seed + i)
        if n:
            toks = S.prompt_tokens(cfg, n, 50 + i)
            assert b.prefill(i, toks, 0) == n
            s.feed(toks)
        seqs.append(s)
    return m, b, seqs


def runs_step(b, entries, what, kv="all"):
    """one forward_runs_sample over entries = [(seq, tokens, sampled)] in that order, judged against the oracles -> (tokens, the flat rows' n0, the other
    top-p rows' n0); kv: "all" checks every K/V row the call wrote, "last" the last row of every run, None none"""
    got = b.forward_runs_sample([(s.slot, s.n, toks, s.dev if sampled else None) for s, toks, sampled in entries])
    want, flat, peaked = [], [], []
    for s, toks, sampled in entries:
        p0 = s.n
        lg = s.feed(toks)
        if sampled:
            want.append(s.ref.sample(lg))                                             # (lg: the probabilities now)
            if is_topp(s.kind):
                n0 = n0_of(lg, s.kind[1])
                (flat if n0 >= SORT_MIN else peaked).append(n0)
        else:
            want.append(0)
        if kv:
            check_slot_rows(b, s, range(p0, s.n) if kv == "all" else [s.n - 1], what)
    assert got.tolist() == want, f"{what}: tokens {got.tolist()} vs the oracle's {want} (kinds {[e[0].kind for e in entries]})"
    return got, flat, peaked


# ---------------------------------------------------------------------------------------------- 1. wide steps

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_sampled_steps_of_a_wide_batch(L, cfg, q):
    """passes of 64, 48, 40 and 17 runs of one token (the ring kernels, the hand-over, the stream GEMM), the six sampler kinds cycling over the slots,
    every row fed its own sampled token: 63 prefilled tokens + 2 x 169 rows"""
    img = S.build_image(cfg, q, seed=301)
    m, b, seqs = make(L, img, cfg, [i % 3 for i in range(64)], KINDS, 3000)
    assert b.width == 64
    V = seqs[0].orc.args.vocab_size
    last = {s.slot: (13 * s.slot + 3) % V for s in seqs}
    most_flat = 0
    for k in range(2):
        for rows in (seqs, seqs[8:56], seqs[24:64][::-1], seqs[:17]):
            got, flat, _ = runs_step(b, [(s, [last[s.slot]], True) for s in rows], f"{cfg} q{q} round {k}, {len(rows)} runs", kv="all" if k == 0 else None)
            for s, t in zip(rows, got.tolist()):
                last[s.slot] = t
            most_flat = max(most_flat, len(flat))
    # (3.0, 0.999) keeps the whole vocabulary of 4096 - the sort threshold - at every step: slots 5, 11 .. 59 are ten flat rows of every 64-run call, all in one sort
    assert most_flat == 10, most_flat


# ---------------------------------------------------------------------------------------------- 2. ragged

@gpu
@pytest.mark.parametrize("cfg,q", [("mini-llama", S.Q8_0), ("mini-gemma", S.Q4_0)])
def test_prompts_sampled_in_the_pass_that_admits_them(L, cfg, q):
    img = S.build_image(cfg, q, seed=302)
    kinds = [(0.7, 0.9), (0.8, 1.0), (3.0, 0.999), (0.0, 0.9), (0.05, 0.5), (1.5, 0.0)]
    #        slots 0-3: prompts of 1, 5, 17, 33 tokens; 4-5: chunks without a sampler; 6-11: decode rows at depths 2, 0, 1, 2, 0, 1
    m, b, seqs = make(L, img, cfg, [0, 0, 0, 0, 0, 0, 2, 0, 1, 2, 0, 1], kinds, 3100, n_slots=12)
    prompt = lambda i, n: S.prompt_tokens(cfg, n, 700 + i).tolist()
    entries = [(seqs[6], prompt(6, 1), True), (seqs[2], prompt(2, 17), True), (seqs[4], prompt(4, 7), False), (seqs[0], prompt(0, 1), True),
               (seqs[7], prompt(7, 1), True), (seqs[3], prompt(3, 33), True), (seqs[8], prompt(8, 1), True), (seqs[5], prompt(5, 3), False),
               (seqs[1], prompt(1, 5), True), (seqs[9], prompt(9, 1), True), (seqs[10], prompt(10, 1), True), (seqs[11], prompt(11, 1), True)]
    got, _, _ = runs_step(b, entries, f"{cfg} admission")
    assert got[2] == 0 and got[7] == 0                                                # the runs without a sampler
    # the follow-up: every sampled sequence goes on from its own token, the two chunked prompts end (and are sampled)
    nxt = [(e[0], [int(t)], True) if e[2] else (e[0], prompt(20 + e[0].slot, 4), True) for e, t in zip(entries, got.tolist())]
    got, _, _ = runs_step(b, nxt[::-1], f"{cfg} follow-up")
    # K/V rows only: neither the final norm nor the classifier runs
    only = [(seqs[0], prompt(30, 3), False), (seqs[9], prompt(31, 1), False)]
    got, _, _ = runs_step(b, only, f"{cfg} K/V only")
    assert got.tolist() == [0, 0]
    runs_step(b, [(s, [7 + s.slot], True) for s in seqs], f"{cfg} after the K/V-only call", kv="last")


# ---------------------------------------------------------------------------------------------- 3. the same tokens as forward_sample

@gpu
def test_the_same_tokens_as_forward_sample(L):
    """16 runs of one token against Batch.forward_sample on a twin batch with twin samplers, 6 steps: the stale candidate vectors take part"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=303)
    kinds = KINDS + [(0.7, 0.9), (3.0, 0.999), (1.0, 0.3), (3.0, 0.999)]
    sides = []
    for wide in (False, True):
        m = L.Transformer(img)
        b = L.Batch(m, 16, wide=wide)
        sides.append((m, b, [L.Sampler(4096, *kinds[i % len(kinds)], 3200 + i) for i in range(16)]))
    (_, b_old, s_old), (_, b_new, s_new) = sides
    toks = [(29 * i + 1) % 4096 for i in range(16)]
    for k in range(6):
        want = b_old.forward_sample(list(range(16)), toks, [k] * 16, s_old)
        got = b_new.forward_runs_sample([(i, k, [toks[i]], s_new[i]) for i in range(16)])
        assert got.tolist() == want.tolist(), f"step {k}"
        toks = want.tolist()
    for layer in range(2):
        for which in (0, 1):
            assert_bit_equal(b_new.kv_row(5, which, layer, 5), b_old.kv_row(5, which, layer, 5), f"twin K/V rows, layer {layer}")


# ---------------------------------------------------------------------------------------------- 4. several flat sizes in one call

@gpu
def test_flat_rows_of_different_lengths_in_one_sort(L):
    """vocabulary 40 000: (0.7, 0.9) keeps about 34 700 candidates, (1.0, 0.3) about 18 900, (3.0, 0.999) all 40 000 - one sort of 65 536 keys a row, the
    shorter rows padded - and (0.02, 0.9) a handful, which cross as they are.  What each row was is read off the ORACLE's probabilities."""
    cfg = "mini-llama-v40k"
    img = S.build_image(cfg, S.Q8_0, seed=304)
    kinds = [(0.7, 0.9), (1.0, 0.3), (3.0, 0.999), (0.02, 0.9)]
    m, b, seqs = make(L, img, cfg, [0] * 8, kinds, 3300, wide=False)
    toks = [5 + i for i in range(8)]
    ok = False
    for k in range(6):
        got, flat, peaked = runs_step(b, [(s, [toks[s.slot]], True) for s in seqs], f"v40k step {k}", kv="all" if k in (0, 5) else None)
        toks = got.tolist()
        ok = ok or (len(set(flat)) >= 3 and len(peaked) >= 1 and max(flat) > 32768)
    assert ok, "no call had three flat rows of different lengths beside a peaked one: choose other kinds"


# ---------------------------------------------------------------------------------------------- 5. interleaving, errors

@gpu
def test_interleaving_with_the_other_calls(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=305)
    m, b, seqs = make(L, img, cfg, [3, 0, 9, 1], KINDS[1:], 3400, wide=False)
    own, own_dev, own_ref, n_own = O.Oracle(img), L.Sampler(4096, 0.7, 0.9, 77), O.Sampler(4096, 0.7, 0.9, 77), 0
    state = {"toks": [11, 12, 13, 14]}

    def ours(what):
        got, _, _ = runs_step(b, [(s, [state["toks"][s.slot]], True) for s in seqs], what)
        state["toks"] = got.tolist()

    ours("before")
    for t in (21, 22):                                                                # the context's own forward_sample (its cache is a sequence of its own)
        lg = own.forward(t, n_own).copy()
        assert m.forward_sample(t, n_own, own_dev) == own_ref.sample(lg), "the context's forward_sample"
        n_own += 1
    ours("after the context's forward_sample")
    pos = [s.n for s in seqs]                                                         # Batch.forward_sample with the same samplers: both calls move them alike
    got = b.forward_sample([0, 1, 2, 3], state["toks"], pos, [s.dev for s in seqs])
    want = [s.want(state["toks"][s.slot])[0] for s in seqs]
    assert got.tolist() == want, "forward_sample between two calls"
    state["toks"] = want
    ours("after forward_sample")
    run = [51, 52, 53, 54, 55]                                                        # forward_runs: a 5-token run on slot 3, one decode row on slot 0
    am = b.forward_runs([(3, seqs[3].n, run, 1), (0, seqs[0].n, [56], 1)])
    assert int(am[0]) == ref_argmax(seqs[3].feed(run)) and int(am[1]) == ref_argmax(seqs[0].feed([56])), "forward_runs"
    ours("after forward_runs")
    out = b.generate_greedy([1], [41], [seqs[1].n], 3)                                # generate_greedy of 3 steps on slot 1
    t = 41
    for j in range(3):
        t2 = ref_argmax(seqs[1].feed([t]))
        assert int(out[0, j]) == t2, f"generate_greedy step {j}"
        t = t2
    ours("after generate_greedy")
    lg = own.forward(23, n_own).copy()
    assert m.forward_sample(23, n_own, own_dev) == own_ref.sample(lg), "the context's forward_sample at the end"


@gpu
def test_errors_come_before_device_work_and_leave_everything_usable(L):
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=306)
    m, b, seqs = make(L, img, cfg, [2, 0, 1], [(0.7, 0.9), (0.8, 1.0), (0.0, 0.9)], 3500, wide=False, n_slots=3)
    lib = L.lib()
    other_vocab = L.Sampler(4100, 0.7, 0.9, 1)
    state = {"toks": [1, 2, 3]}

    def valid(what):
        got, _, _ = runs_step(b, [(s, [state["toks"][s.slot]], True) for s in seqs], what, kv="last")
        state["toks"] = got.tolist()

    u32 = lambda *v: np.array(v, np.uint32)
    hs = lambda *s: (ctypes.c_void_p * len(s))(*[None if x is None else x._h for x in s])
    S3 = [s.dev for s in seqs]
    nxt = np.zeros(600, np.uint32)
    many = np.zeros(700, np.uint32)

    def call(n=3, slot=u32(0, 1, 2), start=HERE, rl=u32(1, 1, 1), tok=u32(1, 2, 3), samplers=S3, nx=nxt, batch=b._h):
        start = u32(*[s.n for s in seqs]) if start is HERE else start
        arr = hs(*samplers) if samplers is not None else None
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        return lib.lmrs_batch_forward_runs_sample(batch, n, p(slot), p(start), p(rl), p(tok), ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, p(nx))

    valid("first")
    cases = [
        (dict(batch=None), "NULL argument (the batch)"),
        (dict(slot=None), "NULL array"), (dict(start=None), "NULL array"), (dict(rl=None), "NULL array"), (dict(tok=None), "NULL array"),
        (dict(samplers=None), "NULL array"), (dict(nx=None), "NULL array"),
        (dict(n=0), "n_runs = 0 is outside 1 .. 16"), (dict(n=17), "n_runs = 17 is outside 1 .. 16"),
        (dict(rl=u32(1, 0, 1)), "run 1: run_len is 0"),
        (dict(rl=u32(300, 300, 1), tok=many), "the runs hold more than 512 rows"),
        (dict(slot=u32(0, 3, 2)), "run 1: slot 3 of 3"),
        (dict(slot=u32(0, 1, 1)), "slot 1 appears in more than one run"),
        (dict(start=u32(0, 255, 0), rl=u32(1, 2, 1), tok=u32(1, 2, 2, 3)), "run 1: start_pos + run_len exceeds seq_len"),
        (dict(tok=u32(1, 4096, 3)), "token 1 out of range"),
        (dict(samplers=[S3[0], other_vocab, S3[2]]), "run 1: the sampler was made for another vocabulary size (4100, the model has 4096)"),
        (dict(samplers=[S3[0], S3[1], S3[0]]), "run 2: the top-p sampler of run 0 appears twice"),
    ]
    seen = set()
    for kw, msg in cases:
        assert call(**kw) != 0, kw
        err = lib.lmrs_last_error().decode()
        assert err.startswith("lmrs_batch_forward_runs_sample: ") and msg in err, (kw, err)
        seen.add(msg)
        valid(f"after {msg!r}")
    assert len(seen) == 12, "a message each"
    # stateless samplers may be shared by runs: the sample_mult sampler in two of them, the third without a sampler
    pos = [s.n for s in seqs]
    got = b.forward_runs_sample([(0, pos[0], [7], S3[1]), (1, pos[1], [8], S3[1]), (2, pos[2], [9], None)])
    want = [O.Sampler(4096, 0.8, 1.0, 3501).sample(seqs[i].feed([7 + i])) for i in range(2)]
    seqs[2].feed([9])
    assert got.tolist() == want + [0], "the sample_mult sampler shared by two runs"
    valid("last")


@gpu
def test_a_top_p_run_without_a_candidate_fails_with_its_run(L):
    """top_p so small that (1 - top_p) / (n - 1) exceeds every probability of a flat row: the reference panics, the call names the run"""
    cfg = "mini-llama"
    img = S.build_image(cfg, S.Q8_0, seed=307)
    m = L.Transformer(img); b = L.Batch(m, 2)
    ok, none = L.Sampler(4096, 0.8, 1.0, 1), L.Sampler(4096, 1e6, 1e-6, 2)              # p = 1 / 4096 each, the cutoff 1 / 4095
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward_runs_sample: run 1: sample_topp: no candidate above the cutoff"):
        b.forward_runs_sample([(0, 0, [5], ok), (1, 0, [6, 7], none)])
    orc = O.Oracle(img)
    lg = orc.forward(5, 0).copy()
    assert int(b.forward_runs_sample([(0, 0, [5], ok)])[0]) == O.Sampler(4096, 0.8, 1.0, 1).sample(lg)


@gpu
def test_a_vocabulary_with_an_unwritten_tail_refuses_sampled_runs_only(L):
    """vocabulary 4098: the classifier writes 4096 logits.  A run sampled at a temperature is refused; argmax runs and runs without a sampler pass"""
    cfg = dataclasses.replace(S.CONFIGS["mini-llama"], name="mini-llama-v4098", vocab_size=4098)
    img = S.build_image(cfg, S.Q8_0, seed=308)
    m = L.Transformer(img); b = L.Batch(m, 2)
    orc = [O.Oracle(img), O.Oracle(img)]
    greedy, mult = L.Sampler(4098, 0.0, 0.9, 1), L.Sampler(4098, 0.8, 1.0, 2)
    with pytest.raises(L.LmrsError, match=r"lmrs_batch_forward_runs_sample: the classifier leaves the last vocab_size % 4 logits unwritten"):
        b.forward_runs_sample([(0, 0, [5], greedy), (1, 0, [6], mult)])
    got = b.forward_runs_sample([(0, 0, [5, 9], greedy), (1, 0, [6], None)])
    orc[0].forward(5, 0)
    assert got.tolist() == [ref_argmax(orc[0].forward(9, 1)), 0]
