"""lmrs_batch_generate_topp (include/lmrs_hip.h), the part that needs no GPU: the entry points in every layer with the header's argument lists, the host
program, the sampler's vector out and in (lmrs_sampler_candidates / lmrs_sampler_set_candidates), the rule the new kernels implement (tests/topp_rules.py)
against lmrs_sampler_topp_pairs on hand-made cases, the refusals that come before any device work, and the new kernels' resources in the BUILT code
object.  The device side is tests/test_batch_generate_topp.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import topp_rules as TR
from test_batch_generate_host import ARGS
from test_batch_mask_host import ROOT, _collector

NAME = "lmrs_batch_generate_topp"
NEW = {
    NAME: None,                                                # lmrs_batch_generate's sixteen
    "lmrs_sampler_candidates": ["s", "pairs", "ordered"],
    "lmrs_sampler_set_candidates": ["s", "pairs"],
    "lmrs_op_topp_rows": ["device", "n_rows", "n", "cand", "n0", "top_p", "rnd", "state", "token", "status"],
}
KERNELS = ("topp_sort_local_kernel", "topp_sort_global_kernel", "topp_rank_kernel", "topp_draw_kernel")
RND_MAX_SEED = 1574392                                         # random_f32 of this seed is 1 - 2^-24, the largest a sampler draws


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    lmrs_amd.build()
    return lmrs_amd


def header_args(header, name):
    cargs = [a.strip() for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1).split(",")]
    return cargs, [re.search(r"(\w+)$", a).group(1) for a in cargs]


def test_the_entry_points_exist_in_every_layer_with_the_headers_arguments(L):
    text = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    rs = re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read())
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name, names in NEW.items():
        assert hasattr(lib, name) and name in L.EXPORTS, name
        cargs, got = header_args(header, name)
        assert got == (ARGS if names is None else names), (name, got)
        assert len(getattr(L.lib(), name).argtypes) == len(got), name
    # the loop's new entry point: lmrs_batch_generate's list, name for name and type for type, in the header, ctypes, the C++ mirror and the Rust binding
    old, _ = header_args(header, "lmrs_batch_generate")
    new, _ = header_args(header, NAME)
    assert [re.sub(r"\s+", " ", a) for a in new] == [re.sub(r"\s+", " ", a) for a in old]
    assert L.lib().lmrs_batch_generate_topp.argtypes == L.lib().lmrs_batch_generate.argtypes
    assert re.search(r"#define\s+LMRS_FINISH_NO_CANDIDATE\s+2\b", header) and L.FINISH_NO_CANDIDATE == 2
    assert re.search(r"enum\s*\{\s*LMRS_FINISH_BUDGET\s*=\s*0\s*,\s*LMRS_FINISH_STOP\s*=\s*1\s*\}", header), "the enum stays as it is"
    assert NAME + "(" in hpp and "generate_topp(" in hpp and "FINISH_NO_CANDIDATE" in hpp
    fn = lambda n: [re.sub(r"\s+", " ", a.strip()) for a in re.search(r"pub\s+fn\s+" + n + r"\s*\((.*?)\)\s*->\s*c_int\s*;", rs, flags=re.S).group(1).split(",")]
    assert fn(NAME) == fn("lmrs_batch_generate")
    assert re.search(r"pub\s+fn\s+generate_topp\s*\(", rs) and re.search(r"pub\s+const\s+FINISH_NO_CANDIDATE\s*:\s*u32\s*=\s*2\s*;", rs)
    assert callable(L.Batch.generate_topp) and callable(L.Sampler.candidates) and callable(L.Sampler.set_candidates) and callable(L.op_topp_rows)
    import inspect
    pub = lambda f: [p for p in inspect.signature(f).parameters.values() if not p.name.startswith("_")]
    assert pub(L.Batch.generate_topp) == pub(L.Batch.generate), "Batch.generate_topp takes what Batch.generate takes"
    # the header's two older paragraphs name the call that now is that loop
    doc = text[text.index("lmrs_batch_forward with a sampler per row"):text.index("int lmrs_batch_forward_sample(")]
    assert NAME in doc and "top-p" in doc
    doc = text[text.index("int lmrs_batch_forward_sample("):text.index("int lmrs_batch_forward_runs_sample(")]
    assert NAME in doc


def test_the_host_program_still_compiles_and_takes_top_p():
    src = os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_generate.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(src).read()
    assert '"--top-p"' in text and "generate_topp(" in text


# ---------------------------------------------------------------------------------------------- the vector out and in

def test_export_and_import_continue_exactly(L):
    V, k, m = 300, 5, 6
    rng = np.random.default_rng(41)
    rows = (rng.standard_normal((k + m, V)) * 3).astype(np.float32)
    a = L.Sampler(V, 1.3, 0.9, 7)
    fresh, ordered = a.candidates()
    assert ordered and fresh.dtype == TR.PAIR and not fresh.view(np.uint64).any(), "a new sampler's vector is all zero and ordered"
    for r in rows[:k]:
        a.sample(r.copy())
    vec, ordered = a.candidates()
    assert ordered and vec.view(np.uint64).any()
    assert np.all(np.diff(vec["prob"]) <= 0), "the vector a call leaves is in descending order"
    b = L.Sampler(V, 1.3, 0.9, 7)
    b.set_candidates(vec)
    assert b.candidates()[1] and b.candidates()[0].tobytes() == vec.tobytes()
    c = L.Sampler(V, 1.3, 0.9, 7)                              # a sampler without the import: the stale entries matter to what follows
    differs = False
    for r in rows[k:]:
        ta, tb, tc = a.sample(r.copy()), b.sample(r.copy()), c.sample(r.copy())
        assert ta == tb and a.candidates()[0].tobytes() == b.candidates()[0].tobytes()
        differs = differs or ta != tc or a.candidates()[0].tobytes() != c.candidates()[0].tobytes()
    assert differs, "the imported state changed nothing: the case is vacuous"


def test_an_unordered_import_is_flagged_and_still_samples_as_written(L):
    V = 64
    rng = np.random.default_rng(42)
    vec = TR.pairs(np.sort(rng.random(V).astype(np.float32))[::-1] * np.float32(0.01), rng.permutation(V))
    s = L.Sampler(V, 1.0, 0.9, 3)
    s.set_candidates(vec)
    assert s.candidates()[1]
    bad = vec.copy(); bad[[10, 40]] = bad[[40, 10]]
    s.set_candidates(bad)
    got, ordered = s.candidates()
    assert not ordered and got.tobytes() == bad.tobytes()
    nan = vec.copy(); nan["prob"][5] = np.nan
    s.set_candidates(nan)
    assert not s.candidates()[1]
    # equal neighbours are in order
    flat = vec.copy(); flat["prob"][:] = np.float32(0.001)
    s.set_candidates(flat)
    assert s.candidates()[1]
    # an unordered vector: the whole vector is sorted, as sampler.rs:81 writes it - the stable sort of candidates + stale rest
    s.set_candidates(bad)
    cand = TR.pairs(np.float32([0.3, 0.2]), [4, 9])
    tok, new = TR.host_step(L, s, cand, 2)
    whole = np.concatenate([cand, bad[2:]])
    want = whole[np.argsort(-whole["prob"].astype(np.float64), kind="stable")]
    assert new.tobytes() == want.tobytes() and tok == TR.cut_and_draw(want, 2, 0.9, s.info()[3])
    with pytest.raises(L.LmrsError, match="vocab_size = 64 entries, 63 were given"):
        s.set_candidates(vec[:63])


def test_set_candidates_between_prepare_and_finish_is_refused(L):
    V = 32
    lib = L.lib()
    s = L.Sampler(V, 1.0, 0.9, 3)
    exps = np.exp(np.linspace(-3, 0, V)).astype(np.float32)
    vec = s.candidates()[0]
    assert lib.lmrs_sampler_exps_prepare(s._h, exps.ctypes.data_as(ctypes.c_void_p), None, None, None) == 0
    with pytest.raises(L.LmrsError, match="lmrs_sampler_set_candidates: between lmrs_sampler_exps_prepare and lmrs_sampler_exps_finish"):
        s.set_candidates(vec)
    nxt = ctypes.c_uint32()
    assert lib.lmrs_sampler_exps_finish(s._h, exps.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(nxt)) == 0
    s.set_candidates(vec)                                      # ... and taken again behind the finish
    assert lib.lmrs_sampler_candidates(None, vec.ctypes.data_as(ctypes.c_void_p), None) != 0
    assert lib.lmrs_sampler_set_candidates(s._h, None) != 0 and lib.lmrs_last_error().decode().startswith("lmrs_sampler_set_candidates: NULL argument")


# ---------------------------------------------------------------------------------------------- the rule against the host sampler

TINY = np.float32(2.0 ** -149)                                 # the smallest subnormal


def hand_cases():
    """(name, n, top_p, seed, [(candidates in index order, n0) per chained step], the vector to start from or None)"""
    P = lambda *v: np.float32(v)
    stale = TR.pairs(P(0.5, 0.4, 0.25, 0.25, 0.125, 0.0625, 0.0, 0.0), [7, 6, 5, 4, 3, 2, 1, 0])
    return [
        ("n0 = 1", 8, 0.9, 5, [(TR.pairs(P(0.75), [3]), 1), (TR.pairs(P(0.5), [6]), 1), (TR.pairs(P(0.75), [1]), 1)], None),
        ("n0 = n", 8, 0.7, 6, [(TR.pairs(P(.1, .2, .05, .3, .05, .1, .15, .05), range(8)), 8), (TR.pairs(P(.2, .1, .3, .05, .05, .1, .05, .15), range(8)), 8)], None),
        ("stale entries larger than every candidate", 8, 0.5, 7, [(TR.pairs(P(0.0625, 0.03125), [1, 5]), 2), (TR.pairs(P(0.015625), [2]), 1)], stale),
        ("a stale probability equal to a candidate's", 8, 0.6, 8, [(TR.pairs(P(0.25, 0.125, 0.25), [0, 1, 2]), 3), (TR.pairs(P(0.125, 0.25), [6, 7]), 2)], stale),
        ("equal candidates", 8, 0.8, 9, [(TR.pairs(P(0.125, 0.125, 0.125, 0.125, 0.125), [1, 2, 4, 6, 7]), 5), (TR.pairs(P(0.125, 0.125), [0, 5]), 2)], None),
        # r = rnd * cumulative < cumulative = the last cdf whenever the product is not rounded up to it: only the largest rnd over subnormal sums gets there
        ("the last_idx exit: r >= cdf for every entry", 8, 0.99, RND_MAX_SEED, [(TR.pairs(P(TINY, TINY), [2, 5]), 2), (TR.pairs(P(TINY), [4]), 1)], None),
        ("n0 = 0", 8, 0.9, 5, [(TR.pairs(P(0.5, 0.25), [2, 3]), 2), (TR.pairs(P(), []), 0), (TR.pairs(P(0.25), [1]), 1)], None),
        ("n0 = 0 at the first step", 8, 0.9, 5, [(TR.pairs(P(), []), 0), (TR.pairs(P(0.25), [1]), 1)], stale),
    ]


def test_the_rule_against_the_host_sampler_on_hand_made_cases(L):
    for name, n, top_p, seed, steps, start in hand_cases():
        s = L.Sampler(n, 1.0, top_p, seed)
        if start is not None:
            s.set_candidates(start)
        rnd = s.info()[3]
        state = s0 = s.candidates()[0]
        toks = []
        for k, (cand, n0) in enumerate(steps):
            tok, new = TR.step(cand, n0, state, top_p, rnd)
            htok, hnew = TR.host_step(L, s, cand, n0)
            assert tok == htok and new.tobytes() == hnew.tobytes(), f"{name}, step {k}: {tok} {new} vs {htok} {hnew}"
            assert (tok is None) == (n0 == 0) and (n0 or new.tobytes() == state.tobytes()), name
            assert np.all(np.diff(new["prob"]) <= 0)
            state = new; toks.append(tok)
        # what each case is about, checked on its own numbers
        if name.startswith("stale entries larger"):
            first = TR.step(steps[0][0], 2, start, top_p, rnd)[1]
            assert first["index"][:5].tolist() == [5, 4, 3, 1, 2] and toks[0] in (5, 4), "the cut and the draw run over stale entries that lie above every candidate"
        if name.startswith("a stale probability equal"):
            first = TR.step(steps[0][0], 3, start, top_p, rnd)[1]
            assert first["index"][:5].tolist() == [0, 2, 4, 1, 3], "equal probabilities: candidates (index order) before the stale entry, then by position"
        if name.startswith("the last_idx exit"):
            assert rnd == np.float32(1.0) - np.float32(2.0 ** -24)
            new = TR.step(steps[0][0], 2, s0, top_p, rnd)[1]
            cum = TR.chain(new["prob"][:2])
            assert cum[-1] > 0 and not np.any(np.float32(rnd) * cum[-1] < cum) and toks[0] == int(new["index"][1]) == 5, "no entry passes r < cdf: the token is the one at last_idx"


def test_the_rule_against_the_host_sampler_on_random_chains(L):
    rng = np.random.default_rng(43)
    for case in range(40):
        n = int(rng.integers(2, 200))
        top_p = float(rng.choice([0.05, 0.5, 0.9, 0.999]))
        s = L.Sampler(n, 1.0, top_p, int(rng.integers(1, 1 << 30)))
        rnd, state = s.info()[3], s.candidates()[0]
        for k in range(4):
            n0 = int(rng.choice([0, 1, 2, n // 2, n - 1, n, int(rng.integers(0, n + 1))]))
            idx = np.sort(rng.choice(n, n0, replace=False))
            prob = (rng.integers(1, 6, n0) / np.float32(8 * max(n0, 1))).astype(np.float32)          # few distinct values: ties among candidates and with stale ones
            cand = TR.pairs(prob, idx)
            tok, new = TR.step(cand, n0, state, top_p, rnd)
            htok, hnew = TR.host_step(L, s, cand, n0)
            assert tok == htok and new.tobytes() == hnew.tobytes(), (case, k, n, n0)
            state = new


# ---------------------------------------------------------------------------------------------- refusals, resources

def test_refusals_that_need_no_device(L):
    lib = L.lib()
    a = np.zeros(4, np.uint32)
    p = a.ctypes.data_as(ctypes.c_void_p)
    assert lib.lmrs_batch_generate_topp(None, 1, p, p, p, p, None, None, None, 1, p, None, p, p, None, None) != 0
    assert lib.lmrs_last_error().decode().startswith(NAME + ": NULL argument (the batch)"), lib.lmrs_last_error().decode()
    b = L.Batch.__new__(L.Batch)                               # no handle: a call that reached the library is refused as NULL
    b._h, b.model = None, None
    with pytest.raises(L.LmrsError, match="max_new must be a scalar or hold one budget per row"):
        b.generate_topp([0, 1], [1, 2], [0, 0], [3])
    with pytest.raises(L.LmrsError, match="stop must be one list of tokens, or one list of tokens per row"):
        b.generate_topp([0, 1], [1, 2], [0, 0], 3, stop=[[1], [2], [3]])
    with pytest.raises(L.LmrsError, match="samplers must have one entry per row"):
        b.generate_topp([0, 1], [1, 2], [0, 0], 3, samplers=[None])
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_generate_topp: NULL argument \(the batch\)"):
        b.generate_topp([0, 1], [1, 2], [0, 0], 3, stop=[7])
    with pytest.raises(L.LmrsError, match=r"^lmrs_batch_generate: NULL argument \(the batch\)"):
        b.generate([0, 1], [1, 2], [0, 0], 3, stop=[7])
    # lmrs_op_topp_rows: everything outside its ranges is refused before the device is touched
    c2 = np.zeros((1, 2), TR.PAIR)
    one, f = np.ones(1, np.uint32), np.float32([0.5])
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    call = lambda n_rows, n, n0: lib.lmrs_op_topp_rows(0, n_rows, n, ptr(c2), ptr(n0), ptr(f), ptr(f), ptr(c2), ptr(one), ptr(one))
    for n_rows, n, n0, msg in [(0, 2, one, "n_rows = 0 is outside 1 .. 64"), (65, 2, one, "n_rows = 65 is outside 1 .. 64"), (1, 1, one, "need 2 <= n <= 2^24"),
                               (1, (1 << 24) + 1, one, "need 2 <= n <= 2^24"), (1, 2, np.uint32([3]), "row 0: n0 = 3 exceeds n = 2")]:
        assert call(n_rows, n, n0) != 0 and lib.lmrs_last_error().decode() == "lmrs_op_topp_rows: " + msg, (msg, lib.lmrs_last_error().decode())
    assert lib.lmrs_op_topp_rows(0, 1, 2, None, ptr(one), ptr(f), ptr(f), ptr(c2), ptr(one), ptr(one)) != 0
    assert lib.lmrs_last_error().decode() == "lmrs_op_topp_rows: NULL argument"


def test_the_new_kernels_have_no_scratch_and_no_spills():
    KR = _collector()
    every = KR.collect(hot_only=False)
    got = {n: r for n, r in every.items() if any(k in n for k in KERNELS)}
    assert len(got) == 5, sorted(got)                          # the local sort kernel twice: the first sort of a block and a later stage's tail
    older = [n for n in every if n not in got]
    for name, g in got.items():
        assert not KR.HOT.match(name), f"{name} must not fall under the hot table's pattern"
        assert g["scratch"] == 0 and g["vgpr_spill"] == 0 and g["sgpr_spill"] == 0, f"{name}: scratch / spills: {g}"
        bare = re.sub(r"<.*", "", name.split("::")[-1])
        assert not any(re.sub(r"<.*", "", o.split("::")[-1]) in bare for o in older), f"{name} contains an older kernel's name"
