"""lmrs_batch_generate (include/lmrs_hip.h), the part that needs no GPU: the entry point in every layer with the header's argument list, the host program,
the stop rule's reference (tests/test_batch_generate.py's ref_generate) against a naive loop over hand-written sequences, the refusals that come before
any device work, and the new kernels' resources in the BUILT code object.  The device side is tests/test_batch_generate.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_batch_generate import BUDGET, STOP, ref_generate, rounds
from test_batch_mask_host import ROOT, _collector

NAME = "lmrs_batch_generate"
KERNELS = ("gen_advance_kernel", "gen_logprobs_kernel")
ARGS = ["b", "n", "slot", "tokens", "pos", "max_new", "n_stop", "stop_tokens", "samplers", "check_every", "out_tokens", "out_logprobs", "n_out", "finish",
        "stats2", "seconds"]


def naive(seq, budget, stop):
    """the contract read off a whole sequence of choices: the first index that holds a stop token, else the budget's last"""
    for j, o in enumerate(seq[:budget]):
        if o in stop:
            return seq[:j + 1], STOP
    return seq[:budget], BUDGET


def test_the_stop_rule_against_a_naive_loop():
    seq = [5, 9, 5, 7, 3, 3, 8, 1]
    cases = [(1, []), (1, [5]), (2, [9]), (3, [7]), (4, [7]), (8, []), (8, [3]), (8, [1]), (8, [2, 4, 6]), (5, [3, 7]), (4, [3]), (8, [8, 5])]
    for budget, stop in cases:
        it, fed = iter(seq), []

        def step(t):
            fed.append(t)
            return next(it)
        got = ref_generate(step, 100, budget, set(stop))
        want = naive(seq, budget, set(stop))
        assert got == want, (budget, stop, got, want)
        # the first token fed is the row's own, every later one the choice before it; the stop token is reported and never fed
        assert fed == [100] + want[0][:-1], (budget, stop, fed)
    assert ref_generate(lambda t: 5, 5, 1, {5}) == ([5], STOP), "STOP wins over BUDGET"
    assert [rounds(k, 3) for k in (1, 3, 4, 12)] == [3, 3, 6, 12] and rounds(5, 1) == 5 and rounds(5, 16) == 16


def test_the_entry_point_exists_in_every_layer_with_the_headers_arguments():
    import lmrs_amd
    lmrs_amd.build()
    text = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(lmrs_amd.LIB_PATH)
    rs = re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read())
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    assert hasattr(lib, NAME) and NAME in lmrs_amd.EXPORTS and NAME + "(" in hpp and callable(lmrs_amd.Batch.generate)
    assert re.search(r"#define\s+LMRS_STOP_MAX\s+16\b", header) and lmrs_amd.STOP_MAX == 16
    assert re.search(r"enum\s*\{\s*LMRS_FINISH_BUDGET\s*=\s*0\s*,\s*LMRS_FINISH_STOP\s*=\s*1\s*\}", header)
    assert (lmrs_amd.FINISH_BUDGET, lmrs_amd.FINISH_STOP) == (BUDGET, STOP) == (0, 1)
    cargs = [a.strip() for a in re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1).split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in cargs] == ARGS
    ctypes_ = [re.sub(r"\s*\*\s*", "*", re.sub(r"\s+", " ", re.match(r"(.*?)\w+$", a).group(1)).strip()) for a in cargs]
    c = {"lmrs_batch*": "*mut LmrsBatch", "uint32_t": "u32", "const uint32_t*": "*const u32", "uint32_t*": "*mut u32", "float*": "*mut f32",
         "lmrs_sampler*const*": "*const *mut LmrsSampler", "uint64_t*": "*mut u64", "double*": "*mut f64"}
    rargs = re.search(r"pub\s+fn\s+" + NAME + r"\s*\((.*?)\)\s*->\s*c_int\s*;", rs, flags=re.S).group(1)
    rnames = [a.split(":", 1)[0].strip() for a in rargs.split(",")]
    rtypes = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in rargs.split(",")]
    assert rnames == ARGS and [c[t] for t in ctypes_] == rtypes, (ctypes_, rtypes)
    assert re.search(r"pub\s+fn\s+generate\s*\(", rs), "batch.rs has no Batch::generate"
    # the ctypes signature: one entry per argument, pointers and the two scalars where the header has them
    at = lmrs_amd.lib().lmrs_batch_generate.argtypes
    assert len(at) == len(ARGS) and at[1] is ctypes.c_uint32 and at[9] is ctypes.c_uint32 and at[15] == ctypes.POINTER(ctypes.c_double)
    assert all(at[k] is ctypes.c_void_p for k in (0, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14))
    # the header says what exists now and what still does not
    doc = text[text.index("lmrs_batch_forward with a sampler per row"):text.index("int lmrs_batch_forward_sample(")]
    assert "lmrs_batch_generate" in doc and "top-p" in doc


def test_batch_generate_program_and_host_mirror_compile():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_generate.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_refusals_that_need_no_device():
    import lmrs_amd
    lib = lmrs_amd.lib()
    a = np.zeros(4, np.uint32)
    p = a.ctypes.data_as(ctypes.c_void_p)
    assert lib.lmrs_batch_generate(None, 1, p, p, p, p, None, None, None, 1, p, None, p, p, None, None) != 0
    assert lib.lmrs_last_error().decode().startswith(NAME + ": NULL argument (the batch)"), lib.lmrs_last_error().decode()
    b = lmrs_amd.Batch.__new__(lmrs_amd.Batch)                                        # no handle: a call that reached the library is refused as NULL
    b._h, b.model = None, None
    with pytest.raises(lmrs_amd.LmrsError, match="max_new must be a scalar or hold one budget per row"):
        b.generate([0, 1], [1, 2], [0, 0], [3])
    with pytest.raises(lmrs_amd.LmrsError, match="stop must be one list of tokens, or one list of tokens per row"):
        b.generate([0, 1], [1, 2], [0, 0], 3, stop=[[1], [2], [3]])
    with pytest.raises(lmrs_amd.LmrsError, match="samplers must have one entry per row"):
        b.generate([0, 1], [1, 2], [0, 0], 3, samplers=[None])
    with pytest.raises(lmrs_amd.LmrsError, match=r"^lmrs_batch_generate: NULL argument \(the batch\)"):
        b.generate([0, 1], [1, 2], [0, 0], 3, stop=[7])


def test_the_new_kernels_have_no_scratch_and_no_spills():
    KR = _collector()
    got = {n: r for n, r in KR.collect(hot_only=False).items() if any(k in n for k in KERNELS)}
    assert len(got) == 2, sorted(got)
    for name, g in got.items():
        assert not KR.HOT.match(name), f"{name} must not fall under the hot table's pattern"
        assert g["scratch"] == 0 and g["vgpr_spill"] == 0 and g["sgpr_spill"] == 0, f"{name}: scratch / spills: {g}"
