"""Penalties over a batch's token record (lmrs_batch_set_penalties / _clear_penalties / _penalty_info / _set_history / _history), the part that needs no
GPU: the rule's numpy form (tests/penalty_rules.py) against a naive per-token loop, the symbols, the host program, the refusals that come before any device
work, and the two kernels' resources in the BUILT code object against tests/golden/kernel_resources_penalty.json.  The device side is
tests/test_batch_penalty.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from penalty_rules import KINDS, NONE, params, penalised
from test_batch_mask_host import GOLDEN, ROOT, _collector, _moved

NAMES = ("lmrs_batch_set_history", "lmrs_batch_history", "lmrs_batch_set_penalties", "lmrs_batch_clear_penalties", "lmrs_batch_penalty_info")
KERNELS = ("penalty_rows_kernel", "record_rows_kernel")


def naive(row, history, p, par):
    """the rule token by token over the whole vocabulary: counts by scanning the record for every token"""
    out = np.asarray(row, np.float32).copy()
    rep, pres, freq = np.float32(par["repetition"]), np.float32(par["presence"]), np.float32(par["frequency"])
    seen = [(i, int(t)) for i, t in enumerate(history[:p + 1]) if int(t) != NONE]
    with np.errstate(all="ignore"):
        for t in range(out.size):
            c_all = sum(1 for _, x in seen if x == t)
            c_out = sum(1 for i, x in seen if x == t and i >= par["out_from"])
            if c_all > 0 and rep != np.float32(1.0):
                out[t] = out[t] / rep if out[t] > 0 else out[t] * rep
            if c_out > 0:
                out[t] = (out[t] - freq * np.float32(c_out)) - pres
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("seed", range(6))
def test_penalised_is_the_rule_token_by_token(seed):
    rng = np.random.default_rng(700 + seed)
    V, n = 97, 60
    row = (rng.standard_normal(V) * 8).astype(np.float32)
    row[rng.integers(0, V, 9)] = 0.0                                                   # l == 0 takes the product
    row[3] = -0.0; row[5] = np.float32(-1e-30); row[7] = np.float32(3e38)
    hist = rng.integers(0, 20, n).astype(np.uint32)                                   # a small alphabet: counts above 1
    hist[[3, 5, 7][seed % 3]] = 3; hist[11] = 5; hist[12] = 7
    hist[rng.integers(0, n, 8)] = NONE
    for kind in list(KINDS) + ["neg"]:
        for p in (0, 1, 17, n - 1):
            for out_from in (0, 3, p, p + 1, n + 5):                                  # out_from beyond p: nothing counts as output
                par = dict(repetition=0.6, presence=-0.3, frequency=-1.1, out_from=out_from) if kind == "neg" else params(kind, out_from=out_from)
                got, want = penalised(row, hist, p, par), naive(row, hist, p, par)
                assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all(), (kind, p, out_from)
                untouched = np.setdiff1d(np.arange(V), hist[:p + 1][hist[:p + 1] != NONE])
                assert (got[untouched].view(np.uint32) == row[untouched].view(np.uint32)).all(), "a logit outside the record changed"
                if out_from > p and par["repetition"] == 1.0:
                    assert (got.view(np.uint32) == row.view(np.uint32)).all()
    assert (penalised(row, hist, n - 1, None).view(np.uint32) == row.view(np.uint32)).all()
    all_none = np.full(n, NONE, np.uint32)
    assert (penalised(row, all_none, n - 1, params("all")).view(np.uint32) == row.view(np.uint32)).all()


def test_the_five_symbols_are_declared_exported_and_listed():
    import lmrs_amd
    lmrs_amd.build()
    text = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(lmrs_amd.LIB_PATH)
    # (declared beside the Rust wrapper, as every batch call since the first seven: ffi.rs's batch block is pinned to those by tests/test_batch.py)
    ffi = re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read())
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/lmrs_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in lmrs_amd.EXPORTS, f"{name} is not in lmrs_amd.EXPORTS"
        assert re.search(r"pub\s+fn\s+" + name + r"\s*\(", ffi), f"{name} is not declared in rust/lmrs-hip/src/batch.rs"
    assert re.search(r"#define\s+LMRS_TOKEN_NONE\s+0xFFFFFFFFu", header) and lmrs_amd.TOKEN_NONE == NONE == 0xFFFFFFFF
    # the Rust declarations, argument for argument (the crate's own test reads the first extern block only)
    c = {"lmrs_batch*": "*mut LmrsBatch", "const lmrs_batch*": "*const LmrsBatch", "uint32_t": "u32", "size_t": "usize", "const uint32_t*": "*const u32",
         "uint32_t*": "*mut u32", "const float*": "*const f32", "float*": "*mut f32", "int*": "*mut c_int"}
    for name in NAMES:
        cargs = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        rargs = re.search(r"pub\s+fn\s+" + name + r"\s*\((.*?)\)\s*->\s*c_int\s*;", ffi, flags=re.S).group(1)
        ctypes_ = [re.sub(r"\s+", " ", re.match(r"(.*?)\w+$", a.strip()).group(1)).strip().replace(" *", "*") for a in cargs.split(",")]
        rtypes = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in rargs.split(",")]
        assert [c[t] for t in ctypes_] == rtypes, (name, ctypes_, rtypes)


def test_refusals_that_need_no_device():
    """a NULL batch is refused by name before anything else is looked at"""
    import lmrs_amd
    lib = lmrs_amd.lib()
    f, u, i = ctypes.c_float(), ctypes.c_uint32(), ctypes.c_int()
    R = ctypes.byref
    for call, name in ((lambda: lib.lmrs_batch_set_history(None, 0, 0, None, 0), NAMES[0]), (lambda: lib.lmrs_batch_history(None, 0, 0, 0, None), NAMES[1]),
                       (lambda: lib.lmrs_batch_set_penalties(None, 0, None, None, None, None, None), NAMES[2]),
                       (lambda: lib.lmrs_batch_clear_penalties(None, 0, None), NAMES[3]),
                       (lambda: lib.lmrs_batch_penalty_info(None, 0, R(f), R(f), R(f), R(u), R(i)), NAMES[4])):
        assert call() != 0
        assert lib.lmrs_last_error().decode().startswith(name + ": NULL argument"), lib.lmrs_last_error().decode()


def test_the_wrappers_check_their_arguments_before_the_library_is_asked():
    import lmrs_amd
    b = lmrs_amd.Batch.__new__(lmrs_amd.Batch)                                        # no handle: a call that reached the library would be refused as NULL
    b._h, b.model = None, None
    with pytest.raises(lmrs_amd.LmrsError, match="presence must be a scalar or hold one value per slot"):
        b.set_penalties([0, 1, 2], presence=[0.1, 0.2])
    with pytest.raises(lmrs_amd.LmrsError, match="out_from must hold whole numbers"):
        b.set_penalties([0, 1], out_from=[1, 2.5])
    with pytest.raises(lmrs_amd.LmrsError, match="n must not be negative"):
        b.history(0, -1)
    with pytest.raises(lmrs_amd.LmrsError, match=r"^lmrs_batch_set_penalties: NULL argument"):
        b.set_penalties([0], repetition=1.3)


def test_batch_penalty_program_and_host_mirror_compile():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_penalty.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name in NAMES:
        assert name + "(" in hpp, f"transformer.hpp's Batch does not call {name}"


def test_penalty_kernels_resources():
    KR = _collector()
    got = {n: r for n, r in KR.collect(hot_only=False).items() if any(k in n for k in KERNELS)}
    want = json.load(open(os.path.join(GOLDEN, "kernel_resources_penalty.json")))
    assert len(got) == 2 and set(got) == set(want), f"kernel classes added / removed: {sorted(set(got) ^ set(want))}"
    for name, g in got.items():
        assert not KR.HOT.match(name), f"{name} must not fall under the hot table's pattern"
        # (the sort's keys live in dynamic LDS, sized by the launch: no static LDS)
        assert g["scratch"] == 0 and g["vgpr_spill"] == 0 and g["sgpr_spill"] == 0 and g["lds_static"] == 0, f"{name}: scratch / spills / LDS: {g}"
    assert not _moved(got, want), "the penalty kernels' resources moved:\n  " + "\n  ".join(_moved(got, want))
    hot = KR.collect(hot_only=True)
    assert not [n for n in hot if any(k in n for k in KERNELS)], "the penalty kernels must not be read as hot classes"
