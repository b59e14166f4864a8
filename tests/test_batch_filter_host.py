"""Candidate filters on batch slots (lmrs_batch_set_filters / _clear_filters / _filter_info, lmrs_op_filter_rows), the part that needs no GPU: the rule's
numpy form (tests/filter_rules.py) against a naive full sort, the symbols, min_p_gap, the host program, the refusals that come before any device work, and
the kernel's resources in the BUILT code object against tests/golden/kernel_resources_filter.json.  The device side is tests/test_batch_filter.py."""
import ctypes
import functools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from filter_rules import INF, filtered
from test_batch_mask_host import GOLDEN, ROOT, _collector, _moved

NAMES = ("lmrs_batch_set_filters", "lmrs_batch_clear_filters", "lmrs_batch_filter_info", "lmrs_op_filter_rows")


def naive(row, top_k, min_gap):
    """the header's rule with the candidate order from a full comparison sort of (value, index) pairs, written without the kernels' keys"""
    row = np.asarray(row, np.float32)
    V = row.size

    def before(a, b):                                                                 # a, b: indices; < 0 when a comes first
        x, y = row[a], row[b]
        xn, yn = bool(np.isnan(x)), bool(np.isnan(y))
        if xn or yn:
            if xn and a == 0:
                return -1
            if yn and b == 0:
                return 1
            if xn != yn:
                return 1 if xn else -1
            return a - b
        if x != y:                                                                    # (-0.0 == +0.0)
            return -1 if x > y else 1
        return a - b
    cand = sorted(range(V), key=functools.cmp_to_key(before))
    out = row.copy()
    m = row[cand[0]]
    if top_k != 0 and top_k < V:
        for t in cand[top_k:]:
            out[t] = -INF
    if math.isfinite(float(min_gap)) and not np.isnan(m):
        thr = np.float32(m) - np.float32(min_gap)
        assert thr.dtype == np.float32
        for t in range(V):
            if not (out[t] >= thr):
                out[t] = -INF
    return out


@pytest.mark.parametrize("seed", range(6))
def test_filtered_is_the_rule_by_a_full_sort(seed):
    rng = np.random.default_rng(900 + seed)
    V = 97
    row = (rng.standard_normal(V) * 4).astype(np.float32)
    row[rng.integers(0, V, 20)] = np.float32(1.5)                                     # ties, broken by index
    row[rng.integers(0, V, 6)] = 0.0; row[rng.integers(1, V, 3)] = -0.0               # both zeros: equal
    row[rng.integers(1, V, 8)] = -INF
    row[5] = np.float32(-1e-40); row[6] = np.float32(1e-40); row[7] = np.float32(3e38)
    if seed == 4:
        row[11] = np.nan
    if seed == 5:
        row[0] = np.nan; row[13] = np.nan                                             # a NaN at index 0 is the first candidate: the gap step clears nothing
    finite = int(np.isfinite(row).sum())
    with np.errstate(all="ignore"):
        for top_k in (0, 1, 2, 5, finite - 1, finite, finite + 1, finite + 4, V - 1, V, V + 3):
            for gap in (INF, np.float32(0.0), np.float32(1e-30), np.float32(0.75), np.float32(3.0), np.float32(1e38)):
                got, want = filtered(row, top_k, gap), naive(row, top_k, gap)
                assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all(), (top_k, gap)
                kept = ~np.isneginf(got) | np.isneginf(row)
                assert (got[kept].view(np.uint32) == row[kept].view(np.uint32)).all(), "a kept logit changed"
                if 0 < top_k < V and gap == INF and seed < 4:                           # (no NaN in the row)
                    assert (~np.isneginf(got)).sum() == min(top_k, (~np.isneginf(row)).sum()), "top_k alone keeps top_k entries, or every entry that is not -inf"
                if top_k in (0, V, V + 3) and gap == INF:
                    assert (got.view(np.uint32) == row.view(np.uint32)).all(), "an inactive filter changed the row"
    # the first candidate stays whatever the parameters; all equal: the first top_k indices stay
    assert not np.isneginf(filtered(row, 1, 0.0)[np.argmax(np.nan_to_num(row, nan=-np.inf))]) or seed == 5
    flat = np.full(50, np.float32(2.0))
    assert np.flatnonzero(~np.isneginf(filtered(flat, 7))).tolist() == list(range(7))
    assert (filtered(flat, 0, 0.0) == flat).all()                                     # every value tied at thr stays


def test_the_four_symbols_are_declared_exported_and_listed():
    import lmrs_amd
    lmrs_amd.build()
    text = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(lmrs_amd.LIB_PATH)
    ffi = re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read())
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/lmrs_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in lmrs_amd.EXPORTS, f"{name} is not in lmrs_amd.EXPORTS"
        assert re.search(r"pub\s+fn\s+" + name + r"\s*\(", ffi), f"{name} is not declared in rust/lmrs-hip/src/batch.rs"
    for name in ("min_p_gap", "filter_rows"):
        assert callable(getattr(lmrs_amd, name, None)), f"lmrs_amd.{name} is missing"
    for name in ("set_filters", "clear_filters", "filter_info"):
        assert callable(getattr(lmrs_amd.Batch, name, None)), f"lmrs_amd.Batch.{name} is missing"
    # the header says that the log-probabilities are renormalised and that generate_greedy skips the launch
    assert "RENORMALISED over the kept set" in text and "lmrs_batch_generate_greedy SKIPS the launch" in text
    # the Rust declarations, argument for argument
    c = {"lmrs_batch*": "*mut LmrsBatch", "const lmrs_batch*": "*const LmrsBatch", "uint32_t": "u32", "size_t": "usize", "int": "c_int",
         "const uint32_t*": "*const u32", "uint32_t*": "*mut u32", "const float*": "*const f32", "float*": "*mut f32", "int*": "*mut c_int"}
    for name in NAMES:
        cargs = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        rargs = re.search(r"pub\s+fn\s+" + name + r"\s*\((.*?)\)\s*->\s*c_int\s*;", ffi, flags=re.S).group(1)
        ctypes_ = [re.sub(r"\s+", " ", re.match(r"(.*?)\w+$", a.strip()).group(1)).strip().replace(" *", "*") for a in cargs.split(",")]
        cnames = [re.search(r"(\w+)$", a.strip()).group(1) for a in cargs.split(",")]
        rtypes = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in rargs.split(",")]
        rnames = [a.split(":", 1)[0].strip() for a in rargs.split(",")]
        assert [c[t] for t in ctypes_] == rtypes and cnames == rnames, (name, ctypes_, rtypes, cnames, rnames)


def test_refusals_that_need_no_device():
    """a NULL batch is refused by name before anything else is looked at; lmrs_op_filter_rows refuses what lies outside its ranges before it touches a device"""
    import lmrs_amd
    lib = lmrs_amd.lib()
    u, f, i = ctypes.c_uint32(), ctypes.c_float(), ctypes.c_int()
    R = ctypes.byref
    for call, name in ((lambda: lib.lmrs_batch_set_filters(None, 0, None, None, None), NAMES[0]), (lambda: lib.lmrs_batch_clear_filters(None, 0, None), NAMES[1]),
                       (lambda: lib.lmrs_batch_filter_info(None, 0, R(u), R(f), R(i)), NAMES[2])):
        assert call() != 0
        assert lib.lmrs_last_error().decode().startswith(name + ": NULL argument"), lib.lmrs_last_error().decode()
    rows, k, g = np.zeros((2, 8), np.float32), np.array([1, 1], np.uint32), np.array([1.0, np.nan], np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for call, msg in ((lambda: lib.lmrs_op_filter_rows(0, None, 2, 8, 8, p(k), p(g)), "NULL argument"),
                      (lambda: lib.lmrs_op_filter_rows(0, p(rows), 2, 8, 8, None, p(g)), "NULL argument"),
                      (lambda: lib.lmrs_op_filter_rows(0, p(rows), 0, 8, 8, p(k), p(g)), "n_rows = 0 is outside 1 .. 65535"),
                      (lambda: lib.lmrs_op_filter_rows(0, p(rows), 2, 0, 8, p(k), p(g)), "need 1 <= n <= ld <= 2^24"),
                      (lambda: lib.lmrs_op_filter_rows(0, p(rows), 2, 8, 7, p(k), p(g)), "need 1 <= n <= ld <= 2^24"),
                      (lambda: lib.lmrs_op_filter_rows(0, p(rows), 2, 8, 8, p(k), p(g)), "row 1: min_gap is NaN or negative"),
                      (lambda: lib.lmrs_op_filter_rows(0, p(rows), 1, 8, 8, p(k), p(np.array([-1.0], np.float32))), "row 0: min_gap is NaN or negative")):
        assert call() != 0
        assert lib.lmrs_last_error().decode() == "lmrs_op_filter_rows: " + msg, (msg, lib.lmrs_last_error().decode())


def test_the_wrappers_check_their_arguments_before_the_library_is_asked():
    import lmrs_amd
    b = lmrs_amd.Batch.__new__(lmrs_amd.Batch)                                        # no handle: a call that reached the library would be refused as NULL
    b._h, b.model = None, None
    with pytest.raises(lmrs_amd.LmrsError, match="min_gap must be a scalar or hold one value per slot"):
        b.set_filters([0, 1, 2], min_gap=[0.1, 0.2])
    with pytest.raises(lmrs_amd.LmrsError, match="top_k must be a scalar or hold one value per slot"):
        b.set_filters([0, 1], top_k=[1, 2, 3])
    with pytest.raises(lmrs_amd.LmrsError, match="top_k must hold whole numbers"):
        b.set_filters([0, 1], top_k=[1, 2.5])
    with pytest.raises(lmrs_amd.LmrsError, match="top_k must hold whole numbers"):
        b.set_filters([0], top_k=-1)
    with pytest.raises(lmrs_amd.LmrsError, match=r"top_k must hold whole numbers >= 0 and below 2\^32"):
        b.set_filters([0, 1], top_k=[5, 2 ** 32])
    with pytest.raises(lmrs_amd.LmrsError, match=r"^lmrs_batch_set_filters: NULL argument"):
        b.set_filters([0], top_k=40)
    with pytest.raises(lmrs_amd.LmrsError, match=r"^lmrs_batch_clear_filters: NULL argument"):
        b.clear_filters()
    with pytest.raises(lmrs_amd.LmrsError, match=r"^lmrs_batch_filter_info: NULL argument"):
        b.filter_info(0)


def test_min_p_gap_is_the_float64_formula_rounded_once():
    import lmrs_amd
    for min_p, t in ((0.05, 1.0), (0.05, 0.7), (0.1, 1.3), (1e-9, 2.0), (0.999, 0.01), (1.0, 1.0), (0.5, 0.0)):
        got = lmrs_amd.min_p_gap(min_p, t)
        want = np.float32(-np.float64(t) * np.log(np.float64(min_p)))
        assert isinstance(got, np.float32) and got.tobytes() == np.float32(want + 0.0).tobytes(), (min_p, t, got, want)
        assert got >= 0 and not np.signbit(got)
        # what it means: a token whose probability is min_p times the largest lies min_gap below it in logit space
        if t > 0:
            assert math.isclose(math.exp(-float(got) / t), min_p, rel_tol=1e-6)
    assert lmrs_amd.min_p_gap(0.0, 1.0) == np.inf
    for bad in ((1.5, 1.0), (0.5, -1.0), (float("nan"), 1.0)):
        with pytest.raises(lmrs_amd.LmrsError, match="min_p must lie in"):
            lmrs_amd.min_p_gap(*bad)


def test_batch_filter_program_and_host_mirror_compile():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_filter.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_filter.cpp")).read()
    for opt in ("--top-k", "--min-p", "--temperature"):
        assert f'"{opt}"' in src, f"batch_filter.cpp does not take {opt}"
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name in NAMES:
        assert name + "(" in hpp, f"transformer.hpp's Batch does not call {name}"


def test_filter_kernel_resources():
    KR = _collector()
    got = {n: r for n, r in KR.collect(hot_only=False).items() if "filter_rows_kernel" in n}
    want = json.load(open(os.path.join(GOLDEN, "kernel_resources_filter.json")))
    assert len(got) == 1 and set(got) == set(want), f"kernel classes added / removed: {sorted(set(got) ^ set(want))}"
    for name, g in got.items():
        assert not KR.HOT.match(name), f"{name} must not fall under the hot table's pattern"
        assert g["scratch"] == 0 and g["vgpr_spill"] == 0 and g["sgpr_spill"] == 0, f"{name}: scratch / spills: {g}"
        assert g["lds_static"] <= 2048, f"{name}: the select's bins and partial sums are about 1 KB of LDS: {g}"
    assert not _moved(got, want), "the filter kernel's resources moved:\n  " + "\n  ".join(_moved(got, want))
    hot = KR.collect(hot_only=True)
    assert not [n for n in hot if "filter_rows_kernel" in n], "the filter kernel must not be read as a hot class"
