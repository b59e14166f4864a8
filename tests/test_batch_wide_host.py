"""The host side of the wide batch (lmrs_batch_create_wide, lmrs_batch_width, lmrs_debug_gemm_wide), no GPU: the entry points in every layer, the
example's syntax, and the resources of the new kernels - the stream GEMM family and the long table's advance - in the built library, pinned in
tests/golden/kernel_resources_wide.json with the tolerances of tests/test_skinny_resources.py."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lmrs_batch_create_wide", "lmrs_batch_width", "lmrs_debug_gemm_wide")
NEW_KERNELS = r"gemm_stream_kernel|runs_advance_kernel"
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_wide.json")


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    lmrs_amd.build()
    return lmrs_amd


def test_entry_points_exist_in_every_layer(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    rust = "".join(open(os.path.join(ROOT, "rust", "lmrs-hip", "src", f)).read() for f in ("ffi.rs", "batch.rs"))
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in L.EXPORTS
        assert re.search(rf"\bint\s+{name}\(", header), f"{name} is not declared in the header"
        assert re.search(rf"\bpub fn {name}\(", rust), f"{name} is not declared in the Rust crate"
        assert name in hpp, f"{name} is not mirrored in transformer.hpp"
    assert callable(L.debug_gemm_wide) and isinstance(L.Batch.width, property)
    import inspect
    assert inspect.signature(L.Batch.__init__).parameters["wide"].default is False
    batch_rs = open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read()
    assert "pub fn new_wide(" in batch_rs and "pub fn width(" in batch_rs
    assert "width()" in hpp and "bool wide = false" in hpp


def test_rust_externs_of_the_new_entry_points_match_the_header():
    """(the batch block of ffi.rs is pinned to the greedy entry points by tests/test_batch.py, so the two batch calls are declared in batch.rs beside
    their callers, as lmrs_batch_forward_sample is; the hook stands beside lmrs_debug_gemm_skinny in ffi.rs's first block)"""
    from test_rust_crate import CMAP, c_prototypes
    cmap = dict(CMAP)
    cmap.update({"lmrs_batch*": "*mut LmrsBatch", "const lmrs_batch*": "*const LmrsBatch", "lmrs_batch**": "*mut *mut LmrsBatch", "lmrs_ctx*": "*mut ffi::LmrsCtx"})
    c = c_prototypes()
    src = {f: re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", f)).read()) for f in ("ffi.rs", "batch.rs")}
    blocks = re.findall(r'extern\s+"C"\s*\{(.*?)\n\}', src["ffi.rs"], flags=re.S)
    assert "lmrs_debug_gemm_wide" in blocks[0] and "lmrs_debug_gemm_skinny" in blocks[0]
    for name in NAMES:
        where = "ffi.rs" if name == "lmrs_debug_gemm_wide" else "batch.rs"
        m = re.search(rf"pub\s+fn\s+{name}\s*\((.*?)\)\s*->\s*c_int\s*;", src[where], flags=re.S)
        assert m, f"{name} is not declared in {where}"
        rargs = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in m.group(1).split(",") if a.strip()]
        cret, cargs = c[name]
        assert cret == "int" and len(cargs) == len(rargs), f"{name}: {cargs} vs {rargs}"
        for i, (ca, ra) in enumerate(zip(cargs, rargs)):
            want = cmap[ca] if where == "batch.rs" else CMAP[ca]
            assert want == ra, f"{name}: argument {i} is {ra} in Rust, {ca} in C"


def test_batch_greedy_example_passes_the_syntax_check():
    src = os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_greedy.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    txt = open(src).read()
    assert "--wide" in txt and "Batch batch(model, n, wide)" in txt


def test_new_kernels_are_not_hot_names():
    from tools import kernel_resources as KR
    for n in ("lmrs::gemm_stream_kernel<0, 4, 1, 8, false>", "lmrs::gemm_stream_kernel<5, 2, 2, 4, true>", "lmrs::runs_advance_kernel"):
        assert not KR.HOT.match(n) and "gemm_skinny_kernel" not in n


def test_new_kernel_resources():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    got = {n: r for n, r in rows.items() if re.search(NEW_KERNELS, n)}
    want = json.load(open(TABLE))
    # 5 epilogues x {2, 3, 4 token tiles} x {Q8_0, Q4_0} x {16-row tiles of 8 waves, 32-row tiles of 4 waves}, and the advance
    assert len(got) == 61 and set(got) == set(want), f"kernel classes added / removed: {sorted(set(got) ^ set(want))[:6]}"
    bad = []
    for name, w in want.items():
        g = got[name]
        if KR.HOT.match(name):
            bad.append(f"{name} must not enter the hot table")
        elif g["scratch"] != 0 or g["vgpr_spill"] != 0:
            bad.append(f"{name}: scratch {g['scratch']} bytes per lane, spilled VGPRs {g['vgpr_spill']}")
        elif g["waves_per_simd"] != w["waves_per_simd"]:
            bad.append(f"{name}: waves per SIMD {w['waves_per_simd']} -> {g['waves_per_simd']} (VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']})")
        elif abs(g["vgpr"] + g["agpr"] - w["vgpr"] - w["agpr"]) > 16:
            bad.append(f"{name}: VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']}")
    assert not bad, "wide-batch kernel resources moved:\n  " + "\n  ".join(bad)
