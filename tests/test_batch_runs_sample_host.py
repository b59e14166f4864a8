"""The host side of lmrs_batch_forward_runs_sample and lmrs_op_sort_candidates, no GPU: the two names in every layer, the example's syntax, and the
resources of the new kernels - the flat rows' common sort - in the built library, pinned in tests/golden/kernel_resources_cand_sort.json with the rules
of tests/test_batch_wide_host.py."""
import inspect
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lmrs_batch_forward_runs_sample", "lmrs_op_sort_candidates")
NEW_KERNELS = r"cand_sort_(keys|local|global|pairs)_kernel"
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_cand_sort.json")


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    lmrs_amd.build()
    return lmrs_amd


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_entry_points_exist_in_every_layer(L):
    lib = L.lib()
    header = read("include", "lmrs_hip.h")
    rust = read("rust", "lmrs-hip", "src", "ffi.rs") + read("rust", "lmrs-hip", "src", "batch.rs")
    hpp = read("lm.rs_amd", "hostcpp", "transformer.hpp")
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in L.EXPORTS
        assert re.search(rf"\bint\s+{name}\(", header), f"{name} is not declared in the header"
        assert re.search(rf"\bpub fn {name}\(", rust), f"{name} is not declared in the Rust crate"
        assert name in hpp, f"{name} is not mirrored in transformer.hpp"
    assert callable(L.Batch.forward_runs_sample) and list(inspect.signature(L.Batch.forward_runs_sample).parameters) == ["self", "runs"]
    assert callable(L.op_sort_candidates) and L.PAIR.itemsize == 8
    assert "pub fn forward_runs_sample(" in read("rust", "lmrs-hip", "src", "batch.rs")
    assert "forward_runs_sample(const std::vector<SampledRun>& runs)" in hpp
    # the header says what the call allocates and that the older call is left alone
    doc = header[header.index("lmrs_batch_forward_runs with a sampler per run"):header.index("int lmrs_batch_forward_runs_sample(")]
    assert "ONE second synchronise" in doc and "lmrs_batch_forward_sample's buffers are not touched" in doc


def test_rust_externs_of_the_new_entry_points_match_the_header():
    """(the call is declared in batch.rs beside its caller, as lmrs_batch_forward_sample is: ffi.rs's batch block is pinned to the greedy entry points;
    the hook stands beside lmrs_op_sample_rows in ffi.rs's first block)"""
    from test_rust_crate import CMAP, c_prototypes
    cmap = dict(CMAP)
    cmap.update({"lmrs_batch*": "*mut LmrsBatch", "lmrs_sampler* const*": "*const *mut LmrsSampler", "lmrs_sampler*const*": "*const *mut LmrsSampler"})
    c = c_prototypes()
    src = {f: re.sub(r"//[^\n]*", " ", read("rust", "lmrs-hip", "src", f)) for f in ("ffi.rs", "batch.rs")}
    blocks = re.findall(r'extern\s+"C"\s*\{(.*?)\n\}', src["ffi.rs"], flags=re.S)
    assert "lmrs_op_sort_candidates" in blocks[0] and "lmrs_op_sample_rows" in blocks[0]
    assert "lmrs_batch_forward_runs_sample" not in src["ffi.rs"]
    for name in NAMES:
        where = "ffi.rs" if name == "lmrs_op_sort_candidates" else "batch.rs"
        m = re.search(rf"pub\s+fn\s+{name}\s*\((.*?)\)\s*->\s*c_int\s*;", src[where], flags=re.S)
        assert m, f"{name} is not declared in {where}"
        rargs = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in m.group(1).split(",") if a.strip()]
        cret, cargs = c[name]
        assert cret == "int" and len(cargs) == len(rargs), f"{name}: {cargs} vs {rargs}"
        for i, (ca, ra) in enumerate(zip(cargs, rargs)):
            assert cmap[ca] == ra, f"{name}: argument {i} is {ra} in Rust, {ca} in C"


def test_batch_sample_example_passes_the_syntax_check():
    src = os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_sample.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    txt = open(src).read()
    assert "--wide" in txt and "Batch batch(model, n, wide)" in txt and "forward_runs_sample(runs)" in txt


def test_new_kernels_are_not_hot_names():
    from tools import kernel_resources as KR
    others = (r"batch_sample_(scale_max|exp|chain|div|pairs)_kernel", r"gemm_stream_kernel|runs_advance_kernel", r"rope_scatter_runs_kernel|attention_runs_kernel|select_rows_kernel",
              r"rope_scatter_rows_kernel|attention_table_kernel|table_advance_kernel")
    for n in ("lmrs::cand_sort_keys_kernel", "lmrs::cand_sort_local_kernel<false>", "lmrs::cand_sort_local_kernel<true>", "lmrs::cand_sort_global_kernel",
              "lmrs::cand_sort_pairs_kernel"):
        assert not KR.HOT.match(n) and re.search(NEW_KERNELS, n)
        assert not any(re.search(o, n) for o in others), f"{n} would enter another test's table"


def test_new_kernel_resources():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    got = {n: r for n, r in rows.items() if re.search(NEW_KERNELS, n)}
    want = json.load(open(TABLE))
    # the keys, the local network as the block sort and as a stage's tail, the global step, the pairs
    assert len(got) == 5 and set(got) == set(want), f"kernel classes added / removed: {sorted(set(got) ^ set(want))}"
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
    assert not bad, "the common sort's kernel resources moved:\n  " + "\n  ".join(bad)
    # the one-row sort's kernels were left alone: still there, beside the new ones
    for n in ("lmrs::sample_keys_kernel", "lmrs::sample_bitonic_local_kernel<false>", "lmrs::sample_bitonic_local_kernel<true>", "lmrs::sample_bitonic_global_kernel"):
        assert n in rows, n
