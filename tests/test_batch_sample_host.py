"""The host side of lmrs_batch_forward_sample, no GPU: lmrs_sampler_topp_sorted_pairs against the oracle's Sampler, the entry points in every layer,
the resources of the new kernels in the built library, the example's syntax."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lmrs_batch_forward_sample", "lmrs_op_sample_rows", "lmrs_sampler_topp_sorted_pairs")
NEW_KERNELS = r"batch_sample_(scale_max|exp|chain|div|pairs)_kernel"


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    lmrs_amd.build()
    return lmrs_amd


def test_topp_sorted_pairs_against_the_oracle_sampler(L):
    """40 calls on ONE sampler per side: the candidates of each call are filtered and sorted here in numpy by the device sort's key rule (prob descending,
    index ascending), the library merges them with the stale rest of its persistent vector (sampler.rs:81) - the oracle's tokens, call for call"""
    V, temp, top_p, seed = 1500, 0.9, 0.85, 4242
    dev, ref = L.Sampler(V, temp, top_p, seed), O.Sampler(V, temp, top_p, seed)
    rng = np.random.default_rng(3)
    cutoff = (np.float32(1.0) - np.float32(top_p)) / np.float32(V - 1)
    counts = []
    for k in range(40):
        lg = (rng.standard_normal(V) * [0.3, 1.0, 3.0, 8.0][k % 4]).astype(np.float32)           # flat to peaked: n0 goes up and down, entries go stale
        if k % 7 == 3:
            lg[rng.integers(0, V, 40)] = lg[5]                                                   # equal probabilities: the index decides
        want = ref.sample(lg)                                                                    # (lg: the probabilities now)
        idx = np.flatnonzero(lg >= cutoff).astype(np.uint32)
        prob = lg[idx]
        key = ((~prob.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
        order = np.argsort(key, kind="stable")
        counts.append(idx.size)
        assert dev.topp_sorted_pairs(prob[order], idx[order]) == want, f"call {k}: {idx.size} candidates"
    assert min(counts) < 50 and max(counts) > 500, counts                                        # stale entries did sit behind short calls


def test_topp_sorted_pairs_refusals(L):
    lib = L.lib()
    import ctypes
    nxt = ctypes.c_uint32()
    mult = L.Sampler(100, 0.8, 1.0, 1)
    assert lib.lmrs_sampler_topp_sorted_pairs(mult._h, None, 0, ctypes.byref(nxt)) != 0 and "not a top-p sampler" in lib.lmrs_last_error().decode()
    topp = L.Sampler(100, 0.8, 0.9, 1)
    assert lib.lmrs_sampler_topp_sorted_pairs(topp._h, None, 3, ctypes.byref(nxt)) != 0 and "NULL" in lib.lmrs_last_error().decode()
    assert lib.lmrs_sampler_topp_sorted_pairs(topp._h, None, 0, ctypes.byref(nxt)) != 0 and "no candidate above the cutoff" in lib.lmrs_last_error().decode()
    pairs = np.zeros(101, dtype=[("prob", np.float32), ("index", np.uint32)])
    assert lib.lmrs_sampler_topp_sorted_pairs(topp._h, pairs.ctypes.data, 101, ctypes.byref(nxt)) != 0 and "more candidates" in lib.lmrs_last_error().decode()


def test_entry_points_exist_in_every_layer(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "ffi.rs")).read() + open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read()
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read() + open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "text.hpp")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in L.EXPORTS
        assert re.search(rf"\bint\s+{name}\(", header), f"{name} is not declared in the header"
        assert re.search(rf"\bpub fn {name}\(", ffi), f"{name} is not declared in the Rust crate"
    assert "lmrs_batch_forward_sample" in hpp and "handle()" in hpp
    assert callable(L.Batch.forward_sample) and callable(L.op_sample_rows) and callable(L.Sampler.topp_sorted_pairs)
    assert "forward_sample" in open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read()
    # the header says why there is no device loop
    doc = header[header.index("lmrs_batch_forward with a sampler per row"):header.index("int lmrs_batch_forward_sample(")]
    assert "no device-resident sampled loop" in doc and "host round trip" in doc


def test_rust_externs_of_the_new_entry_points_match_the_header():
    from test_rust_crate import CMAP, c_prototypes
    cmap = dict(CMAP)
    cmap.update({"lmrs_batch*": "*mut LmrsBatch", "lmrs_sampler* const*": "*const *mut LmrsSampler", "lmrs_sampler*const*": "*const *mut LmrsSampler"})
    c = c_prototypes()
    # (lmrs_batch_forward_sample is declared in batch.rs, beside its caller: ffi.rs's batch block is pinned to the greedy entry points)
    txt = "".join(re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", f)).read()) for f in ("ffi.rs", "batch.rs"))
    for name in NAMES:
        m = re.search(rf"pub\s+fn\s+{name}\s*\((.*?)\)\s*->\s*c_int\s*;", txt, flags=re.S)
        assert m, name
        rargs = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in m.group(1).split(",") if a.strip()]
        cret, cargs = c[name]
        assert cret == "int" and len(cargs) == len(rargs), f"{name}: {cargs} vs {rargs}"
        for i, (ca, ra) in enumerate(zip(cargs, rargs)):
            assert cmap[ca] == ra, f"{name}: argument {i} is {ra} in Rust, {ca} in C"


def test_new_kernels_have_no_scratch_and_the_tables_have_not_moved():
    import json
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    new = {n: r for n, r in rows.items() if re.search(NEW_KERNELS, n)}
    # scale + maxima, exponentials, the chain as the sum and as the cdf, the division, the ordered candidates
    assert len(new) == 6, sorted(new)
    assert sum("batch_sample_chain_kernel" in n for n in new) == 2
    for n, r in new.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{n}: scratch {r['scratch']} bytes per lane, spilled VGPRs {r['vgpr_spill']}"
        assert not KR.HOT.match(n), f"{n} must not enter the hot table"
    # the one-row kernels share their bodies with the new ones and are what they were; so is every pinned table
    hot = json.load(open(KR.TABLE))
    assert set(hot) == {n for n in rows if KR.HOT.match(n)}, "the hot table's kernel classes moved"
    skinny = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_skinny.json")))
    assert set(skinny) == {n for n in rows if "gemm_skinny_kernel" in n}
    for table in (hot, skinny):
        for n, w in table.items():
            g = rows[n]
            assert (g["scratch"], g["vgpr_spill"], g["waves_per_simd"]) == (w["scratch"], w["vgpr_spill"], w["waves_per_simd"]), f"{n}: {w} -> {g}"
    for n in ("lmrs::sample_scale_max_kernel", "lmrs::sample_exp_kernel"):
        assert {k: rows[n][k] for k in hot[n]} == hot[n], f"{n}: {hot[n]} -> {rows[n]}"


def test_batch_sample_example_passes_the_syntax_check():
    src = os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_sample.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    txt = open(src).read()
    assert "forward_runs" in txt and "forward_sample" in txt and "--temperature" in txt and "--top-p" in txt
