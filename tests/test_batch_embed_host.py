"""The embedding entry points of the batch API (tests/test_batch_embed.py) in every layer: header with its reference citations, library, Python, the
C++ mirror, the Rust crate; the example program's syntax; the resources of the one new kernel in the built code object; the committed resource tables.
No GPU."""
import inspect
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lmrs_batch_prefill_embeddings", "lmrs_batch_forward_runs_embed", "lmrs_batch_forward_runs_embed_sample")
# the kernel names the earlier batch tests count: the new kernel's name must match none of them
COUNTED = r"rope_scatter_runs_kernel|attention_runs_kernel|select_rows_kernel|attention_table_kernel|rope_scatter_rows_kernel|table_advance_kernel|cand_sort_"


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_entry_points_exist_in_every_layer():
    import lmrs_amd as L
    lib = L.lib()
    header = read("include", "lmrs_hip.h")
    hpp = read("lm.rs_amd", "hostcpp", "transformer.hpp")
    batch_rs = read("rust", "lmrs-hip", "src", "batch.rs")
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in L.EXPORTS and getattr(lib, name).argtypes is not None
        m = re.search(rf"/\*((?:(?!\*/).)*)\*/\s*int\s+{name}\(", header, flags=re.S)
        assert m, f"{name} is not declared in the header behind its comment"
        assert "transformer.rs:672-684" in m.group(1) and ":388-657" in m.group(1), f"{name}: the reference citations"
        assert name in hpp, f"{name} is not mirrored in transformer.hpp"
        assert re.search(rf"\bpub fn {name}\(", batch_rs), f"{name} is not declared in batch.rs"
        assert name not in read("rust", "lmrs-hip", "src", "ffi.rs")
    doc = header[header.index("== lmrs_fill_kv_cache(embeddings, n, start_pos) on a context"):header.index("int lmrs_batch_prefill_embeddings(")]
    assert "INTEGRATION.md" in doc and "never written" in doc and "nothing is downloaded" in doc
    doc = header[header.index("lmrs_batch_forward_runs with a kind per run"):header.index("int lmrs_batch_forward_runs_embed(")]
    assert "only on Gemma-2 past 4096 positions" in doc and "OWN position" in doc
    assert list(inspect.signature(L.Batch.prefill_embeddings).parameters) == ["self", "slot", "embeddings", "start_pos", "residual"]
    assert "prefill_embeddings(" in hpp and "std::vector<float> embeddings" in hpp
    assert "pub fn prefill_embeddings(" in batch_rs
    assert len(L.lib().lmrs_batch_prefill_embeddings.argtypes) == 6 and len(lib.lmrs_batch_forward_runs_embed.argtypes) == 14
    assert len(lib.lmrs_batch_forward_runs_embed_sample.argtypes) == 10


def test_rust_externs_match_the_header():
    from test_rust_crate import CMAP, c_prototypes
    cmap = dict(CMAP)
    cmap.update({"lmrs_batch*": "*mut LmrsBatch", "lmrs_sampler* const*": "*const *mut LmrsSampler", "lmrs_sampler*const*": "*const *mut LmrsSampler"})
    c = c_prototypes()
    src = re.sub(r"//[^\n]*", " ", read("rust", "lmrs-hip", "src", "batch.rs"))
    for name in NAMES:
        m = re.search(rf"pub\s+fn\s+{name}\s*\((.*?)\)\s*->\s*c_int\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in batch.rs"
        rargs = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in m.group(1).split(",") if a.strip()]
        cret, cargs = c[name]
        assert cret == "int" and len(cargs) == len(rargs), f"{name}: {cargs} vs {rargs}"
        for i, (ca, ra) in enumerate(zip(cargs, rargs)):
            assert cmap[ca] == ra, f"{name}: argument {i} is {ra} in Rust, {ca} in C"


def test_batch_image_example_passes_the_syntax_check():
    src = os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_image.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    txt = open(src).read()
    assert "prefill_embeddings(" in txt and "forward_runs(" in txt and "generate_greedy(" in txt
    for prog in ("batch_admit", "batch_greedy", "batch_sample"):    # Run / SampledRun grew a member: their brace initialisers still build
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "lm.rs_amd", "hostcpp", prog + ".cpp")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_new_kernel_has_no_scratch_and_the_tables_have_not_moved():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    new = {n: r for n, r in rows.items() if "source_rows_kernel" in n}
    assert len(new) == 1, sorted(new)
    for n, r in new.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{n}: {r}"
        assert not KR.HOT.match(n), f"{n} must not enter the hot table"
        assert not re.search(COUNTED, n), f"{n} matches a name pattern an earlier test counts"
    golden = os.path.join(ROOT, "tests", "golden")
    tables = sorted(f for f in os.listdir(golden) if re.fullmatch(r"kernel_resources.*\.json", f))
    assert "kernel_resources.json" in tables and len(tables) >= 4
    for f in tables:
        for n, w in json.load(open(os.path.join(golden, f))).items():
            assert n in rows, f"{f}: {n} is gone from the library"
            g = rows[n]
            assert (g["scratch"], g["vgpr_spill"], g["waves_per_simd"]) == (w["scratch"], w["vgpr_spill"], w["waves_per_simd"]), f"{f}: {n}: {w} -> {g}"
