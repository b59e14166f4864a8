"""The host side of paged batches (lmrs_batch_create_paged, lmrs_batch_pages, lmrs_batch_slot_pages, lmrs_batch_release): the entry points in every
layer, the Rust declarations against the header, and hostcpp/batch_paged.cpp - its syntax here, and on the GPU a shared-prompt session whose
continuations do not depend on how many slots and pages it was given."""
import inspect
import os
import re
import subprocess

import pytest

from tools import synth_lmrs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lmrs_batch_create_paged", "lmrs_batch_pages", "lmrs_batch_slot_pages", "lmrs_batch_release")
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    lmrs_amd.build()
    return lmrs_amd


def test_entry_points_exist_in_every_layer(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "lmrs_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read()
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in L.EXPORTS
        assert re.search(rf"\bint\s+{name}\(", header), f"{name} is not declared in the header"
        assert re.search(rf"\bpub fn {name}\(", rust), f"{name} is not declared in the Rust crate"
        assert name in hpp, f"{name} is not mirrored in transformer.hpp"
    assert "no reference counterpart" in header[header.index("---- paged K/V"):header.index("int lmrs_batch_create_paged(")]
    p = inspect.signature(L.Batch.__init__).parameters
    assert p["page_len"].default is None and p["n_pages"].default is None and p["page_len"].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(L.Batch.pages) and callable(L.Batch.slot_pages) and inspect.signature(L.Batch.release).parameters["n_pos"].default == 0
    for fn in ("pub fn new_paged(", "pub fn pages(", "pub fn slot_pages(", "pub fn release("):
        assert fn in rust, fn


def test_rust_externs_of_the_new_entry_points_match_the_header():
    """(declared in batch.rs beside their callers, as the wide batch's calls are: the batch block of ffi.rs is pinned by tests/test_batch.py)"""
    from test_rust_crate import CMAP, c_prototypes
    cmap = dict(CMAP)
    cmap.update({"lmrs_batch*": "*mut LmrsBatch", "const lmrs_batch*": "*const LmrsBatch", "lmrs_batch**": "*mut *mut LmrsBatch", "lmrs_ctx*": "*mut ffi::LmrsCtx"})
    c = c_prototypes()
    src = re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "batch.rs")).read())
    for name in NAMES:
        m = re.search(rf"pub\s+fn\s+{name}\s*\((.*?)\)\s*->\s*c_int\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in batch.rs"
        rargs = [re.sub(r"\s+", " ", a.split(":", 1)[1].strip()) for a in m.group(1).split(",") if a.strip()]
        cret, cargs = c[name]
        assert cret == "int" and len(cargs) == len(rargs), f"{name}: {cargs} vs {rargs}"
        for i, (ca, ra) in enumerate(zip(cargs, rargs)):
            assert cmap[ca] == ra, f"{name}: argument {i} is {ra} in Rust, {ca} in C"


def test_batch_paged_example_passes_the_syntax_check():
    src = os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_paged.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@gpu
def test_batch_paged_program_reuses_slots_and_pages(tmp_path):
    """hostcpp/batch_paged.cpp, built and run twice over the same seven lines behind one system prompt (a small tokenizer.bin in the layout of
    tokenizer.rs:24-64 for mini-llama's vocabulary): with slots and pages for everybody at once, and with three continuation slots and a pool of four
    pages - two of them the system prompt's - where lines wait for a finished one's page.  The continuations are equal, line by line; every
    admission shares the system prompt's whole page; at the end only the system prompt's pages are held."""
    import struct
    cfg = S.CONFIGS["mini-llama"]
    S.build_image(cfg, S.Q8_0, seed=571).tofile(tmp_path / "model.lmrs")
    toks = [("<unk>", 0.0), ("<s>", 0.0), ("</s>", 0.0)] + [("<0x%02X>" % b, 0.0) for b in range(256)]
    toks += [(ch, -1.0 - i) for i, ch in enumerate(" abcdefghijklmnopqrstuvwxyz")]
    toks += [(m, 5.0 - 0.1 * i) for i, m in enumerate(["he", "ll", "hell", "hello", " w", "or", "ld", " world", "wor"])]
    toks += [("<fill_%d>" % i, 0.0) for i in range(cfg.vocab_size - len(toks))]
    blob = struct.pack("IIII", len(toks), 16, 1, 2)
    for s_, sc in toks:
        b = s_.encode(); blob += struct.pack("fI", sc, len(b)) + b
    (tmp_path / "tokenizer.bin").write_bytes(blob)
    lines = ["hello world", "world", "a quick brown fox", "hello hello hello world", "the longest of them all by far", "or", "hell"]
    (tmp_path / "prompts.txt").write_text("\n".join(lines) + "\n")
    system = "you are a world " * 7                          # 7 x 11 tokens or so: more than one page of 64 positions, fewer than two with a line and 12 tokens
    exe = str(tmp_path / "batch_paged")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "lm.rs_amd", "hostcpp", "batch_paged.cpp"), "-I", os.path.join(ROOT, "include"),
                    "-L", os.path.join(ROOT, "lm.rs_amd"), "-llmrs_hip", f"-Wl,-rpath,{os.path.join(ROOT, 'lm.rs_amd')}", "-o", exe], check=True)
    out = {}
    for name, extra in (("roomy", ["--slots", "8", "--pages", "32"]), ("tight", ["--slots", "4", "--pages", "4"])):
        r = subprocess.run([exe, "--model", str(tmp_path / "model.lmrs"), "--tokenizer", str(tmp_path / "tokenizer.bin"), "--prompts", str(tmp_path / "prompts.txt"),
                            "--system", system, "--n", "12"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = r.stdout.split("\n")
    cont = {k: sorted(l for l in v if l.startswith("[")) for k, v in out.items()}
    assert len(cont["roomy"]) == 7 and cont["tight"] == cont["roomy"], out
    for k, v in out.items():
        admits = [l for l in v if l.startswith("admit line")]
        assert len(admits) == 7 and all("holds 2 pages (1 shared)" in l for l in admits), (k, admits)
    assert out["roomy"][0].startswith("system prompt:") and " in 2 pages of 64 positions; 30 of 32 pages free" in out["roomy"][0], out["roomy"][0]
    assert "30 of 32 pages free at the end" in out["roomy"][-2] and "2 of 4 pages free at the end" in out["tight"][-2]
    assert [int(re.search(r"into slot (\d+)", l).group(1)) for l in out["tight"] if l.startswith("admit line")].count(1) >= 2, "slot 1 was not reused"
