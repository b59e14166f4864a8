"""Allowed-token masks (lmrs_batch_set_masks / _clear_masks / _mask_info), the part that needs no GPU: the symbols, the packed layout, the host program,
and mask_rows_kernel's resources in the BUILT code object against tests/golden/kernel_resources_mask.json - tests/test_skinny_resources.py's gate and
tolerances for a kernel of lmrs_score.o.  The device side is tests/test_batch_mask.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lmrs_batch_set_masks", "lmrs_batch_clear_masks", "lmrs_batch_mask_info")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_the_three_symbols_are_declared_exported_and_listed():
    import lmrs_amd
    lmrs_amd.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmrs_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(lmrs_amd.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/lmrs_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in lmrs_amd.EXPORTS, f"{name} is not in lmrs_amd.EXPORTS"
    # the Rust binding declares no batch call (tests/test_rust_crate.py has no mapping for them)
    assert "lmrs_batch_set_masks" not in open(os.path.join(ROOT, "rust", "lmrs-hip", "src", "ffi.rs")).read()


def test_refusals_that_need_no_device():
    """a NULL batch is refused by name before anything else is looked at"""
    import lmrs_amd
    lib = lmrs_amd.lib()
    n = ctypes.c_uint32(7)
    for call, name in ((lambda: lib.lmrs_batch_set_masks(None, 0, None, None), NAMES[0]), (lambda: lib.lmrs_batch_clear_masks(None, 0, None), NAMES[1]),
                       (lambda: lib.lmrs_batch_mask_info(None, 0, ctypes.byref(n)), NAMES[2])):
        assert call() != 0
        assert lib.lmrs_last_error().decode().startswith(name + ": NULL argument"), lib.lmrs_last_error().decode()


@pytest.mark.parametrize("V", [1, 31, 32, 33, 48, 4096, 4112, 40000])
def test_pack_mask_round_trips(V):
    """bit t -> word t >> 5, bit t & 31; vocabularies that are no multiple of 32 (4112 = 16 * 257: a batch may have one) leave the top bits of the last word zero"""
    import lmrs_amd
    rng = np.random.default_rng(V)
    a = rng.random((3, V)) < 0.5
    a[1] = False; a[1, [0, V - 1, min(31, V - 1), min(32, V - 1)]] = True
    w = lmrs_amd.pack_mask(a)
    W = (V + 31) // 32
    assert w.dtype == np.uint32 and w.shape == (3, W)
    for r in range(3):
        for t in list(range(min(V, 70))) + list(range(max(0, V - 70), V)):
            assert bool(int(w[r, t >> 5]) >> (t & 31) & 1) == bool(a[r, t]), (r, t)
        assert sum(bin(int(x)).count("1") for x in w[r]) == int(a[r].sum()), "a bit at or above vocab_size is set"
    back = lmrs_amd.unpack_mask(w, V)
    assert back.dtype == np.bool_ and back.shape == a.shape and (back == a).all()
    one = lmrs_amd.pack_mask(a[2])                                                    # a single mask: 1-D in, 1-D out
    assert one.shape == (W,) and (one == w[2]).all() and (lmrs_amd.unpack_mask(one, V) == a[2]).all()
    with pytest.raises(lmrs_amd.LmrsError):
        lmrs_amd.pack_mask(a.astype(np.uint8))
    with pytest.raises(lmrs_amd.LmrsError):
        lmrs_amd.unpack_mask(np.zeros(W + 1, np.uint32), V)


def test_batch_constrained_program_and_host_mirror_compile():
    for example in ("batch_constrained.cpp", "batch_sample.cpp"):
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(ROOT, "lm.rs_amd", "hostcpp", example)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    hpp = open(os.path.join(ROOT, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name in NAMES:
        assert name + "(" in hpp, f"transformer.hpp's Batch does not call {name}"


def _collector():
    pytest.importorskip("yaml", reason="PyYAML is needed to read the code objects' metadata")
    from tools import kernel_resources as KR
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(KR.LLVM, tool)):
            pytest.skip(f"{tool} not found under {KR.LLVM}")
    if not shutil.which("c++filt"):
        pytest.skip("c++filt not found")
    import lmrs_amd
    lmrs_amd.build()                                            # (no-op when the library is fresh)
    return KR


def _moved(got, want):
    """tests/test_skinny_resources.py's rule, per class"""
    bad = []
    for name, w in want.items():
        g = got[name]
        if g["scratch"] != w["scratch"] or g["vgpr_spill"] != w["vgpr_spill"]:
            bad.append(f"{name}: scratch {w['scratch']} -> {g['scratch']}, spilled VGPRs {w['vgpr_spill']} -> {g['vgpr_spill']}")
        elif g["waves_per_simd"] != w["waves_per_simd"]:
            bad.append(f"{name}: waves per SIMD {w['waves_per_simd']} -> {g['waves_per_simd']} (VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']})")
        elif abs(g["vgpr"] + g["agpr"] - w["vgpr"] - w["agpr"]) > 16:
            bad.append(f"{name}: VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']}")
    return bad


def test_mask_rows_kernel_resources():
    KR = _collector()
    got = {n: r for n, r in KR.collect(hot_only=False).items() if "mask_rows_kernel" in n}
    want = json.load(open(os.path.join(GOLDEN, "kernel_resources_mask.json")))
    assert len(got) == 1 and set(got) == set(want), f"kernel classes added / removed: {sorted(set(got) ^ set(want))}"
    for name, g in got.items():
        assert not KR.HOT.match(name), f"{name} must not fall under the hot table's pattern"
        assert g["scratch"] == 0 and g["vgpr_spill"] == 0 and g["sgpr_spill"] == 0 and g["lds_static"] == 0, f"{name}: scratch / spills / LDS: {g}"
    assert not _moved(got, want), "mask_rows_kernel's resources moved:\n  " + "\n  ".join(_moved(got, want))


def test_the_committed_hot_and_skinny_tables_are_what_the_library_gives():
    """the mask launch lives in lmrs_score.o: the objects behind the other tables hold the classes they held, at the registers the tables allow"""
    KR = _collector()
    got = KR.collect(hot_only=True)
    want = json.load(open(KR.TABLE))
    assert set(got) == set(want), f"hot kernel classes added / removed: {sorted(set(got) ^ set(want))[:6]}"
    assert not _moved(got, want), "hot kernel resources moved:\n  " + "\n  ".join(_moved(got, want)[:12])
    every = KR.collect(hot_only=False)
    assert not [n for n in got if "mask_rows_kernel" in n] and [n for n in every if "mask_rows_kernel" in n], "mask_rows_kernel must be read, and not as a hot class"
    skinny = {n: r for n, r in every.items() if "gemm_skinny_kernel" in n}
    want = json.load(open(os.path.join(GOLDEN, "kernel_resources_skinny.json")))
    assert set(skinny) == set(want) and not _moved(skinny, want), _moved(skinny, want)
