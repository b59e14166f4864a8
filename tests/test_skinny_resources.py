"""The skinny GEMM family (gemm_skinny_kernel: the GEMM of lmrs_verify_tokens' pass) in the BUILT code objects: no scratch, no spilled registers,
and the registers of tests/golden/kernel_resources_skinny.json - the gate of tests/test_tooling.py::test_hot_kernel_resources_have_not_moved,
same tolerances, for a family that is deliberately not part of the hot table.  No GPU."""
import json
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_skinny.json")


def _collect():
    pytest.importorskip("yaml", reason="PyYAML is needed to read the code objects' metadata")
    from tools import kernel_resources as KR
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(KR.LLVM, tool)):
            pytest.skip(f"{tool} not found under {KR.LLVM}")
    if not shutil.which("c++filt"):
        pytest.skip("c++filt not found")
    import lmrs_amd
    lmrs_amd.build()                                            # (no-op when the library is fresh)
    return {n: r for n, r in KR.collect(hot_only=False).items() if "gemm_skinny_kernel" in n}


def test_skinny_kernels_are_not_hot_names():
    from tools import kernel_resources as KR
    assert not KR.HOT.match("lmrs::gemm_skinny_kernel<0, 1, 8, false>")


def test_skinny_kernel_resources():
    got = _collect()
    want = json.load(open(TABLE))
    # 5 epilogues x {Q8_0, Q4_0} x {16-row tiles of 8 waves, 32-row tiles of 4 waves}
    assert len(got) == 20 and set(got) == set(want), f"kernel classes added / removed: {sorted(set(got) ^ set(want))[:6]}"
    bad = []
    for name, w in want.items():
        g = got[name]
        if g["scratch"] != 0 or g["vgpr_spill"] != 0:
            bad.append(f"{name}: scratch {g['scratch']} bytes per lane, spilled VGPRs {g['vgpr_spill']}")
        elif g["scratch"] != w["scratch"] or g["vgpr_spill"] != w["vgpr_spill"]:
            bad.append(f"{name}: scratch {w['scratch']} -> {g['scratch']}, spilled VGPRs {w['vgpr_spill']} -> {g['vgpr_spill']}")
        elif g["waves_per_simd"] != w["waves_per_simd"]:
            bad.append(f"{name}: waves per SIMD {w['waves_per_simd']} -> {g['waves_per_simd']} (VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']})")
        elif abs(g["vgpr"] + g["agpr"] - w["vgpr"] - w["agpr"]) > 16:
            bad.append(f"{name}: VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']}")
    assert not bad, "skinny kernel resources moved:\n  " + "\n  ".join(bad)
