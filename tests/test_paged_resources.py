"""The kernels of the paged table pass (lm.rs_amd/csrc/lmrs_paged.inc: paged_scatter_kernel, paged_attn_kernel) in the BUILT code objects: no scratch,
no spilled vector registers, waves per SIMD not below attention_runs_kernel's of the same <head size, Gemma> - the contiguous form whose operations they
repeat - and the registers of tests/golden/kernel_resources_paged.json, with the tolerances of tests/test_split_merged_resources.py; none of them
may match the hot table's name pattern.  No GPU."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_paged.json")
NEW_KERNELS = r"lmrs::paged_\w+_kernel"


def test_paged_kernel_resources():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    got = {n: r for n, r in rows.items() if re.match(NEW_KERNELS, n)}
    want = json.load(open(TABLE))
    # RoPE + scatter, and the attention for head sizes 64 / 96 / 128 and Gemma's 256
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
        if "paged_attn_kernel" in name:
            twin = rows.get(name.replace("paged_attn_kernel", "attention_runs_kernel"))
            if twin is None:
                bad.append(f"{name}: no attention_runs_kernel class of this shape")
            elif g["waves_per_simd"] < twin["waves_per_simd"]:
                bad.append(f"{name}: {g['waves_per_simd']} waves per SIMD, attention_runs_kernel has {twin['waves_per_simd']}")
    assert not bad, "paged kernel resources moved:\n  " + "\n  ".join(bad)
