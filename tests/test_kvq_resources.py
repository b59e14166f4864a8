"""The kernels of the Q8 table pass (lm.rs_amd/csrc/lmrs_kvq.inc: kvq_scatter_kernel, kvq_import_kernel, kvq_attn_kernel) in the BUILT code objects: no
scratch, no spilled vector registers, none in the hot table, waves per SIMD not below paged_attn_kernel's of the same <head size, Gemma>, and the registers
of tests/golden/kernel_resources_kvq.json with the tolerances of tests/test_paged_resources.py.  No GPU."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_kvq.json")


def test_kvq_kernel_resources():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    got = {n: r for n, r in rows.items() if re.match(r"lmrs::kvq_\w+_kernel", n)}
    want = json.load(open(TABLE))
    # RoPE + quantising scatter, the quantising copy, and the attention for head sizes 64 / 96 / 128 and Gemma's 256
    assert len(got) == 6 and set(got) == set(want), f"kernel classes added / removed: {sorted(set(got) ^ set(want))}"
    bad = []
    for name, w in want.items():
        g = got[name]
        if KR.HOT.match(name) or re.match(r"lmrs::paged_\w+_kernel", name):
            bad.append(f"{name} must not enter the hot table or the paged kernels' pattern")
        elif g["scratch"] != 0 or g["vgpr_spill"] != 0:
            bad.append(f"{name}: scratch {g['scratch']} bytes per lane, spilled VGPRs {g['vgpr_spill']}")
        elif g["waves_per_simd"] != w["waves_per_simd"]:
            bad.append(f"{name}: waves per SIMD {w['waves_per_simd']} -> {g['waves_per_simd']} (VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']})")
        elif abs(g["vgpr"] + g["agpr"] - w["vgpr"] - w["agpr"]) > 16:
            bad.append(f"{name}: VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']}")
        if "kvq_attn_kernel" in name:
            twin = rows.get(name.replace("kvq_attn_kernel", "paged_attn_kernel"))
            if twin is None:
                bad.append(f"{name}: no paged_attn_kernel class of this shape")
            elif g["waves_per_simd"] < twin["waves_per_simd"]:
                bad.append(f"{name}: {g['waves_per_simd']} waves per SIMD, paged_attn_kernel has {twin['waves_per_simd']}")
    assert not bad, "Q8 kernel resources moved:\n  " + "\n  ".join(bad)
