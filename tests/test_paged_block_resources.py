"""The block-attention kernels over the page table (lm.rs_amd/csrc/lmrs_paged.inc: block_paged_scores_kernel, block_paged_scores_wide_kernel,
block_paged_values_kernel) in the BUILT code objects: one class per instantiation launch_attention_block uses, no scratch, no spilled registers,
waves per SIMD not below the contiguous twin's of the same template arguments - att_scores_kernel, att_scores_wide_kernel, att_values_kernel, whose
sums they repeat - and the registers of tests/golden/kernel_resources_paged_block.json, with tests/test_paged_resources.py's tolerance; none of them
may match the hot table's name pattern.  No GPU."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_paged_block.json")
NEW_KERNELS = r"lmrs::block_paged_\w+_kernel"
TWIN = {"block_paged_scores_kernel": "att_scores_kernel", "block_paged_scores_wide_kernel": "att_scores_wide_kernel",
        "block_paged_values_kernel": "att_values_kernel"}
# head sizes 64 / 96 / 128; Gemma-2's two score forms (32 keys on 8 waves, 64 keys on 4); the value slices of each head size, Gemma's 32- and 64-dim ones
EXPECTED = {"lmrs::block_paged_scores_kernel<64>", "lmrs::block_paged_scores_kernel<96>", "lmrs::block_paged_scores_kernel<128>",
            "lmrs::block_paged_scores_wide_kernel<256, 32, 512>", "lmrs::block_paged_scores_wide_kernel<256, 64, 256>",
            "lmrs::block_paged_values_kernel<64, 8, 4>", "lmrs::block_paged_values_kernel<96, 4, 12>", "lmrs::block_paged_values_kernel<128, 8, 8>",
            "lmrs::block_paged_values_kernel<256, 8, 4>", "lmrs::block_paged_values_kernel<256, 8, 8>"}


def test_paged_block_kernel_resources():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    got = {n: r for n, r in rows.items() if re.match(NEW_KERNELS, n)}
    want = json.load(open(TABLE))
    assert set(want) == EXPECTED, "the golden table names another set of classes"
    assert set(got) == EXPECTED, f"kernel classes added / removed: {sorted(set(got) ^ EXPECTED)}"
    bad = []
    for name, w in want.items():
        g = got[name]
        if KR.HOT.match(name) or re.match(r"lmrs::paged_\w+_kernel", name):
            bad.append(f"{name} must match neither the hot table's pattern nor the table pass's")
        if g["scratch"] != 0 or g["vgpr_spill"] != 0 or g["sgpr_spill"] != 0:
            bad.append(f"{name}: scratch {g['scratch']} bytes per lane, spilled registers {g['vgpr_spill']} / {g['sgpr_spill']}")
        if abs(g["vgpr"] + g["agpr"] - w["vgpr"] - w["agpr"]) > 16:
            bad.append(f"{name}: VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']}")
        stem = re.match(r"lmrs::(\w+)<", name).group(1)
        twin = rows.get(name.replace(stem, TWIN[stem]))
        if twin is None:
            bad.append(f"{name}: no {TWIN[stem]} class of these template arguments")
        elif g["waves_per_simd"] < twin["waves_per_simd"]:
            bad.append(f"{name}: {g['waves_per_simd']} waves per SIMD, {TWIN[stem]} has {twin['waves_per_simd']}")
    assert not bad, "paged block kernel resources moved:\n  " + "\n  ".join(bad)
