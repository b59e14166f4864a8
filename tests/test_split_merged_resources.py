"""The merged qkv + scores launch (qkv_scores_kernel: the split attention form's score items behind the qkv GEMV workgroups) in the BUILT code
objects: no scratch, no spilled vector registers, and the registers of tests/golden/kernel_resources_split_merged.json - the gate of
tests/test_tooling.py::test_hot_kernel_resources_have_not_moved, same tolerances, in a table of its own as the skinny and the stream GEMM
families have theirs (tests/test_skinny_resources.py).  The GEMV role shares its registers with the score role: against the plain qkv GEMV of
the six-launch form it does lose occupancy (Llama-3.2-1B: five waves per SIMD there, three here; the measured gain is net of that), so the
floor held here is the wave-form launch of the same shape (qkv_attn_kernel), whose GEMV role it copies.  No GPU."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_split_merged.json")


def test_qkv_scores_kernel_resources():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    got = {n: r for n, r in rows.items() if "qkv_scores_kernel" in n}
    want = json.load(open(TABLE))
    # one class per qkv_attn_kernel shape: Llama 1B / 3B, Phi (96-wide heads), Gemma-2 (256-wide heads), Q8_0 and Q4_0 tiles
    assert len(got) == 9 and set(got) == set(want), f"kernel classes added / removed: {sorted(set(got) ^ set(want))[:6]}"
    bad = []
    for name, w in want.items():
        g = got[name]
        shape = re.search(r"<(.*)>", name).group(1)
        wave_forms = [r for n, r in rows.items() if n.startswith(f"lmrs::qkv_attn_kernel<{shape}, ")]
        if not wave_forms:
            bad.append(f"{name}: no qkv_attn_kernel class of this shape")
        elif g["scratch"] != 0 or g["vgpr_spill"] != 0:
            bad.append(f"{name}: scratch {g['scratch']} bytes per lane, spilled VGPRs {g['vgpr_spill']}")
        elif g["waves_per_simd"] < min(r["waves_per_simd"] for r in wave_forms):
            bad.append(f"{name}: {g['waves_per_simd']} waves per SIMD, the wave form has {min(r['waves_per_simd'] for r in wave_forms)}")
        elif g["waves_per_simd"] != w["waves_per_simd"]:
            bad.append(f"{name}: waves per SIMD {w['waves_per_simd']} -> {g['waves_per_simd']} (VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']})")
        elif abs(g["vgpr"] + g["agpr"] - w["vgpr"] - w["agpr"]) > 16:
            bad.append(f"{name}: VGPRs {w['vgpr']}+{w['agpr']} -> {g['vgpr']}+{g['agpr']}")
    assert not bad, "qkv + scores kernel resources moved:\n  " + "\n  ".join(bad)
