"""The kernels of the token-tree pass (lm.rs_amd/csrc/lmrs_tree.inc: tree_scatter_kernel, tree_attn_kernel, tree_commit_kernel) in the BUILT code
objects: exactly the twelve instantiations the launchers name, no scratch, no spilled vector or scalar registers, none in the hot table or in another
family's pattern.  No GPU."""
import re

WANT = {f"lmrs::tree_scatter_kernel<{p}>" for p in ("false", "true")} | {f"lmrs::tree_commit_kernel<{p}>" for p in ("false", "true")} | {
    f"lmrs::tree_attn_kernel<{hs}, {g}, {p}>" for hs, g in ((64, "false"), (96, "false"), (128, "false"), (256, "true")) for p in ("false", "true")}
OTHERS = [r"lmrs::paged_\w+_kernel", r"lmrs::kvq_\w+_kernel", r"lmrs::block_kv4_\w+_kernel", r"lmrs::block_paged_", r"lmrs::rope_scatter_rows_kernel",
          r"lmrs::rope_scatter_runs_kernel", r"lmrs::attention_table_kernel", r"lmrs::attention_runs_kernel", r"lmrs::select_rows_kernel", r"lmrs::table_advance_kernel"]


def test_tree_kernel_resources():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    got = {n: r for n, r in rows.items() if re.match(r"lmrs::tree_\w+_kernel", n)}
    assert len(got) == 12 and set(got) == WANT, f"kernel classes added / removed: {sorted(set(got) ^ WANT)}"
    bad = []
    for name, g in got.items():
        if KR.HOT.match(name) or any(re.match(p, name) for p in OTHERS):
            bad.append(f"{name} must not enter the hot table or another family's pattern")
        if g["scratch"] != 0 or g["vgpr_spill"] != 0 or g["sgpr_spill"] != 0:
            bad.append(f"{name}: scratch {g['scratch']} bytes per lane, spilled VGPRs {g['vgpr_spill']}, spilled SGPRs {g['sgpr_spill']}")
    assert not bad, "tree kernel resources:\n  " + "\n  ".join(bad)
