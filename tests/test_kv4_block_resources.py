"""The kernels of block attention over Q4 pages (lm.rs_amd/csrc/lmrs_kv4.inc: block_kv4_scores_kernel, block_kv4_scores_wide_kernel,
block_kv4_values_kernel) in the BUILT code objects: exactly the ten instantiations the launcher names, no scratch, no spilled vector or scalar
registers, none in the hot table or in the paged and Q8 kernels' patterns.  No GPU."""
import re

WANT = {f"lmrs::block_kv4_scores_kernel<{hs}>" for hs in (64, 96, 128)} | {f"lmrs::block_kv4_scores_wide_kernel<256, {nk}, {nt}>" for nk, nt in ((32, 512), (64, 256))} | {
    f"lmrs::block_kv4_values_kernel<{hs}, {nw}, {dw}>" for hs, nw, dw in ((64, 8, 4), (96, 4, 12), (128, 8, 8), (256, 8, 4), (256, 8, 8))}


def test_kv4_block_kernel_resources():
    from test_batch import _collect_new_kernels
    KR, rows = _collect_new_kernels()
    got = {n: r for n, r in rows.items() if re.match(r"lmrs::block_kv4_\w+_kernel", n)}
    assert len(got) == 10 and set(got) == WANT, f"kernel classes added / removed: {sorted(set(got) ^ WANT)}"
    bad = []
    for name, g in got.items():
        if KR.HOT.match(name) or re.match(r"lmrs::paged_\w+_kernel", name) or re.match(r"lmrs::kvq_\w+_kernel", name):
            bad.append(f"{name} must not enter the hot table, the paged kernels' or the Q8 kernels' pattern")
        if g["scratch"] != 0 or g["vgpr_spill"] != 0 or g["sgpr_spill"] != 0:
            bad.append(f"{name}: scratch {g['scratch']} bytes per lane, spilled VGPRs {g['vgpr_spill']}, spilled SGPRs {g['sgpr_spill']}")
    assert not bad, "Q4 block kernel resources:\n  " + "\n  ".join(bad)
