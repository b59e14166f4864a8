"""The host side of the token-tree pass (lmrs_batch_forward_tree, lmrs_batch_accept_path, lmrs_tree_accept): greedy acceptance on hand-written trees, and
the entry points in every layer.  No GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lmrs_batch_forward_tree", "lmrs_batch_accept_path", "lmrs_tree_accept")


@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    lmrs_amd.build()
    return lmrs_amd


# (parents, tokens, argmax, expected) -> (path, next)
ACCEPT = {
    "nothing": (([None, None, 0], [5, 6, 7], [1, 2, 3], 9), ([], 9)),
    "full-chain": (([None, 0, 1, 2], [5, 6, 7, 8], [6, 7, 8, 4], 5), ([0, 1, 2, 3], 4)),
    # depth 0: node 0; depth 1: node 1 (8) or its sibling 2 (7) - the model says 7; depth 2 under the sibling: node 4, whose argmax nobody drafted
    "branch-at-depth-2": (([None, 0, 0, 1, 2, 2], [5, 8, 7, 3, 3, 2], [7, 3, 3, 1, 11, 12], 5), ([0, 2, 4], 11)),
    "same-token-twice": (([None, None, 0, 1], [5, 5, 6, 6], [6, 6, 2, 3], 5), ([0, 2], 2)),
    "stops-inside": (([None, 0, 1], [5, 6, 7], [6, 9, 8], 5), ([0, 1], 9)),
}


@pytest.mark.parametrize("case", list(ACCEPT))
def test_tree_accept(L, case):
    (parents, tokens, argmax, expected), want = ACCEPT[case]
    assert L.tree_accept(parents, tokens, argmax, expected) == want


def test_tree_accept_refuses_a_parent_at_or_above_its_index(L):
    with pytest.raises(RuntimeError, match=r"lmrs_tree_accept: parent\[1\] = 1 is neither LMRS_TREE_ROOT nor below its own index"):
        L.tree_accept([None, 1], [1, 2], [1, 2], 1)
    assert L.tree_accept([], [], [], 7) == ([], 7)


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
    assert "#define LMRS_TREE_ROOT 0xFFFFFFFFu" in header and L.TREE_ROOT == 0xFFFFFFFF
    assert callable(L.Batch.forward_tree) and callable(L.Batch.accept_path) and callable(L.tree_accept)
