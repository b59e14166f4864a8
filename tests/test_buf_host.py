"""The owner template of device and pinned memory (lm.rs_amd/csrc/lmrs_buf.h: a template with no HIP in it) on the CPU: tests/buf_check.cpp - a stand-alone
program with its own main - instantiates it over a counting policy backed by malloc and checks that a moved-from owner is empty, that move-assignment frees
the target's old block exactly once, that an all-or-nothing set whose k-th allocation fails (every k) is left null with exactly the obtained blocks released,
none twice, that a set which grows releases the old blocks before it obtains the new, that a zero count still obtains a block, and that at exit obtained
equals released.  Built with -fsanitize=address,undefined where a trial link with those flags works (as tests/test_pages_host.py builds its program); no
Python process loads the sanitized code."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lm.rs_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """(the program, whether it is sanitized)"""
    d = tmp_path_factory.mktemp("buf_check")
    trial = d / "trial.cpp"
    trial.write_text("int main() { return 0; }\n")
    san = subprocess.run(["g++", *SAN, str(trial), "-o", str(d / "trial")], capture_output=True).returncode == 0 and \
        subprocess.run([str(d / "trial")], capture_output=True).returncode == 0
    exe = d / "buf_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(SAN if san else []), "-I", CSRC, os.path.join(ROOT, "tests", "buf_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe), san


def test_owners_keep_the_books(check):
    exe, _ = check
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "buf_check: ok" in r.stdout


def test_the_check_program_was_sanitized(check):
    _, san = check
    if not san:
        pytest.skip("g++ -fsanitize=address,undefined does not link here: the check program ran without the sanitizers")


def test_the_template_has_no_hip_in_it():
    txt = open(os.path.join(CSRC, "lmrs_buf.h")).read()
    assert "#include <hip" not in txt and "hipMalloc(" not in txt and "hipFree(" not in txt


def test_the_runtime_frees_are_the_policies():
    """hipFree / hipHostFree in lmrs_api.hip: the two policies, and the memory that is not an owner's - the arena, the exchange arena, the shards' pfx_* blocks"""
    hits = [ln.strip() for ln in open(os.path.join(CSRC, "lmrs_api.hip")) if "hipFree(" in ln or "hipHostFree(" in ln]
    for ln in hits:
        assert ln.startswith(("struct DevMem", "struct PinMem")) or "c->arena" in ln or "c->xarena" in ln or "c->pfx_" in ln, ln
    assert sum(ln.startswith("struct ") for ln in hits) == 2
