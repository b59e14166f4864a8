"""The page accounting of paged batches (lm.rs_amd/csrc/lmrs_pages.cpp: plain C++, no HIP) on the CPU: tests/pages_fuzz.cpp - a stand-alone program with
its own main - runs a few thousand random write / fork / release operations a seed, plans that must fail among them, beside a naive model of what every
position of every slot should read, and audits the pool after each: reference counts against the table, free + held = n_pages, the zero page never a
destination, a refused plan changing nothing, every position read back through the table.  Built with -fsanitize=address,undefined where a trial link
with those flags works; no Python process loads the sanitized code."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lm.rs_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    """(the program, whether it is sanitized)"""
    d = tmp_path_factory.mktemp("pages_fuzz")
    trial = d / "trial.cpp"
    trial.write_text("int main() { return 0; }\n")
    san = subprocess.run(["g++", *SAN, str(trial), "-o", str(d / "trial")], capture_output=True).returncode == 0 and \
        subprocess.run([str(d / "trial")], capture_output=True).returncode == 0
    exe = d / "pages_fuzz"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *(SAN if san else []), "-I", CSRC, os.path.join(CSRC, "lmrs_pages.cpp"),
           os.path.join(ROOT, "tests", "pages_fuzz.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe), san


@pytest.mark.parametrize("seed", [1, 2, 3, 5, 8, 13])
def test_random_operations_keep_the_books(fuzz, seed):
    exe, _ = fuzz
    r = subprocess.run([exe, str(seed), "4000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ": ok" in r.stdout


def test_the_fuzz_program_was_sanitized(fuzz):
    _, san = fuzz
    if not san:
        pytest.skip("g++ -fsanitize=address,undefined does not link here: the fuzz program ran without the sanitizers")


def test_the_accounting_file_has_no_hip_in_it():
    for f in ("lmrs_pages.h", "lmrs_pages.cpp"):
        txt = open(os.path.join(CSRC, f)).read()
        assert "#include <hip" not in txt and "hipMalloc" not in txt and "__global__" not in txt, f
