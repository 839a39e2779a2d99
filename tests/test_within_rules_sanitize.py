"""The walk with an upper bound and the within host code under AddressSanitizer
+ UBSan (CPU only): a stand-alone program (tests/sanitize/within_rules_check.cpp)
built together with csrc/pm_seqrules_host.cpp runs csrc/pm_seqwalk.h's walk --
the function the device kernel calls -- on the host over seeded inputs, with
cursor arrays of exactly the set's longest run and every output array sized
exactly, and compares it with the twin.  Nothing is loaded into Python under a
sanitizer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "patternmatching_amd", "csrc")
HARNESS = os.path.join(REPO, "tests", "sanitize", "within_rules_check.cpp")


@pytest.fixture(scope="module")
def within_rules_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    assert os.path.exists(HARNESS)
    exe = str(tmp_path_factory.mktemp("asan_within_rules") / "within_rules_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I" + os.path.join(REPO, "include"), "-I" + CSRC, HARNESS, os.path.join(CSRC, "pm_seqrules_host.cpp"),
                    "-o", exe], check=True)
    return exe


def test_the_walk_and_the_within_host_code_clean_under_asan_ubsan(within_rules_check):
    # verify_asan_link_order=0: the environment may preload a library of its
    # own ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([within_rules_check], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.startswith("ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
