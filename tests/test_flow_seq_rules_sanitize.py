"""The flow ordered rules' walk and host code under AddressSanitizer + UBSan
(CPU only): a stand-alone program (tests/sanitize/flow_seq_rules_check.cpp)
built together with csrc/pm_flowseqrules_host.cpp (and csrc/pm_seqrules_host.cpp,
whose checks and records it uses) runs csrc/pm_flowseqwalk.h's advance and rule
walk -- the functions the device kernel calls -- on the host from the device's
tables over seeded flows cut into calls, with every array sized exactly, and
compares hits and rows with the twin.  Nothing is loaded into Python under a
sanitizer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "patternmatching_amd", "csrc")
HARNESS = os.path.join(REPO, "tests", "sanitize", "flow_seq_rules_check.cpp")


@pytest.fixture(scope="module")
def flow_seq_rules_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    assert os.path.exists(HARNESS)
    exe = str(tmp_path_factory.mktemp("asan_flow_seq_rules") / "flow_seq_rules_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I" + os.path.join(REPO, "include"), "-I" + CSRC, HARNESS,
                    os.path.join(CSRC, "pm_flowseqrules_host.cpp"), os.path.join(CSRC, "pm_seqrules_host.cpp"),
                    "-o", exe], check=True)
    return exe


def test_the_walk_and_the_flow_seq_host_code_clean_under_asan_ubsan(flow_seq_rules_check):
    # verify_asan_link_order=0: the environment may preload a library of its
    # own ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([flow_seq_rules_check], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.startswith("ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
