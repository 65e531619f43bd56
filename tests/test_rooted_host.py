"""CPU: the rooted exchange planner (csrc/mx_rooted_plan.hip) compiles with the
host compiler alone -- no HIP library -- and, under AddressSanitizer and
UBSan, its plans for gather, gatherv, scatter and scatterv move exactly the
bytes a brute-force walk moves, on 1, 2, 3, 5 and 16 simulated ranks
(tests/native/rooted_check.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_rooted_plan_under_host_sanitizers(tmp_path):
    exe = tmp_path / "rooted_check"
    csrc = os.path.join(ROOT, "zhpe-ompi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "native", "rooted_check.cpp"), "-x", "c++",
                    os.path.join(csrc, "mx_rooted_plan.hip"), os.path.join(csrc, "mx_exchange_vec_plan.hip"),
                    os.path.join(csrc, "mx_exchange_plan.hip"), os.path.join(csrc, "mx_ddt_layout.hip"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
