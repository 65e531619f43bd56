"""CPU: the mini-host's plain-C binary16 conversions and base functions
(zhpe-ompi_amd/mca/host/mx_host.c) built with the host compiler under
AddressSanitizer and UBSan into a stand-alone program
(tests/native/half_check.c) and run: exact half -> float, round trip,
nearest-even rounding at every tie, no access past the operands."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no host C compiler")
def test_host_binary16_under_host_sanitizers(tmp_path):
    exe = tmp_path / "half_check"
    mca = os.path.join(ROOT, "zhpe-ompi_amd", "mca")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", mca, os.path.join(ROOT, "tests", "native", "half_check.c"),
                    os.path.join(mca, "host", "mx_host.c"), "-o", str(exe), "-ldl", "-lm"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
