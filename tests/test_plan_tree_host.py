"""CPU: the planning unit (csrc/mx_plan.hip) plans the oracle's trees.

tests/native/plan_tree_check.cpp links the planner, compiled as host C++,
with the collective oracle (oracle/mx_oracle_coll.c, oracle/mx_oracle_op.c)
and compares, tree for tree, what every rank's every element carries for
2..MX_MAX_RANKS ranks, every root, in place and not; every DAG's VM program
is interpreted for every owner with the info bit clear and set.  All of it
runs under AddressSanitizer and UBSan, as a stand-alone program."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("gcc") is None, reason="no host C/C++ compiler")
def test_planned_trees_are_the_oracles_under_host_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "zhpe-ompi_amd", "csrc")
    objs = []
    for name in ("mx_oracle_coll", "mx_oracle_op"):      # the oracle Makefile's floating-point and overflow flags
        objs.append(str(tmp_path / (name + ".o")))
        subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-fwrapv", "-ffp-contract=off", *SAN, "-c",
                        os.path.join(ROOT, "oracle", name + ".c"), "-o", objs[-1]], check=True)
    exe = tmp_path / "plan_tree_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", csrc,
                    os.path.join(ROOT, "tests", "native", "plan_tree_check.cpp"),
                    "-x", "c++", os.path.join(csrc, "mx_plan.hip"), "-x", "none", *objs, "-lm", "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    m = re.search(r"(\d+) tree comparisons, (\d+) VM outputs, (\d+) decisions, (\d+) segmented-ring cases in phases, "
                  r"0 mismatches", r.stdout)
    assert m, r.stdout
    # nothing was skipped: the figures of the full walk
    assert int(m.group(1)) > 1_000_000 and int(m.group(2)) > 300_000 and int(m.group(3)) > 19_000 and int(m.group(4)) > 0
