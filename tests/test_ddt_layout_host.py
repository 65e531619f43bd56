"""CPU: the datatype layout planner (csrc/mx_ddt_layout.hip) compiles with the
host compiler alone -- no HIP library -- and, under AddressSanitizer and
UBSan, every table and tile size it plans for the 18 golden types and for
the convertor fuzz's layouts (its SEEDS x CLASSES) keeps the invariants the
convertor's kernels trust (tests/native/ddt_layout_check.cpp).

Each case carries an index map of one instance that does not come from the
planner: `Layout.map` for the fuzz layouts; for the golden types the CPU
oracle packs one instance of a buffer holding its own offsets, a byte of them
at a time.  The piece tables are checked for all 16 user-origin alignments
in every case (the program runs about ten seconds under the sanitizers)."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ddt_gen as G
import golden_io
import oracle_lib
from test_convertor_fuzz import SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name, desc, nrec, size, lb, ub, tlb, tub, basic, m):
    m = np.ascontiguousarray(m, np.int64)
    assert m.size == size and len(desc) == 32 * nrec
    return b"".join([name.encode()[:63].ljust(64, b"\0"), struct.pack("<II5q", nrec, 0, size, lb, ub, tlb, tub),
                     np.ascontiguousarray(basic, np.uint64).tobytes(), bytes(desc), m.tobytes()])


def _golden_map(rec, basic):
    """user offset of every packed byte of one instance, from the oracle's walk"""
    O = oracle_lib.oracle()
    vp, sz, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64
    O.mxo_ddt_convert.argtypes = [vp, sz, vp, i64, i64, sz, vp, vp, ctypes.c_int]
    tlb, tub = rec["true_lb"], rec["true_ub"]
    at = np.arange(tub - tlb, dtype=np.int64)
    m = np.zeros(rec["size"], np.int64)
    for k in range(4):                      # offsets below 2^32, one byte of them per pack
        user = ((at >> (8 * k)) & 255).astype(np.uint8)
        out = np.zeros(rec["size"], np.uint8)
        n = O.mxo_ddt_convert(rec["desc"].ctypes.data, rec["nrec"], basic.ctypes.data, rec["lb"], rec["ub"], 1,
                              user.ctypes.data - tlb, out.ctypes.data, 0)
        assert n == rec["size"]
        m |= out.astype(np.int64) << (8 * k)
    assert tub - tlb < 1 << 32
    return m + tlb


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_layout_invariants_under_host_sanitizers(tmp_path):
    exe = tmp_path / "ddt_layout_check"
    csrc = os.path.join(ROOT, "zhpe-ompi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "native", "ddt_layout_check.cpp"),
                    "-x", "c++", os.path.join(csrc, "mx_ddt_layout.hip"), "-o", str(exe)], check=True)
    basic, recs = golden_io.ddt_records()
    basic = np.ascontiguousarray(basic, np.uint64)
    cases = []
    for r in recs:
        cases.append(_case(r["name"], r["desc"].tobytes(), r["nrec"], r["size"], r["lb"], r["ub"], r["true_lb"],
                           r["true_ub"], basic, _golden_map(r, basic)))
    assert len(cases) == 18
    for klass in G.CLASSES:
        for seed in SEEDS:
            lay = G.layout(seed, klass)
            cases.append(_case(f"{klass}-{seed} ({lay.note})", lay.desc, lay.nrec, lay.size, lay.lb, lay.ub, lay.true_lb,
                               lay.true_ub, G.BASIC, lay.map))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"MXLAYC01" + struct.pack("<I", len(cases)))
        for c in cases:
            f.write(c)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert f"{len(cases)} cases" in r.stdout
