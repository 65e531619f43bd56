"""CPU: the binary16 slots (MPIX_SHORT_FLOAT, MPIX_C_SHORT_FLOAT_COMPLEX)
at the C-ABI and in the mini-host.

* the pattern under MX_TABLE_SHORT_FLOAT equals the reference's op tables
  expanded with HAVE_OPAL_SHORT_FLOAT_T and HAVE_OPAL_SHORT_FLOAT_COMPLEX_T
  set (tests/ref_optable.py's expansion; the recorded list is
  tests/golden/ref_optable_short_float.json, and a reference tree named by
  MX_REFERENCE_TREE is expanded and compared with it);
* table variants 0 and 1 and mx_type_size are what they were for all 41
  slots; mx_type_size_ex gives 2 and 4 under the flag;
* the mini-host's half <-> float conversions agree with numpy on all 65,536
  bit patterns, its base functions with numpy float16 on a few thousand
  operand pairs per op.

`python tests/test_short_float_host.py <reference tree>` rewrites the
recorded list."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import mxompi
import oracle_lib
import ref_optable
import short_float as sf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_optable_short_float.json")
SF = mxompi.TABLE_SHORT_FLOAT
SLOTS = {"SHORT_FLOAT": ("MAX", "MIN", "SUM", "PROD"), "C_SHORT_FLOAT_COMPLEX": ("SUM", "PROD")}


def _expand(ref, fortran, three):
    """The reference table's non-NULL pattern with the two short-float
    switches set, by ref_optable's own expansion under that configuration."""
    base = ref_optable.config

    def cfg(f):
        c = dict(base(f))
        c.update({"HAVE_OPAL_SHORT_FLOAT_T": 1, "HAVE_OPAL_SHORT_FLOAT_COMPLEX_T": 1})
        return c
    ref_optable.config = cfg
    try:
        return ref_optable.pattern_from_source(os.path.join(ref, ref_optable.SRC), fortran, three)
    finally:
        ref_optable.config = base


def _record(ref):
    return {"source": ref_optable.SRC,
            "switches": ["HAVE_OPAL_SHORT_FLOAT_T", "HAVE_OPAL_SHORT_FLOAT_COMPLEX_T"],
            "patterns": {ref_optable._key(f, t): sorted(_expand(ref, f, t)) for f in (0, 1) for t in (False, True)}}


def _golden(fortran, three):
    with open(GOLDEN) as f:
        return {tuple(p) for p in json.load(f)["patterns"][ref_optable._key(fortran, three)]}


@pytest.mark.parametrize("fortran", [0, 1])
def test_pattern_under_the_flag_equals_the_reference_tables(fortran):
    want = _golden(fortran, False)
    assert want == _golden(fortran, True)            # 2- and 3-buffer tables have one pattern
    ref = os.environ.get("MX_REFERENCE_TREE")
    if ref and os.path.isfile(os.path.join(ref, ref_optable.SRC)):
        for three in (False, True):
            assert _expand(ref, fortran, three) == want
    got = {(mxompi.OPS[op], mxompi.TYPES[t]) for op in range(15) for t in range(41)
           if mxompi.lib().mx_op_supported(op, t, fortran | SF)}
    assert got == want
    assert len(got) == (182 if fortran else 122)
    # exactly the six pairs on top of the plain variant
    assert got - ref_optable.pattern(fortran) == {(o, t) for t, ops in SLOTS.items() for o in ops}
    assert ref_optable.pattern(fortran) <= got


def test_plain_variants_and_type_size_are_unchanged():
    O = oracle_lib.oracle()
    L = mxompi.lib()
    for table in (mxompi.TABLE_C_ONLY, mxompi.TABLE_WITH_FORTRAN):
        for op in range(15):
            for t in range(41):
                assert bool(L.mx_op_supported(op, t, table)) == bool(O.mxo_supported(op, t, table))
        for t in SLOTS:
            for op in range(15):
                assert not mxompi.op_supported(op, t, table)
    for t in range(41):
        assert mxompi.type_size(t) == O.mxo_type_size(t)
        if mxompi.TYPES[t] not in SLOTS:
            for table in (0, 1, SF, 1 | SF):
                assert mxompi.type_size_ex(t, table) == mxompi.type_size(t)
    assert mxompi.type_size("SHORT_FLOAT") == 0 and mxompi.type_size("C_SHORT_FLOAT_COMPLEX") == 0


def test_type_size_ex():
    for table in (SF, mxompi.TABLE_WITH_FORTRAN | SF):
        assert mxompi.type_size_ex("SHORT_FLOAT", table) == 2
        assert mxompi.type_size_ex("C_SHORT_FLOAT_COMPLEX", table) == 4
    for table in (mxompi.TABLE_C_ONLY, mxompi.TABLE_WITH_FORTRAN):
        assert mxompi.type_size_ex("SHORT_FLOAT", table) == 0
        assert mxompi.type_size_ex("C_SHORT_FLOAT_COMPLEX", table) == 0
    assert mxompi.type_size_ex("MPIX_SHORT_FLOAT") == 2 and mxompi.type_size_ex("MPIX_C_FLOAT16") == 2
    assert mxompi.type_size_ex("MPIX_C_SHORT_FLOAT_COMPLEX") == 4


def test_decisions_use_the_two_byte_element():
    """AUTO decides by message size: the binary16 slots decide as the
    integer types of their size do."""
    for n in (2, 3, 5, 8):
        for count in (1, 13, 4099, 5000, 40003, 300001, 1 << 22):
            assert mxompi.allreduce_decision(n, count, "SHORT_FLOAT") == mxompi.allreduce_decision(n, count, "UINT16_T")
            assert mxompi.allreduce_decision(n, count, "C_SHORT_FLOAT_COMPLEX") == \
                mxompi.allreduce_decision(n, count, "UINT32_T")
            assert mxompi.reduce_scatter_decision(n, count, "SHORT_FLOAT") == \
                mxompi.reduce_scatter_decision(n, count, "UINT16_T")


def test_slots_are_accepted_without_a_device():
    """count 0 returns before any device work: the slots are no longer
    MX_ERR_UNSUPPORTED, ops outside their rows still are."""
    L = mxompi.lib()
    for t, ops in SLOTS.items():
        for op in range(1, 13):
            rc = L.mx_reduce2(op, mxompi.TYPE[t], None, None, 0, None)
            assert rc == (0 if mxompi.OPS[op] in ops else -2), (mxompi.OPS[op], t)
            rc = L.mx_reduce3(op, mxompi.TYPE[t], None, None, None, 0, None)
            assert rc == (0 if mxompi.OPS[op] in ops else -2), (mxompi.OPS[op], t)


# ---- the mini-host's plain-C binary16 -------------------------------------
def _host_lib():
    H = ctypes.CDLL(os.path.join(mxompi.LIB_DIR, "libmx_host.so"))
    H.mxh_half_to_float.restype = ctypes.c_float
    H.mxh_half_to_float.argtypes = [ctypes.c_uint16]
    H.mxh_float_to_half.restype = ctypes.c_uint16
    H.mxh_float_to_half.argtypes = [ctypes.c_float]
    H.mxh_short_float_reduce.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_size_t]
    return H


def test_host_conversions_agree_with_numpy_on_every_pattern():
    H = _host_lib()
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    want = allh.view(np.float16).astype(np.float32)
    got = np.array([H.mxh_half_to_float(int(h)) for h in allh], dtype=np.float32)
    nan = np.isnan(want)
    assert nan.sum() == 2 * 1023
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    # NaN: sign and payload kept (numpy may or may not set the quiet bit)
    q = np.uint32(0x00400000)
    np.testing.assert_array_equal(got.view(np.uint32)[nan] | q, want.view(np.uint32)[nan] | q)
    # float -> half: every binary16 value comes back, a NaN stays a NaN of its sign
    back = np.array([H.mxh_float_to_half(float(x)) for x in want], dtype=np.uint16)
    np.testing.assert_array_equal(back[~nan], allh[~nan])
    assert ((back[nan] & 0x7C00) == 0x7C00).all() and ((back[nan] & 0x03FF) != 0).all()
    np.testing.assert_array_equal(back[nan] & 0x8000, allh[nan] & 0x8000)
    # rounding: ties, the subnormal range, overflow, on floats that are no binary16 values
    rng = np.random.default_rng(16)
    x = np.concatenate([
        rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),
        (rng.uniform(-1, 1, 20000) * 2.0 ** rng.uniform(-27, 17, 20000)).astype(np.float32),
        # exact ties between neighbouring binary16 values, normal and subnormal
        ((allh[:0x7BFF].view(np.float16).astype(np.float64) +
          allh[1:0x7C00].view(np.float16).astype(np.float64)) / 2).astype(np.float32),
        np.array([65504.0, 65519.99, 65520.0, 65536.0, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), 1),
                  2.0 ** -24, 2.0 ** -26, -2.0 ** -25, 0.0, -0.0, np.inf, -np.inf], np.float32)])
    x = x[~np.isnan(x)]
    with np.errstate(all="ignore"):
        want16 = x.astype(np.float16).view(np.uint16)
    got16 = np.array([H.mxh_float_to_half(float(v)) for v in x], dtype=np.uint16)
    np.testing.assert_array_equal(got16, want16)


@pytest.mark.parametrize("t,op", [(t, o) for t, ops in SLOTS.items() for o in ops])
def test_host_base_functions_agree_with_numpy(t, op):
    H = _host_lib()
    n = 4000
    a, b = sf.gen(op, t, n, 1), sf.gen(op, t, n, 2)
    if t == "C_SHORT_FLOAT_COMPLEX" and op == "PROD":
        a[:2], b[:2] = sf.DISTINGUISHING[0], sf.DISTINGUISHING[1]
    # 2-buffer: inout = inout OP in (x = inout, y = in)
    io = b.copy()
    assert H.mxh_short_float_reduce(mxompi.OP[op], mxompi.TYPE[t], a.ctypes.data, None, io.ctypes.data, n) == 0
    sf.assert_equal(op, io, sf.ref(op, t, b, a), f"host 2-buffer {op} {t}")
    # 3-buffer: out = in1 OP in2
    out = np.zeros_like(a)
    assert H.mxh_short_float_reduce(mxompi.OP[op], mxompi.TYPE[t], a.ctypes.data, b.ctypes.data, out.ctypes.data,
                                    n) == 0
    sf.assert_equal(op, out, sf.ref(op, t, a, b), f"host 3-buffer {op} {t}")
    if t == "C_SHORT_FLOAT_COMPLEX" and op == "PROD":
        np.testing.assert_array_equal(io[:2], sf.DISTINGUISHING[2])
        np.testing.assert_array_equal(out[:2], sf.DISTINGUISHING[2])
    assert H.mxh_short_float_reduce(mxompi.OP["BAND"], mxompi.TYPE[t], a.ctypes.data, None, io.ctypes.data, n) == -1


def test_oracle_helper_distinguishes_the_two_complex_products():
    a, b, want = sf.DISTINGUISHING
    np.testing.assert_array_equal(sf.ref("PROD", "C_SHORT_FLOAT_COMPLEX", b, a), want)
    f = lambda u: u.view(np.float16).astype(np.float32)      # noqa: E731
    wide = np.array([f(a)[0] * f(b)[0] - f(a)[1] * f(b)[1], f(a)[0] * f(b)[1] + f(a)[1] * f(b)[0]], np.float32)
    np.testing.assert_array_equal(wide.astype(np.float16).view(np.uint16), np.array([0x4843, 0x3800], np.uint16))


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(_record(sys.argv[1]), f, indent=1)
        f.write("\n")
