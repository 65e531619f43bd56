"""Adversarial operands for every (op, type) pair (TEST INFRASTRUCTURE).

pairs()        the 176 (op, type) names of the Fortran-enabled table;
edge_values()  `count` elements of one operand, the mix oracle/gen_op_golden.c
               documents, for any count and any pair;
inputs() / expected()
               the per-rank operands of a collective case and the oracle's
               results for it, computed once per case and shared (read-only)
               by the host and GPU pair-matrix tests.

The mix, per component:
  * integers: raw bits, small values -3..3, and 0 / 1 / all-ones / MIN / MAX
    of the width; BOOL 0/1 only; LOGICAL mostly 0/1/2;
  * float, double, x87 long double and their complex types: SUM (and MAX/MIN)
    magnitudes over 16 decades, PROD in +-[0.5, 2), 10 % small-integer ties,
    the rest specials (NaN of both signs, +-inf, +-0, the smallest subnormal,
    half the smallest normal, +-max, the smallest normal; signalling NaNs for
    the selecting ops).  x87 values carry all 64 significand bits, random
    bytes in the padding, and among the specials the x87-only encodings
    (denormal, pseudo-denormal, unnormal, pseudo-NaN, pseudo-infinity);
  * pair types: few distinct values (ties across operands are common), +-0,
    small indices with some raw ints, NaN about 1 in 16 for FP values,
    random bytes in the struct gaps.

Special density.  MAX, MIN, MAXLOC, MINLOC and the integer ops are compared
bit for bit, so about 20 % of their components are specials; every 8th
element (the same positions in every operand) is drawn from a six-value
clash set (+-0, +-NaN, a signalling NaN, 1) so that NaN-vs-number and
+0-vs--0 meet at the same element of two operands.  Floating-point SUM/PROD
results only have to be NaN where the oracle's are, so a NaN-flooded result
would hide a wrong kernel: their special rate is 1 in 128 per component
(x87: 1 in 256, and 1 in 512 more for the x87-only encodings, three of
which are invalid operands and so NaN results; the 32-byte complex type is
also folded over 16 ranks), which keeps the NaN share of the oracle's
results under 10 % for every case the GPU tests use
(tests/test_pair_matrix_host.py asserts it).  The first 8 elements of a
SUM/PROD operand are never special: a one-element case whose result is NaN
would leave nothing to compare.
"""
import ctypes
import functools
import json
import os

import numpy as np

import mxompi
import oracle_lib

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_optable.json")

F4 = ("FLOAT", "REAL", "REAL4")
F8 = ("DOUBLE", "REAL8", "DOUBLE_PRECISION")
FP_COMPONENT = {**{t: ("f4", 1) for t in F4}, **{t: ("f8", 1) for t in F8}, "LONG_DOUBLE": ("ld", 1),
                "C_FLOAT_COMPLEX": ("f4", 2), "C_DOUBLE_COMPLEX": ("f8", 2), "C_LONG_DOUBLE_COMPLEX": ("ld", 2)}
# pair layouts (op.h pair structs, x86-64): value format, index format, index offset
PAIR = {"FLOAT_INT": ("f4", "i4", 4), "DOUBLE_INT": ("f8", "i4", 8), "LONG_INT": ("i8", "i4", 8),
        "2INT": ("i4", "i4", 4), "2INTEGER": ("i4", "i4", 4), "SHORT_INT": ("i2", "i4", 4),
        "LONG_DOUBLE_INT": ("ld", "i4", 16), "2REAL": ("f4", "f4", 4), "2DOUBLE_PRECISION": ("f8", "f8", 8)}
SELECTING = ("MAX", "MIN", "MAXLOC", "MINLOC")


@functools.lru_cache(maxsize=None)
def pairs():
    """The (op, type) names the product supports under the Fortran-enabled
    table: 176, the set of the reference's table."""
    got = [(op, t) for op in mxompi.OPS for t in mxompi.TYPES
           if mxompi.op_supported(op, t, mxompi.TABLE_WITH_FORTRAN)]
    with open(_GOLDEN) as f:
        ref = {tuple(p) for p in json.load(f)["patterns"]["with_fortran/2buff"]}
    assert len(got) == 176, len(got)
    assert set(got) == ref, sorted(set(got) ^ ref)
    return tuple(got)


def is_fp_arith(op, t):
    """Floating-point SUM/PROD: compared up to the NaN payload."""
    return op in ("SUM", "PROD") and t in FP_COMPONENT


# ---- integers ---------------------------------------------------------------
def _int_words(rng, n, bits, kind="int"):
    """n uint64 words whose low `bits` bits are the value."""
    if kind == "bool":
        return rng.integers(0, 2, n).astype(np.uint64)
    raw = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    small = rng.integers(-3, 4, n).astype(np.int64).view(np.uint64)
    ext = np.array([0, 1, 0xFFFFFFFFFFFFFFFF, (1 << (bits - 1)) - 1, 1 << (bits - 1)], np.uint64)[rng.integers(0, 5, n)]
    r = rng.integers(0, 100, n)
    v = np.where(r < 60, raw, np.where(r < 75, small, ext))
    if kind == "logical":
        v = np.where(rng.integers(0, 2, n) == 0, rng.integers(0, 3, n).astype(np.uint64), v)
    return v


def _low_bytes(words, nbytes):
    return np.ascontiguousarray(words.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :nbytes])


# ---- float / double ---------------------------------------------------------
_IEEE = {"f4": (np.float32, np.uint32, 23, 8), "f8": (np.float64, np.uint64, 52, 11)}


def _ieee_specials(fmt):
    """(the SUM/PROD list, the selecting ops' list, the clash set) as bit patterns."""
    ft, ut, mb, eb = _IEEE[fmt]
    sign = 1 << (mb + eb)
    emax = ((1 << eb) - 1) << mb
    qnan, snan, inf = emax | (1 << (mb - 1)), emax | (1 << (mb - 2)) | 1, emax
    vmax, tiny, half_tiny, sub = emax - 1, 1 << mb, 1 << (mb - 1), 1
    one = ((1 << (eb - 1)) - 1) << mb
    arith = [qnan, sign | qnan, inf, sign | inf, 0, sign, sub, sign | sub, half_tiny, vmax, sign | vmax, tiny]
    select = arith + [snan, sign | snan]
    clash = [0, sign, qnan, sign | qnan, snan, one]
    return [np.array(x, ut) for x in (arith, select, clash)]


def _ieee_components(rng, k, op, fmt, stripe, plain):
    """k components as raw bits; stripe = boolean mask of the clash positions."""
    ft, ut, _, _ = _IEEE[fmt]
    if op == "PROD":
        v = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
    else:
        v = rng.uniform(-1, 1, k) * 10.0 ** rng.uniform(-8, 8, k)
    bits = v.astype(ft).view(ut).copy()
    ties = rng.integers(-3, 4, k).astype(ft).view(ut)
    arith, select, clash = _ieee_specials(fmt)
    dense = op not in ("SUM", "PROD")
    spec = select if dense else arith
    rate = 0.10 if dense else 1.0 / 128
    r = rng.random(k)
    if not dense:
        r[:plain] = 0.99
    bits = np.where(r < 0.10, ties, bits)
    bits = np.where((r >= 0.10) & (r < 0.10 + rate), spec[rng.integers(0, len(spec), k)], bits)
    if dense:
        bits = np.where(stripe, clash[rng.integers(0, len(clash), k)], bits)
    return bits.astype(ut)


# ---- x87 long double --------------------------------------------------------
_B63 = np.uint64(1 << 63)


def _x87_small(vals):
    """Small numbers as (significand, sign+exponent) of an x87 long double."""
    b = np.ascontiguousarray(np.asarray(vals).astype(np.longdouble)).view(np.uint8).reshape(-1, 16)
    return (np.ascontiguousarray(b[:, :8]).view(np.uint64).ravel().copy(),
            np.ascontiguousarray(b[:, 8:10]).view(np.uint16).ravel().copy())


def _x87_specials(rng, k, dense):
    qn, sn = 0xC000000000000000, 0xA000000000000001
    table = [(qn, 0x7FFF), (qn, 0xFFFF), (1 << 63, 0x7FFF), (1 << 63, 0xFFFF), (0, 0), (0, 0x8000), (1, 0),
             (1, 0x8000), (1 << 62, 0), (0xFFFFFFFFFFFFFFFF, 0x7FFE), (0xFFFFFFFFFFFFFFFF, 0xFFFE), (1 << 63, 1)]
    if dense:
        table += [(sn, 0x7FFF), (sn, 0xFFFF)]
    j = rng.integers(0, len(table), k)
    m = np.array([x[0] for x in table], np.uint64)[j]
    se = np.array([x[1] for x in table], np.uint16)[j]
    return m, se


def _x87_only(rng, k):
    """The encodings only the 80-bit format has (tests/native/x87_check.cpp
    cases 1, 10, 11): denormal, pseudo-denormal, unnormal, pseudo-NaN,
    pseudo-infinity, either sign."""
    raw = rng.integers(0, 1 << 64, k, dtype=np.uint64)
    sh = rng.integers(1, 64, k).astype(np.uint64)
    sign = (rng.integers(0, 2, k) << 15).astype(np.uint16)
    e_mid = rng.integers(1, 0x7FFF, k).astype(np.uint16)
    kind = rng.integers(0, 5, k)
    m = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                  [raw >> sh, raw | _B63, (raw >> np.uint64(1)) >> (sh * (raw & np.uint64(1))),
                   (raw >> np.uint64(1)) | np.uint64(1)], np.uint64(0))
    se = np.select([kind <= 1, kind == 2], [np.uint16(0), e_mid], np.uint16(0x7FFF)).astype(np.uint16) | sign
    return m.astype(np.uint64), se


# a few fixed full-significand values: ties between operands for the x87 pair type
_X87_POOL = (np.array([0xC90FDAA22168C235, 0xADF85458A2BB4A9B, 0xB504F333F9DE6485, 0xC90FDAA22168C234], np.uint64),
             np.array([0x4000, 0xC000, 0x3FFF, 0x4000], np.uint16))


def _x87_components(rng, k, op, stripe, plain):
    """k long doubles as (significand, sign+exponent)."""
    m = rng.integers(0, 1 << 64, k, dtype=np.uint64) | _B63        # all 64 significand bits
    if op == "PROD":
        e = rng.integers(16382, 16384, k)                          # [0.5, 2)
    else:
        e = 16383 + rng.integers(-27, 28, k)                       # 16 decades
    se = (e | (rng.integers(0, 2, k) << 15)).astype(np.uint16)
    dense = op not in ("SUM", "PROD")
    r = rng.random(k)
    if not dense:
        r[:plain] = 0.99
    tm, tse = _x87_small(rng.integers(-3, 4, k))
    sm, sse = _x87_specials(rng, k, dense)
    om, ose = _x87_only(rng, k)
    rate, only = (0.07, 0.03) if dense else (1.0 / 256, 1.0 / 512)
    for lo, hi, am, ase in ((0.0, 0.10, tm, tse), (0.10, 0.10 + rate, sm, sse),
                            (0.10 + rate, 0.10 + rate + only, om, ose)):
        sel = (r >= lo) & (r < hi)
        m, se = np.where(sel, am, m), np.where(sel, ase, se)
    if dense:
        cm = np.array([0, 0, 0xC000000000000000, 0xC000000000000000, 0xA000000000000001, 1 << 63], np.uint64)
        cse = np.array([0, 0x8000, 0x7FFF, 0xFFFF, 0x7FFF, 0x3FFF], np.uint16)
        j = rng.integers(0, 6, k)
        m, se = np.where(stripe, cm[j], m), np.where(stripe, cse[j], se)
    return m.astype(np.uint64), se.astype(np.uint16)


def _x87_store(rows, col, m, se):
    """Write long doubles into bytes col..col+9 of each row (the 6 bytes after stay)."""
    rows[:, col:col + 8] = _low_bytes(m, 8)
    rows[:, col + 8:col + 10] = _low_bytes(se.astype(np.uint64), 2)


# ---- pair types -------------------------------------------------------------
def _pair_rows(rng, n, t, es):
    vf, kf, koff = PAIR[t]
    rows = rng.integers(0, 256, (n, es), dtype=np.uint8)            # struct gaps and x87 padding: random
    k = np.where(rng.integers(0, 4, n) == 0, rng.integers(-(1 << 31), 1 << 31, n), rng.integers(-4, 5, n))
    nan = rng.integers(0, 16, n) == 0
    nsign = rng.integers(0, 2, n) == 0
    if vf in ("f4", "f8"):
        ft, ut, mb, eb = _IEEE[vf]
        v = np.array([-1.0, -0.0, 0.0, 1.0, 2.0], ft)[rng.integers(0, 5, n)].view(ut)
        qnan = (((1 << eb) - 1) << mb) | (1 << (mb - 1))
        v = np.where(nan, np.where(nsign, ut(qnan), ut(qnan | (1 << (mb + eb)))), v).astype(ut)
        rows[:, :v.itemsize] = v.view(np.uint8).reshape(n, -1)
    elif vf == "ld":
        sm, sse = _x87_small(np.array([-1.0, -0.0, 0.0, 1.0, 2.0])[rng.integers(0, 5, n)])
        j = rng.integers(0, len(_X87_POOL[0]), n)
        om, ose = _x87_only(rng, n)
        r = rng.random(n)
        m = np.where(r < 0.20, _X87_POOL[0][j], np.where(r < 0.25, om, sm))
        se = np.where(r < 0.20, _X87_POOL[1][j], np.where(r < 0.25, ose, sse))
        m = np.where(nan, np.uint64(0xC000000000000000), m)
        se = np.where(nan, np.where(nsign, np.uint16(0x7FFF), np.uint16(0xFFFF)), se)
        _x87_store(rows, 0, m.astype(np.uint64), se.astype(np.uint16))
    else:
        nb = int(vf[1])
        small = rng.integers(-1, 3, n).astype(np.int64).view(np.uint64)
        v = np.where(rng.integers(0, 8, n) == 0, rng.integers(0, 1 << 64, n, dtype=np.uint64), small)
        rows[:, :nb] = _low_bytes(v, nb)
    if kf == "i4":
        rows[:, koff:koff + 4] = _low_bytes(k.astype(np.int64).view(np.uint64), 4)
    else:
        kv = k.astype(np.float32 if kf == "f4" else np.float64)
        rows[:, koff:koff + kv.itemsize] = kv.view(np.uint8).reshape(n, -1)
    return rows


def edge_values(op, t, count, seed):
    """`count` elements of type t as bytes (np.uint8[count * es]), adversarial
    for `op`; deterministic per (op, t, count, seed)."""
    es = mxompi.type_size(t)
    rng = np.random.default_rng([int(seed), mxompi.OP[op], mxompi.TYPE[t]])
    if t in PAIR:
        return _pair_rows(rng, count, t, es).ravel()
    if t in FP_COMPONENT:
        fmt, nc = FP_COMPONENT[t]
        k = count * nc
        stripe = (np.arange(k) // nc) % 8 == 5
        plain = 8 * nc    # SUM/PROD: no specials in the first 8 elements
        if fmt == "ld":
            rows = rng.integers(0, 256, (k, 16), dtype=np.uint8)    # padding bytes: random
            m, se = _x87_components(rng, k, op, stripe, plain)
            _x87_store(rows, 0, m, se)
            return rows.ravel()
        return _ieee_components(rng, k, op, fmt, stripe, plain).view(np.uint8).copy()
    kind = {"BOOL": "bool", "LOGICAL": "logical"}.get(t, "int")
    return _low_bytes(_int_words(rng, count, 8 * es, kind), es).ravel()


# ---- shared cases: operands and the oracle's results ------------------------
vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
ALLREDUCE = {"auto": 0, "recursive_doubling": 3, "ring": 4, "rabenseifner": 6}
PREFILL = 0xA5


@functools.lru_cache(maxsize=None)
def _oracle():
    L = oracle_lib.oracle()
    pv = ctypes.POINTER(vp)
    L.mxo_allreduce.argtypes = [ci, ci, ci, ci, sz, pv, pv]
    L.mxo_reduce_scatter.argtypes = [ci, ci, ci, ci, ctypes.POINTER(sz), pv, pv]
    L.mxo_reduce.argtypes = [ci, ci, ci, ci, sz, ci, pv, vp]
    L.mxo_scan.argtypes = [ci, ci, ci, ci, sz, pv, pv]
    L.mxo_exscan.argtypes = [ci, ci, ci, ci, sz, pv, pv]
    L.mxo_reduce_scatter_block.argtypes = [ci, ci, ci, ci, sz, pv, pv]
    return L


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def inputs(op, t, n, count, base=0):
    """The n ranks' operands of a case: edge_values(op, t, count, base + rank), read-only."""
    return _frozen([edge_values(op, t, count, base + r) for r in range(n)])


def _ptrs(arrays):
    return (vp * len(arrays))(*[a.ctypes.data for a in arrays])


@functools.lru_cache(maxsize=None)
def expected(kind, alg, n, count, op, t, root=0, base=0):
    """The oracle's result buffers (one per rank, read-only) of a collective
    over inputs(): kind is allreduce | reduce_scatter | reduce | scan |
    exscan | reduce_scatter_block; alg the product's algorithm name.
    Buffers start at the 0xA5 prefill, so bytes the algorithm does not write
    (exscan's rank 0, the non-root ranks of a reduce) show it.  `count` is
    the per-rank element count (reduce_scatter: rcounts = count + 3 * rank)."""
    L = _oracle()
    o, ty, es = mxompi.OP[op], mxompi.TYPE[t], mxompi.type_size(t)
    if kind == "reduce_scatter":
        rc = [count + 3 * r for r in range(n)]
        xs = inputs(op, t, n, sum(rc), base)
        out = [np.full(c * es, PREFILL, np.uint8) for c in rc]
        rc_ = L.mxo_reduce_scatter(mxompi.REDUCE_SCATTER[alg], o, ty, n, (sz * n)(*rc), _ptrs(xs), _ptrs(out))
    elif kind == "reduce_scatter_block":
        xs = inputs(op, t, n, count * n, base)
        out = [np.full(count * es, PREFILL, np.uint8) for _ in range(n)]
        rc_ = L.mxo_reduce_scatter_block(mxompi.REDUCE[alg], o, ty, n, count, _ptrs(xs), _ptrs(out))
    else:
        xs = inputs(op, t, n, count, base)
        out = [np.full(count * es, PREFILL, np.uint8) for _ in range(n)]
        if kind == "allreduce":
            rc_ = L.mxo_allreduce(ALLREDUCE[alg], o, ty, n, count, _ptrs(xs), _ptrs(out))
        elif kind == "reduce":
            rc_ = L.mxo_reduce(mxompi.REDUCE[alg], o, ty, n, count, root, _ptrs(xs), out[root].ctypes.data)
        else:
            fn = L.mxo_scan if kind == "scan" else L.mxo_exscan
            rc_ = fn(mxompi.SCAN[alg], o, ty, n, count, _ptrs(xs), _ptrs(out))
    assert rc_ == 0, (kind, alg, n, count, op, t, rc_)
    return _frozen(out)


# The cases of tests/test_pair_matrix_gpu.py, as (kind, alg, n, count, root):
# the host test checks the generator's conditions on exactly these.
FOLD_CASES = ([("allreduce", alg, 5, c, 0) for alg in ("ring", "recursive_doubling", "rabenseifner")
               for c in (1, 1031)] + [("reduce_scatter", "ring", 5, 37, 0)])
VM_CASES = [case for c in (1, 1031) for case in
            (("reduce", "binomial", 5, c, 4), ("reduce", "in_order_binary", 5, c, 0),
             ("scan", "recursive_doubling", 5, c, 0), ("exscan", "linear", 5, c, 0),
             ("reduce_scatter_block", "binomial", 5, c, 0))]
# 32-byte elements x 16 ranks: past the default LDS limit of the VM fold
VM16_PAIRS = (("SUM", "C_LONG_DOUBLE_COMPLEX"), ("PROD", "C_LONG_DOUBLE_COMPLEX"),
              ("MAXLOC", "LONG_DOUBLE_INT"), ("MINLOC", "LONG_DOUBLE_INT"))
VM16_CASES = [("reduce", "binomial", 16, 257, 4), ("scan", "recursive_doubling", 16, 257, 0)]
ONESHOT_BASE = 7000                    # edge_values(op, t, count, 7000 + rank)
ONESHOT_BYTES = (0, 2048, 12288)       # one element; inside the tagged-word limit (4 KiB); several workgroups
SERVICE_COUNT = 4099


def oneshot_counts(t):
    es = mxompi.type_size(t)
    return [max(1, nb // es) for nb in ONESHOT_BYTES]


def nan_share(buf, t):
    """Fraction of the elements of a result buffer of FP type t that hold a NaN component."""
    import golden_io
    _, nan = golden_io._components(np.ascontiguousarray(buf), mxompi.TYPE[t])
    nc = FP_COMPONENT[t][1]
    return float(nan.reshape(-1, nc).any(axis=1).mean())
