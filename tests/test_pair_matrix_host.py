"""CPU: the conditions the pair-matrix GPU tests rest on.

tests/test_pair_matrix_gpu.py runs every (op, type) pair through every device
consumer on operands from op_values.edge_values and compares with the oracle.
That comparison only means something if the operands are adversarial in the
ways checked here, on the oracle alone (no GPU):

  * the pair list is the reference table's 176;
  * floating-point SUM/PROD results are compared up to the NaN payload, so at
    most 10 % of the oracle's elements of any such case may be NaN (a case
    of one element: none), and ring and recursive doubling must differ on at
    least 40 non-NaN elements of 1031 (a fold that associates wrongly cannot
    pass);
  * MAX/MIN/MAXLOC/MINLOC operands hold NaNs and both zeros (FP), meet as
    +0 against -0 at one element of two ranks (FP), tie on the value with
    different indices (LOC), and for FP values swapping the operand roles of
    mxo_reduce2 changes the result (for integer values MAX, MIN and the LOC
    ops are commutative, index tie-break included: no role to observe);
  * the generator is deterministic per seed.
"""
import numpy as np
import pytest

import golden_io
import mxompi
import op_values as ov
import oracle_lib

PAIRS = ov.pairs()
FP_ARITH = [p for p in PAIRS if ov.is_fp_arith(*p)]
SELECT = [p for p in PAIRS if p[0] in ov.SELECTING]
_ids = lambda p: f"{p[0]}-{p[1]}"   # noqa: E731


def test_pairs_are_the_reference_table():
    assert len(PAIRS) == 176 and len(set(PAIRS)) == 176
    import ref_optable
    assert set(PAIRS) == ref_optable.pattern(True)
    assert len(FP_ARITH) == 20 and len(SELECT) == 2 * 20 + 2 * 9


def test_edge_values_deterministic_and_sized():
    for op, t in PAIRS:
        es = mxompi.type_size(t)
        for count in (1, 37, 1031):
            a, b = ov.edge_values(op, t, count, 11), ov.edge_values(op, t, count, 11)
            assert a.dtype == np.uint8 and a.shape == (count * es,)
            np.testing.assert_array_equal(a, b)
        assert not np.array_equal(ov.edge_values(op, t, 1031, 11), ov.edge_values(op, t, 1031, 12))
    for op in ("LAND", "LOR", "LXOR"):
        assert ov.edge_values(op, "BOOL", 1031, 3).max() == 1
        lg = ov.edge_values(op, "LOGICAL", 1031, 3).view(np.uint32)
        assert (lg <= 2).mean() > 0.5 and (lg > 2).any()


def _cap(bufs, t, what):
    for r, b in enumerate(bufs):
        share = ov.nan_share(b, t)
        n = len(b) // mxompi.type_size(t)
        assert share <= (0.10 if n > 1 else 0.0), f"{what} rank {r}: {share:.3f} of {n} elements NaN"


@pytest.mark.parametrize("op,t", FP_ARITH, ids=map(_ids, FP_ARITH))
def test_nan_cap_of_every_fp_arith_case(op, t):
    for kind, alg, n, count, root in ov.FOLD_CASES + ov.VM_CASES + (ov.VM16_CASES if (op, t) in ov.VM16_PAIRS else []):
        exp = ov.expected(kind, alg, n, count, op, t, root)
        if kind == "reduce":
            exp = [exp[root]]
        elif kind == "exscan":
            exp = exp[1:]
        _cap(exp, t, f"{kind} {alg} n={n} count={count}")
    for n in (2, 3):
        for count in ov.oneshot_counts(t):
            _cap(ov.expected("allreduce", "auto", n, count, op, t, 0, ov.ONESHOT_BASE), t, f"one-shot n={n} {count}")
    O = oracle_lib.oracle()
    a, b = ov.inputs(op, t, 2, ov.SERVICE_COUNT, 100)
    out = b.copy()
    assert O.mxo_reduce2(mxompi.OP[op], mxompi.TYPE[t], a.ctypes.data, out.ctypes.data, ov.SERVICE_COUNT, 1) == 0
    _cap([out], t, "reduce2")


def _differing(a, b, t):
    """Elements whose non-NaN values differ."""
    va, na = golden_io._components(np.ascontiguousarray(a), mxompi.TYPE[t])
    vb, nb = golden_io._components(np.ascontiguousarray(b), mxompi.TYPE[t])
    d = (va != vb).any(axis=1) if va.ndim == 2 else va != vb
    d = d & ~na & ~nb
    return int(d.reshape(-1, ov.FP_COMPONENT[t][1]).any(axis=1).sum())


@pytest.mark.parametrize("op,t", FP_ARITH, ids=map(_ids, FP_ARITH))
def test_fold_order_shows_in_the_values(op, t):
    ring = ov.expected("allreduce", "ring", 5, 1031, op, t)
    rd = ov.expected("allreduce", "recursive_doubling", 5, 1031, op, t)
    assert _differing(ring[0], rd[0], t) >= 40


def _values(buf, t):
    """(value bits as a sortable key, isnan, is +0, is -0, index) per element of a selecting pair's operand."""
    es = mxompi.type_size(t)
    rows = buf.reshape(-1, es)
    fmt = ov.PAIR[t][0] if t in ov.PAIR else ov.FP_COMPONENT.get(t, (None,))[0]
    idx = None
    if t in ov.PAIR:
        ko = ov.PAIR[t][2]
        idx = np.ascontiguousarray(rows[:, ko:ko + (8 if ov.PAIR[t][1] == "f8" else 4)])
    if fmt in ("f4", "f8"):
        nb = 4 if fmt == "f4" else 8
        v = np.ascontiguousarray(rows[:, :nb]).view(np.float32 if fmt == "f4" else np.float64).ravel()
        return rows[:, :nb], np.isnan(v), (v == 0) & ~np.signbit(v), (v == 0) & np.signbit(v), idx
    if fmt == "ld":
        m = np.ascontiguousarray(rows[:, :8]).view(np.uint64).ravel()
        se = np.ascontiguousarray(rows[:, 8:10]).view(np.uint16).ravel()
        nan = ((se & 0x7FFF) == 0x7FFF) & ((m << np.uint64(1)) != 0)
        return rows[:, :10], nan, (m == 0) & (se == 0), (m == 0) & (se == 0x8000), idx
    return rows[:, :int(fmt[1])] if fmt else rows, None, None, None, idx


@pytest.mark.parametrize("op,t", SELECT, ids=map(_ids, SELECT))
def test_selecting_ops_see_nan_zero_pairs_and_ties(op, t):
    xs = ov.inputs(op, t, 5, 1031)
    parts = [_values(x, t) for x in xs]
    fp = parts[0][1] is not None
    for r, (val, nan, pz, nz, idx) in enumerate(parts):
        if fp:
            assert nan.any() and pz.any() and nz.any(), (r, int(nan.sum()), int(pz.sum()), int(nz.sum()))
    for r in range(4):
        (va, _, pza, nza, ia), (vb, _, pzb, nzb, ib) = parts[r], parts[r + 1]
        if fp:
            assert ((pza & nzb) | (nza & pzb)).any(), f"no +0 against -0 between ranks {r} and {r + 1}"
        if idx is not None:
            tie = (va == vb).all(axis=1) & (ia != ib).any(axis=1)
            assert tie.sum() >= 8, (r, int(tie.sum()))
    if fp:
        O = oracle_lib.oracle()
        a, b = xs[0], xs[1]
        ab, ba = b.copy(), a.copy()
        assert O.mxo_reduce2(mxompi.OP[op], mxompi.TYPE[t], a.ctypes.data, ab.ctypes.data, 1031, 1) == 0
        assert O.mxo_reduce2(mxompi.OP[op], mxompi.TYPE[t], b.ctypes.data, ba.ctypes.data, 1031, 1) == 0
        assert not np.array_equal(golden_io.data_bytes(ab, mxompi.TYPE[t]), golden_io.data_bytes(ba, mxompi.TYPE[t]))
