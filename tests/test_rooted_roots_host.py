"""CPU: the conditions tests/test_rooted_roots_mp_gpu.py rests on, on the oracle alone.

The device test runs rooted reductions at every root, in place at the root
and not, and compares with the oracle bit for bit.  It observes the root's
MPI_IN_PLACE bit (the guarded instructions of the part owners' programs) and
the root itself only if the oracle's two variants, and two neighbouring
roots, give different bytes on the operands it uses,
op_values.inputs(op, t, n, 1031).  Asserted here, with a floor of 50 of 1031
elements:

  * in place against out of place, every root, n = 3, 5, 8:
    (MAXLOC, FLOAT_INT) on libnbc's chain and on coll/base's chain, pipeline,
    binary and binomial; (MAX, FLOAT) on libnbc's chain and on the pipeline
    (the deep trees).  (MAX, FLOAT) on coll/base's chain, binary and binomial
    changes only 2..31 elements -- MAX's operand roles show only where a NaN
    or +0 against -0 meets at the root's last combination -- so the device
    test reads the bit there through (MAXLOC, FLOAT_INT), whose index tie-break
    depends on the roles at every tie of the value;
  * the in-order binary tree is rooted at n - 1 whatever the root: the variants
    differ (by the floor, for MAXLOC) for root n - 1 only and are the same
    bytes for every other root;
  * root r against root (r + 1) mod n, (MAX, FLOAT), out of place: every
    algorithm whose tree depends on the root;
  * where the variants coincide exactly: linear, libnbc's binomial; and SUM and
    PROD of every real and complex type on every algorithm (IEEE and x87
    addition and multiplication commute; compared as the device test
    compares, up to the NaN payload -- the bytes of a NaN result do differ).
    Linear and in-order binary give the same bytes at every root;
  * the chunked call of the device test (100003 elements): the floor holds in
    every stretch of 1031 elements, so in every chunk.
"""
import numpy as np
import pytest

import golden_io
import mxompi
import op_values as ov
from rooted_roots_util import COUNT, IREDUCE_ALGS, NS, REDUCE_ALGS, rooted

FLOOR = 50
MAXF, MAXLOC = ("MAX", "FLOAT"), ("MAXLOC", "FLOAT_INT")
# (kind, alg, pairs whose two variants must differ by the floor at every root)
BIT_OBSERVED = [("ireduce", "chain", (MAXF, MAXLOC)), ("reduce", "pipeline", (MAXF, MAXLOC)),
                ("reduce", "chain", (MAXLOC,)), ("reduce", "binary", (MAXLOC,)), ("reduce", "binomial", (MAXLOC,))]
ROOT_OBSERVED = [("ireduce", "chain"), ("ireduce", "binomial"), ("reduce", "chain"), ("reduce", "pipeline"),
                 ("reduce", "binary"), ("reduce", "binomial")]


def _differing(a, b, t):
    """elements of which any data byte differs"""
    T = mxompi.TYPE[t]
    a, b = golden_io.data_bytes(a, T), golden_io.data_bytes(b, T)
    return int((a.reshape(COUNT, -1) != b.reshape(COUNT, -1)).any(axis=1).sum())


@pytest.mark.parametrize("n", NS)
def test_the_inplace_bit_shows_at_every_root(n):
    for kind, alg, prs in BIT_OBSERVED:
        for op, t in prs:
            for root in range(n):
                d = _differing(rooted(kind, alg, n, COUNT, op, t, root, True),
                               rooted(kind, alg, n, COUNT, op, t, root, False), t)
                assert d >= FLOOR, (kind, alg, op, t, n, root, d)


@pytest.mark.parametrize("n", NS)
def test_in_order_binary_depends_on_the_bit_at_root_n_minus_1_only(n):
    for op, t in (MAXF, MAXLOC):
        for root in range(n):
            a = rooted("reduce", "in_order_binary", n, COUNT, op, t, root, True)
            b = rooted("reduce", "in_order_binary", n, COUNT, op, t, root, False)
            if root != n - 1:
                np.testing.assert_array_equal(a, b)
            elif (op, t) == MAXLOC:
                assert _differing(a, b, t) >= FLOOR, (n, root, _differing(a, b, t))
            else:
                assert _differing(a, b, t) > 0


@pytest.mark.parametrize("n", NS)
def test_the_root_shows_in_the_values(n):
    op, t = MAXF
    for kind, alg in ROOT_OBSERVED:
        for root in range(n):
            d = _differing(rooted(kind, alg, n, COUNT, op, t, root, False),
                           rooted(kind, alg, n, COUNT, op, t, (root + 1) % n, False), t)
            assert d >= FLOOR, (kind, alg, n, root, d)
    for alg in ("linear", "in_order_binary"):          # one tree for every root
        for root in range(1, n):
            np.testing.assert_array_equal(rooted("reduce", alg, n, COUNT, op, t, root, False),
                                          rooted("reduce", alg, n, COUNT, op, t, 0, False))


@pytest.mark.parametrize("n", NS)
def test_where_the_variants_coincide(n):
    for op, t in (MAXF, MAXLOC):
        for root in range(n):
            for kind, alg in (("reduce", "linear"), ("ireduce", "binomial")):
                np.testing.assert_array_equal(rooted(kind, alg, n, COUNT, op, t, root, True),
                                              rooted(kind, alg, n, COUNT, op, t, root, False))


ARITH = [p for p in ov.pairs() if ov.is_fp_arith(*p)]
EVERY_ALG = [("reduce", a) for a in REDUCE_ALGS] + [("ireduce", a) for a in IREDUCE_ALGS]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("op,t", ARITH, ids=[f"{o}-{t}" for o, t in ARITH])
def test_sum_and_prod_do_not_see_the_bit(op, t, n):
    # not equal bytes: which NaN survives NaN (op) NaN depends on the operand
    # order, so the comparison is the device test's (golden_io.assert_op_equal)
    for kind, alg in EVERY_ALG:
        for root in range(n):
            golden_io.assert_coll_equal(rooted(kind, alg, n, COUNT, op, t, root, True),
                                        rooted(kind, alg, n, COUNT, op, t, root, False), mxompi.OP[op], mxompi.TYPE[t],
                                        f"{kind} {alg} n {n} root {root}")


@pytest.mark.parametrize("n", NS)
def test_the_bit_shows_in_every_stretch_of_the_chunked_call(n):
    """The device test's chunked call (pipeline, root n // 2, (MAX, FLOAT),
    100003 elements): every chunk's READY word carries the bit anew, and a
    chunk is far longer than 1031 elements, so the floor is asserted for every
    consecutive stretch of 1031 elements."""
    count, (op, t) = 100003, MAXF
    a = rooted("reduce", "pipeline", n, count, op, t, n // 2, True).view(np.uint32)
    b = rooted("reduce", "pipeline", n, count, op, t, n // 2, False).view(np.uint32)
    d = (a != b)[:count // COUNT * COUNT].reshape(-1, COUNT).sum(axis=1)
    assert d.min() >= FLOOR, (n, int(d.min()))
