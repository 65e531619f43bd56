"""Shared by tests/test_rooted_roots_host.py and tests/test_rooted_roots_mp_gpu.py
(TEST INFRASTRUCTURE): the oracle's result of a rooted reduction over
op_values.inputs(), computed once per case and read-only."""
import ctypes
import functools

import numpy as np

import mxompi
import op_values as ov
import oracle_lib

vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
PREFILL = ov.PREFILL
NS = (3, 5, 8)
COUNT = 1031
REDUCE_ALGS = ("linear", "chain", "pipeline", "binary", "binomial", "in_order_binary")
IREDUCE_ALGS = ("chain", "binomial", "rabenseifner")


@functools.lru_cache(maxsize=None)
def oracle():
    L = oracle_lib.oracle()
    pv = ctypes.POINTER(vp)
    L.mxo_reduce.argtypes = [ci, ci, ci, ci, sz, ci, pv, vp]
    L.mxo_ireduce.argtypes = [ci, ci, ci, ci, sz, ci, pv, vp]
    L.mxo_iallreduce.argtypes = [ci, ci, ci, ci, sz, pv, pv]
    L.mxo_reduce_scatter.argtypes = [ci, ci, ci, ci, ctypes.POINTER(sz), pv, pv]
    L.mxo_ireduce_scatter.argtypes = [ci, ci, ci, ctypes.POINTER(sz), pv, pv]
    L.mxo_scan.argtypes = [ci, ci, ci, ci, sz, pv, pv]
    L.mxo_exscan.argtypes = [ci, ci, ci, ci, sz, pv, pv]
    return L


@functools.lru_cache(maxsize=None)
def rooted(kind, alg, n, count, op, t, root, inplace, base=0):
    """The root's result bytes of kind "reduce" (mxo_reduce, the product's
    algorithm names) or "ireduce" (mxo_ireduce, libnbc's) over
    op_values.inputs(op, t, n, count, base); inplace: MPI_IN_PLACE at the root."""
    xs = ov.inputs(op, t, n, count, base)
    out = xs[root].copy() if inplace else np.full(count * mxompi.type_size(t), PREFILL, np.uint8)
    sp = [x.ctypes.data for x in xs]
    if inplace:
        sp[root] = None
    fn, table = (oracle().mxo_reduce, mxompi.REDUCE) if kind == "reduce" else (oracle().mxo_ireduce, mxompi.IREDUCE)
    assert fn(table[alg], mxompi.OP[op], mxompi.TYPE[t], n, count, root, (vp * n)(*sp), out.ctypes.data) == 0
    out.setflags(write=False)
    return out
