"""GPU: the collective folds on the binary16 slots, local communicators of
n in {2, 3, 5, 8} virtual ranks, counts {1, 13, 4099}; SUM and MAX on
SHORT_FLOAT, PROD on C_SHORT_FLOAT_COMPLEX.

The collective oracle (oracle/mx_oracle_coll.c) cannot compute binary16.
Its symbolic mode gives, for the same forced algorithm, n and count on
INT64_T ids, the operation tree of every output element; the trees are
evaluated in numpy float16 (tests/short_float.py).  Only forced algorithms
whose order does not depend on the element size are compared that way; for
AUTO the decision must equal UINT16_T's (same element size), and the AUTO
result the forced one's.  SUM inputs are spread over 12 binades, so a wrong
association changes bits: ring and recursive doubling must give different
expected arrays (asserted on the CPU)."""
import ctypes

import numpy as np
import pytest

import mxompi
import oracle_lib
import short_float as sf

torch = pytest.importorskip("torch")

vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
NS = [2, 3, 5, 8]
COUNTS = [1, 13, 4099]
CASES = [("SUM", "SHORT_FLOAT"), ("MAX", "SHORT_FLOAT"), ("PROD", "C_SHORT_FLOAT_COMPLEX")]
ES = {"SHORT_FLOAT": 2, "C_SHORT_FLOAT_COMPLEX": 4}
I64 = mxompi.TYPE["INT64_T"]


def _oracle():
    L = oracle_lib.oracle()
    L.mxo_allreduce.argtypes = [ci, ci, ci, ci, sz, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.mxo_reduce_scatter.argtypes = [ci, ci, ci, ci, ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.mxo_reduce.argtypes = [ci, ci, ci, ci, sz, ci, ctypes.POINTER(vp), vp]
    L.mxo_scan.argtypes = [ci, ci, ci, ci, sz, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.mxo_exscan.argtypes = [ci, ci, ci, ci, sz, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.mxo_reduce_scatter_block.argtypes = [ci, ci, ci, ci, sz, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    return L


def inputs(op, t, n, count, seed):
    if op == "SUM":
        return [sf.gen_spread(count, seed + r) for r in range(n)]
    if op == "MAX":
        return [sf.gen("MAX", t, count, seed + r) for r in range(n)]
    return [sf.gen_unit(count, seed + r) for r in range(n)]


_SYM = {}


def sym(kind, alg, n, count, root=0):
    """The symbolic result of one oracle collective (cached: every (op, type)
    case evaluates the same trees)."""
    key = (kind, alg, n, count, root)
    if key in _SYM:
        return _SYM[key]
    L = _oracle()
    SUM = mxompi.OP["SUM"]
    if kind == "allreduce":
        r = sf.sym_run(L, lambda sp, rp: L.mxo_allreduce(alg, SUM, I64, n, count, sp, rp), n, count)
    elif kind == "reduce":
        r = sf.sym_run(L, lambda sp, rp: L.mxo_reduce(alg, SUM, I64, n, count, root, sp, rp[0]), n, count, nout=1)
    elif kind in ("scan", "exscan"):
        fn = L.mxo_scan if kind == "scan" else L.mxo_exscan
        r = sf.sym_run(L, lambda sp, rp: fn(alg, SUM, I64, n, count, sp, rp), n, count)
    elif kind == "reduce_scatter":          # `count` per rank
        rc = (sz * n)(*([count] * n))
        r = sf.sym_run(L, lambda sp, rp: L.mxo_reduce_scatter(alg, SUM, I64, n, rc, sp, rp), n, count * n,
                       out_len=count)
    else:                                   # reduce_scatter_block, `count` per rank
        r = sf.sym_run(L, lambda sp, rp: L.mxo_reduce_scatter_block(alg, SUM, I64, n, count, sp, rp), n, count * n,
                       out_len=count)
    if len(_SYM) > 64:
        _SYM.clear()
    _SYM[key] = r
    return r


def test_sum_inputs_tell_ring_from_recursive_doubling():
    """CPU: for the seeds the GPU tests use, ring and recursive doubling give
    different expected arrays at count 4099 for n > 2, so a fold that
    associates wrongly cannot pass."""
    for n in (3, 5, 8):
        xs = inputs("SUM", "SHORT_FLOAT", n, 4099, 100 * n)
        ring = sym("allreduce", mxompi.ALLREDUCE["ring"], n, 4099).evaluate("SUM", "SHORT_FLOAT", xs)
        rd = sym("allreduce", mxompi.ALLREDUCE["recursive_doubling"], n, 4099).evaluate("SUM", "SHORT_FLOAT", xs)
        assert (ring[0][0] != rd[0][0]).sum() > 40, n
        assert sf.nan_fraction(ring[0][0].ravel()) == 0 and sf.nan_fraction(rd[0][0].ravel()) == 0


def test_auto_decides_as_the_two_byte_integer():
    for n in NS:
        for count in COUNTS + [5000, 40003, 300001]:
            assert mxompi.allreduce_decision(n, count, "SHORT_FLOAT") == mxompi.allreduce_decision(n, count, "UINT16_T")
            assert mxompi.reduce_decision(n, count, "SHORT_FLOAT") == mxompi.reduce_decision(n, count, "UINT16_T")
            assert mxompi.reduce_scatter_decision(n, count * n, "SHORT_FLOAT") == \
                mxompi.reduce_scatter_decision(n, count * n, "UINT16_T")


# ---- GPU ------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    mxompi.init(0)
    return torch.cuda.current_stream().cuda_stream


def _dev(u16):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.uint8).copy()).to("cuda")


def _check(op, got, exp_v, written, what):
    """got: device bytes; exp_v [len, w] uint16 with the written mask; bytes
    of unwritten elements must still hold the 0xA5 fill."""
    g = got.cpu().numpy().view(np.uint16).reshape(exp_v.shape)
    sf.assert_equal(op, g[written].ravel(), exp_v[written].ravel(), what)
    assert (g[~written] == 0xA5A5).all(), what + ": wrote where the reference does not"


def _fill(nbytes):
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("alg", ["recursive_doubling", "ring", "rabenseifner", "auto"])
def test_allreduce(gpu, alg, n):
    comm = mxompi.Comm.local(n)
    for count in COUNTS:
        if alg == "auto":       # decided by size as for UINT16_T: below 10000 bytes recursive doubling
            aid = mxompi.allreduce_decision(n, count, "SHORT_FLOAT")
            assert aid == mxompi.allreduce_decision(n, count, "UINT16_T") == mxompi.ALLREDUCE["recursive_doubling"]
        else:
            aid = mxompi.ALLREDUCE[alg]
        for op, t in CASES:
            if alg == "auto" and t != "SHORT_FLOAT":
                continue
            xs = inputs(op, t, n, count, 100 * n)
            exp = sym("allreduce", aid, n, count).evaluate(op, t, xs)
            S = [_dev(x) for x in xs]
            R = [_fill(count * ES[t]) for _ in range(n)]
            comm.allreduce_local([s.data_ptr() for s in S], [r.data_ptr() for r in R], count, t, op, alg, gpu)
            torch.cuda.synchronize()
            for r in range(n):
                _check(op, R[r], exp[r][0], exp[r][1], f"allreduce {alg} n={n} count={count} {op} {t} rank {r}")
    comm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("alg", ["linear", "binomial", "in_order_binary"])
def test_reduce(gpu, alg, n):
    comm = mxompi.Comm.local(n)
    for count in COUNTS:
        for root in sorted({0, n - 1}):
            for op, t in CASES:
                xs = inputs(op, t, n, count, 200 * n + root)
                exp = sym("reduce", mxompi.REDUCE[alg], n, count, root).evaluate(op, t, xs)
                S = [_dev(x) for x in xs]
                R = _fill(count * ES[t])
                rb = [0] * n
                rb[root] = R.data_ptr()
                comm.reduce_local([s.data_ptr() for s in S], rb, count, t, op, root, alg, gpu)
                torch.cuda.synchronize()
                _check(op, R, exp[0][0], exp[0][1], f"reduce {alg} n={n} count={count} root={root} {op} {t}")
    comm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("alg", ["linear", "recursive_doubling"])
@pytest.mark.parametrize("kind", ["scan", "exscan"])
def test_scan_exscan(gpu, kind, alg, n):
    comm = mxompi.Comm.local(n)
    for count in COUNTS:
        for op, t in CASES:
            xs = inputs(op, t, n, count, 300 * n)
            exp = sym(kind, mxompi.SCAN[alg], n, count).evaluate(op, t, xs)
            S = [_dev(x) for x in xs]
            R = [_fill(count * ES[t]) for _ in range(n)]
            getattr(comm, kind + "_local")([s.data_ptr() for s in S], [r.data_ptr() for r in R], count, t, op, alg,
                                           gpu)
            torch.cuda.synchronize()
            for r in range(n):
                if kind == "exscan" and r == 0:
                    assert not exp[0][1].any()          # rank 0's buffer is not written
                _check(op, R[r], exp[r][0], exp[r][1], f"{kind} {alg} n={n} count={count} {op} {t} rank {r}")
    comm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_reduce_scatter_ring(gpu, n):
    comm = mxompi.Comm.local(n)
    for count in COUNTS:                    # per rank
        for op, t in CASES:
            xs = inputs(op, t, n, count * n, 400 * n)
            exp = sym("reduce_scatter", mxompi.REDUCE_SCATTER["ring"], n, count).evaluate(op, t, xs)
            S = [_dev(x) for x in xs]
            R = [_fill(count * ES[t]) for _ in range(n)]
            comm.reduce_scatter_local([s.data_ptr() for s in S], [r.data_ptr() for r in R], [count] * n, t, op,
                                      "ring", gpu)
            torch.cuda.synchronize()
            for r in range(n):
                _check(op, R[r], exp[r][0], exp[r][1], f"reduce_scatter ring n={n} count={count} {op} {t} rank {r}")
    comm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("alg", ["linear", "binomial"])
def test_reduce_scatter_block(gpu, alg, n):
    """basic_linear: a rooted reduce (forced algorithm: its order does not
    depend on the element size) to rank 0, then a scatter."""
    comm = mxompi.Comm.local(n)
    for count in COUNTS:                    # per rank
        for op, t in CASES:
            xs = inputs(op, t, n, count * n, 500 * n)
            exp = sym("reduce_scatter_block", mxompi.REDUCE[alg], n, count).evaluate(op, t, xs)
            S = [_dev(x) for x in xs]
            R = [_fill(count * ES[t]) for _ in range(n)]
            comm.reduce_scatter_block_local([s.data_ptr() for s in S], [r.data_ptr() for r in R], count, t, op, alg,
                                            gpu)
            torch.cuda.synchronize()
            for r in range(n):
                _check(op, R[r], exp[r][0], exp[r][1],
                       f"reduce_scatter_block {alg} n={n} count={count} {op} {t} rank {r}")
    comm.close()
