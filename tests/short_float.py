"""CPU oracle for the binary16 slots (MX_TYPE_SHORT_FLOAT and its complex
type): numpy float16, whose + - * are single correctly rounded binary16
operations (computed in float and rounded once more, which is innocuous:
24 >= 2 * 11 + 2 significand bits).  Semantics: DESIGN.md section 5.

Arrays are uint16 bit patterns throughout; complex values are interleaved
(re, im).  x is the reference's first operand (2-buffer: the target `out`;
3-buffer: in1), y the second (the source `in`; in2)."""
import numpy as np

F16 = np.float16
NAN_CAP = 0.01          # at most 1 % of the expected SUM / PROD elements may be NaN

# COMPLEX_PROD_FUNC with every operation rounded to binary16 gives
# (0x4842, 0x3800) for a = (0x3c01, 0x4203), b = (0x3bff, 0xc101); evaluating
# the expression in float and rounding once gives (0x4843, 0x3800)
DISTINGUISHING = (np.array([0x3C01, 0x4203], np.uint16), np.array([0x3BFF, 0xC101], np.uint16),
                  np.array([0x4842, 0x3800], np.uint16))


def _f(u):
    return np.ascontiguousarray(u, dtype=np.uint16).view(F16)


def ref(op, t, x, y):
    """x OP y element-wise on uint16 patterns; t: "SHORT_FLOAT" or "C_SHORT_FLOAT_COMPLEX"."""
    x = np.ascontiguousarray(x, dtype=np.uint16)
    y = np.ascontiguousarray(y, dtype=np.uint16)
    with np.errstate(all="ignore"):
        if t == "SHORT_FLOAT":
            if op == "MAX":
                return np.where(_f(x) > _f(y), x, y)
            if op == "MIN":
                return np.where(_f(x) < _f(y), x, y)
            if op == "SUM":
                return (_f(x) + _f(y)).view(np.uint16)
            if op == "PROD":
                return (_f(x) * _f(y)).view(np.uint16)
        else:
            if op == "SUM":
                return (_f(x) + _f(y)).view(np.uint16)
            if op == "PROD":            # COMPLEX_PROD_FUNC, a = y (in), b = x (out): six rounded operations
                b0, b1 = _f(x[0::2]), _f(x[1::2])
                a0, a1 = _f(y[0::2]), _f(y[1::2])
                r = np.empty(len(x), np.uint16)
                r[0::2] = ((a0 * b0).astype(F16) - (a1 * b1).astype(F16)).astype(F16).view(np.uint16)
                r[1::2] = ((a0 * b1).astype(F16) + (a1 * b0).astype(F16)).astype(F16).view(np.uint16)
                return r
    raise ValueError((op, t))


def nan_fraction(exp):
    return float(np.isnan(_f(exp)).mean()) if len(exp) else 0.0


def assert_equal(op, got, exp, what=""):
    """MAX / MIN: every bit of every element (NaN payloads, zero signs).
    SUM / PROD: bits where the expected value is not NaN, a NaN where it is;
    the share of NaNs among the expected elements is capped (on the CPU side,
    so that a generator change cannot hide the comparison)."""
    got = np.ascontiguousarray(got).view(np.uint16).ravel()
    exp = np.ascontiguousarray(exp).view(np.uint16).ravel()
    assert got.shape == exp.shape, what
    if op in ("MAX", "MIN"):
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:1]}: {got[bad[:1]]} != {exp[bad[:1]]}"
        return
    nan = np.isnan(_f(exp))
    assert nan.sum() <= NAN_CAP * len(exp), f"{what}: {nan.sum()} of {len(exp)} expected elements are NaN"
    bad = np.nonzero((got != exp) & ~nan)[0]
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:1]}: {got[bad[:1]]} != {exp[bad[:1]]}"
    assert np.isnan(_f(got)[nan]).all(), f"{what}: a NaN expected"


def _finite(rng, n, emin=0, emax=30):
    """Random finite patterns, exponent field uniform in [emin, emax] (0 =
    subnormals), random sign and significand."""
    e = rng.integers(emin, emax + 1, n).astype(np.uint16)
    m = rng.integers(0, 1024, n).astype(np.uint16)
    s = rng.integers(0, 2, n).astype(np.uint16)
    return (s << 15) | (e << 10) | m


def gen(op, t, n, seed):
    """Operand of n elements (uint16 patterns, 2n for the complex type).
    SUM / PROD: normal values over the whole exponent range, subnormals, both
    zeros, a few infinities; sums and products overflow to infinity.
    MAX / MIN: few distinct values (ties), both zeros, infinities, NaNs of
    both signs with payloads.  Complex PROD: moderate magnitudes with a few
    full-range values (inf - inf in a component would be a NaN)."""
    rng = np.random.default_rng(seed)
    if t == "C_SHORT_FLOAT_COMPLEX":
        m = 2 * n
        if op == "PROD":
            v = _finite(rng, m, 10, 20)
            k = rng.random(m) < 0.04
            v[k] = _finite(rng, int(k.sum()))
            return v
        return _mixed(rng, m)
    if op in ("MAX", "MIN"):
        pool = np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFDFF, 0x7FFF, 0x0001, 0x8001,
                         0x3C00, 0xBC00, 0x3C01, 0x7BFF, 0xFBFF, 0x03FF, 0x0400], np.uint16)
        v = pool[rng.integers(0, len(pool), n)]
        k = rng.random(n) < 0.5
        v[k] = _finite(rng, int(k.sum()))
        return v
    return _mixed(rng, n)


def _mixed(rng, n):
    v = _finite(rng, n)
    u = rng.random(n)
    v[u < 0.01] = 0x0000
    v[(u >= 0.01) & (u < 0.02)] = 0x8000
    v[(u >= 0.02) & (u < 0.023)] = 0x7C00
    v[(u >= 0.023) & (u < 0.026)] = 0xFC00
    v[(u >= 0.026) & (u < 0.05)] = _finite(rng, int(((u >= 0.026) & (u < 0.05)).sum()), 30, 30)   # near the top
    return v


def gen_spread(n, seed):
    """SUM operands for the collectives: magnitudes spread over ~12 binades
    around 1 so that the association order changes bits and nothing
    overflows (no NaN from inf - inf)."""
    rng = np.random.default_rng(seed)
    return _finite(rng, n, 9, 21)


def gen_unit(n, seed, width=2):
    """Complex PROD operands for the collectives: components in +-[0.5, 2),
    so a product of 16 of them neither overflows nor underflows."""
    rng = np.random.default_rng(seed)
    return _finite(rng, width * n, 14, 15)


# ---------------------------------------------------------------------------
# Collectives: the collective oracle (oracle/mx_oracle_coll.c) cannot compute
# binary16, but its symbolic mode records, for INT64_T "expression ids", the
# exact operation tree of every output element.  sym_run() runs one oracle
# call that way; SymResult.evaluate() then evaluates the trees with ref()
# above, all nodes of one depth at a time.
# ---------------------------------------------------------------------------
LEAF_STRIDE = 1 << 24
UNTOUCHED = np.iinfo(np.int64).min


def sym_inputs(n, count):
    """Per rank, the leaf ids of its `count` elements."""
    return [-(r * LEAF_STRIDE + np.arange(count, dtype=np.int64) + 1) for r in range(n)]


class SymResult:
    def __init__(self, L, outs):
        import ctypes
        self.outs = outs                      # per output buffer: int64 ids (UNTOUCHED: never written)
        top = max([int(o[o != UNTOUCHED].max()) for o in outs if (o != UNTOUCHED).any()] + [-1])
        nn = top + 1
        self.T = np.empty(nn, np.int64)
        self.S = np.empty(nn, np.int64)
        t, s = ctypes.c_int64(), ctypes.c_int64()
        pt, ps = ctypes.byref(t), ctypes.byref(s)
        for i in range(nn):
            assert L.mxo_sym_node(i, pt, ps) == 0
            self.T[i], self.S[i] = t.value, s.value
        # nodes are numbered in creation order: operands precede their node
        assert nn == 0 or ((self.T < np.arange(nn)) & (self.S < np.arange(nn))).all()
        lvl = np.zeros(nn, np.int32)
        T, S = self.T.tolist(), self.S.tolist()
        lv = [0] * nn
        for i in range(nn):
            a = lv[T[i]] if T[i] >= 0 else 0
            b = lv[S[i]] if S[i] >= 0 else 0
            lv[i] = (a if a > b else b) + 1
        lvl[:] = lv
        self.order = [np.nonzero(lvl == d)[0] for d in range(1, int(lvl.max()) + 1)] if nn else []

    def evaluate(self, op, t, inputs):
        """inputs: per rank uint16 patterns (width w per element).  Returns
        per output buffer (values [len, w] uint16, written mask)."""
        w = 2 if t == "C_SHORT_FLOAT_COMPLEX" else 1
        leaves = np.stack([np.ascontiguousarray(x, dtype=np.uint16).reshape(-1, w) for x in inputs])
        vals = np.zeros((len(self.T), w), np.uint16)

        def look(ids):
            out = np.empty((len(ids), w), np.uint16)
            neg = ids < 0
            k = -ids[neg] - 1
            out[neg] = leaves[k // LEAF_STRIDE, k % LEAF_STRIDE]
            out[~neg] = vals[ids[~neg]]
            return out
        for ids in self.order:      # node = target OP source: x = target, y = source
            vals[ids] = ref(op, t, look(self.T[ids]).ravel(), look(self.S[ids]).ravel()).reshape(-1, w)
        res = []
        for o in self.outs:
            wr = o != UNTOUCHED
            v = np.zeros((len(o), w), np.uint16)
            v[wr] = look(o[wr])
            res.append((v, wr))
        return res


def sym_run(L, call, n, count, nout=None, out_len=None):
    """call(sbuf pointers, rbuf pointers) runs one oracle collective on
    INT64_T in symbolic mode; returns the SymResult of its output buffers."""
    import ctypes
    vp = ctypes.c_void_p
    L.mxo_sym_node.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    nout = n if nout is None else nout
    xs = sym_inputs(n, count)
    outs = [np.full(count if out_len is None else out_len, UNTOUCHED, np.int64) for _ in range(nout)]
    L.mxo_sym_reset(1)
    try:
        rc = call((vp * n)(*[x.ctypes.data for x in xs]), (vp * nout)(*[o.ctypes.data for o in outs]))
        assert rc == 0, rc
        return SymResult(L, outs)
    finally:
        L.mxo_sym_reset(0)
