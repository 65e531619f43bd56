"""GPU: mx_reduce2 / mx_reduce3 and their _sync forms on the binary16 slots
(SHORT_FLOAT x {MAX MIN SUM PROD}, C_SHORT_FLOAT_COMPLEX x {SUM PROD}) vs
numpy float16 (tests/short_float.py), bit for bit.

Counts 1, 7, 8, 9 (around one 16-byte vector of 8 halves), 2051 (more than
one workgroup, ragged) and the smallest count whose launch takes the
non-temporal instantiation (mx_reduce.hip: mx_nt_for(2 * n * size) for the
2-buffer form, 3 * n * size for the 3-buffer form, threshold 384 MiB).
Buffer offsets of 0 and 2 bytes on each operand independently for the real
type, 0, 4 and 12 bytes for the complex type: equal misalignment takes the
vector kernel's ragged head, mismatched misalignment the element kernel."""
import itertools

import numpy as np
import pytest

import mxompi
import short_float as sf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAIRS = [("MAX", "SHORT_FLOAT"), ("MIN", "SHORT_FLOAT"), ("SUM", "SHORT_FLOAT"), ("PROD", "SHORT_FLOAT"),
         ("SUM", "C_SHORT_FLOAT_COMPLEX"), ("PROD", "C_SHORT_FLOAT_COMPLEX")]
COUNTS = [1, 7, 8, 9, 2051]
NT_MIN_BYTES = 384 << 20           # mx_runtime.hip nt_min_bytes()
OFFS = {"SHORT_FLOAT": (0, 2), "C_SHORT_FLOAT_COMPLEX": (0, 4, 12)}
ES = {"SHORT_FLOAT": 2, "C_SHORT_FLOAT_COMPLEX": 4}
PAD = 32                           # bytes around every operand


@pytest.fixture(scope="module", autouse=True)
def _init():
    assert torch.cuda.is_available()
    mxompi.init(0)


def _dev(u8):
    return torch.from_numpy(np.ascontiguousarray(u8)).to("cuda")


def _operand(op, t, n, seed, off):
    """(host bytes with `off` bytes in front and padding behind, the uint16 patterns)"""
    v = sf.gen(op, t, n, seed)
    raw = np.random.default_rng(seed + 1).integers(0, 256, off + v.nbytes + PAD, dtype=np.uint8)
    raw[off:off + v.nbytes] = v.view(np.uint8)
    return raw, v


def _run(form, op, t, n, offs, seed, fixed=None):
    es = ES[t]
    nb = n * es
    ra, a = _operand(op, t, n, seed, offs[0])
    rb, b = _operand(op, t, n, seed + 10, offs[1])
    if fixed is not None:                      # a fixed pair in element 0
        k = len(fixed[0])
        a[:k], b[:k] = fixed
        ra[offs[0]:offs[0] + 2 * k] = a[:k].view(np.uint8)
        rb[offs[1]:offs[1] + 2 * k] = b[:k].view(np.uint8)
    A, B = _dev(ra), _dev(rb)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    what = f"{form} {op} {t} n={n} offs={offs}"
    if form.startswith("reduce2"):
        if form == "reduce2":
            mxompi.reduce2(op, t, A.data_ptr() + offs[0], B.data_ptr() + offs[1], n,
                           torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        else:
            mxompi.reduce2_sync(op, t, A.data_ptr() + offs[0], B.data_ptr() + offs[1], n, side.cuda_stream)
        got = B.cpu().numpy()
        sf.assert_equal(op, got[offs[1]:offs[1] + nb], sf.ref(op, t, b, a), what)      # x = inout, y = in
        np.testing.assert_array_equal(got[:offs[1]], rb[:offs[1]], what)
        np.testing.assert_array_equal(got[offs[1] + nb:], rb[offs[1] + nb:], what)
        np.testing.assert_array_equal(A.cpu().numpy(), ra, what)
        return got[offs[1]:offs[1] + nb].view(np.uint16)
    ro = np.random.default_rng(seed + 20).integers(0, 256, offs[2] + nb + PAD, dtype=np.uint8)
    OUT = _dev(ro)
    torch.cuda.synchronize()
    if form == "reduce3":
        mxompi.reduce3(op, t, A.data_ptr() + offs[0], B.data_ptr() + offs[1], OUT.data_ptr() + offs[2], n,
                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    else:
        mxompi.reduce3_sync(op, t, A.data_ptr() + offs[0], B.data_ptr() + offs[1], OUT.data_ptr() + offs[2], n,
                            side.cuda_stream)
    got = OUT.cpu().numpy()
    sf.assert_equal(op, got[offs[2]:offs[2] + nb], sf.ref(op, t, a, b), what)          # x = in1, y = in2
    np.testing.assert_array_equal(got[:offs[2]], ro[:offs[2]], what)
    np.testing.assert_array_equal(got[offs[2] + nb:], ro[offs[2] + nb:], what)
    return got[offs[2]:offs[2] + nb].view(np.uint16)


@pytest.mark.parametrize("form", ["reduce2", "reduce2_sync", "reduce3", "reduce3_sync"])
@pytest.mark.parametrize("op,t", PAIRS)
def test_counts_and_offsets(form, op, t):
    nops = 2 if form.startswith("reduce2") else 3
    seed = 0
    for n in COUNTS:
        for offs in itertools.product(OFFS[t], repeat=nops):
            seed += 1
            _run(form, op, t, n, offs, 1000 * seed)


@pytest.mark.parametrize("form", ["reduce2", "reduce2_sync", "reduce3", "reduce3_sync"])
def test_complex_product_rounds_every_operation(form):
    """a = (0x3c01, 0x4203), b = (0x3bff, 0xc101): six binary16 operations
    give (0x4842, 0x3800); a float expression rounded once gives (0x4843,
    0x3800).  Element 0 of a vector-path and of an element-path launch."""
    a, b, want = sf.DISTINGUISHING
    for n, offs in ((1, (0, 0, 0)), (9, (0, 0, 0)), (9, (4, 0, 12)), (2051, (4, 4, 4))):
        got = _run(form, "PROD", "C_SHORT_FLOAT_COMPLEX", n, offs[:2 if form.startswith("reduce2") else 3], 77,
                   fixed=(a, b))
        np.testing.assert_array_equal(got[:2], want)


# a period of the large operands: prime, so a kernel that mixes up element
# indices pairs operands the period did not pair (as tests/test_reduce_gpu.py)
_PERIOD = 100_003


@pytest.mark.parametrize("form", ["reduce2", "reduce3"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("op,t", PAIRS)
def test_smallest_non_temporal_count(form, op, t, off):
    """The smallest count that selects the non-temporal instantiation, with
    aligned buffers and with one element of equal misalignment (ragged head
    and tail).  The operands repeat a period of random elements; the expected
    result is the period's, tiled the same way on the device."""
    es = ES[t]
    nops = 2 if form == "reduce2" else 3
    n = -(-NT_MIN_BYTES // (nops * es))
    assert nops * n * es >= NT_MIN_BYTES > nops * (n - 1) * es
    a, b = sf.gen(op, t, _PERIOD, 5), sf.gen(op, t, _PERIOD, 6)
    exp = sf.ref(op, t, b, a) if form == "reduce2" else sf.ref(op, t, a, b)
    if op in ("SUM", "PROD"):
        assert sf.nan_fraction(exp) <= sf.NAN_CAP
    reps = -(-(n + off) // _PERIOD)
    ob = off * es

    def tile(v):
        return _dev(v.view(np.uint8)).repeat(reps)[: (n + off) * es].contiguous()
    A, B, E = tile(a), tile(b), tile(exp)
    s = torch.cuda.current_stream().cuda_stream
    if form == "reduce2":
        head = B[:ob].clone()
        mxompi.reduce2(op, t, A.data_ptr() + ob, B.data_ptr() + ob, n, s)
        out = B
    else:
        out = torch.zeros_like(B)
        head = out[:ob].clone()
        mxompi.reduce3(op, t, A.data_ptr() + ob, B.data_ptr() + ob, out.data_ptr() + ob, n, s)
    torch.cuda.synchronize()
    assert torch.equal(out[:ob], head)
    g16, e16 = out[ob:].view(torch.int16), E[ob:].view(torch.int16)
    if op in ("SUM", "PROD"):      # a NaN where one is expected, the bits elsewhere
        enan = torch.isnan(E[ob:].view(torch.float16))
        assert bool(torch.isnan(out[ob:].view(torch.float16))[enan].all())
        g16, e16 = g16[~enan], e16[~enan]
    bad = torch.nonzero(g16 != e16)
    assert bad.numel() == 0, f"{form} {op} {t}: {bad.shape[0]} elements differ, first {int(bad[0, 0])}"
    del A, B, E, out
    torch.cuda.empty_cache()


def test_sync_call_routes_service_and_launch():
    """mx_reduce2_sync on an idle non-default stream: 16-byte aligned buffers
    of at most 2 MiB go to the resident reduce service, a buffer 2 bytes off
    the alignment is declined to the launch path; mx_op_service_stats tells
    which route ran.  Both bit-equal to the oracle."""
    op, t, n = "SUM", "SHORT_FLOAT", 4099
    s = torch.cuda.Stream()
    ra, a = _operand(op, t, n, 41, 0)
    rb, b = _operand(op, t, n, 42, 16)
    A, B = _dev(ra), _dev(rb)
    torch.cuda.synchronize()
    st, served0, _ = mxompi.op_service_stats()
    mxompi.reduce2_sync(op, t, A.data_ptr(), B.data_ptr() + 16, n, s.cuda_stream)
    got = B.cpu().numpy()
    st, served1, _ = mxompi.op_service_stats()
    assert st == 1, "service unusable on this box"
    assert served1 == served0 + 1
    sf.assert_equal(op, got[16:16 + 2 * n], sf.ref(op, t, b, a), "served")
    # declined: inout 2 bytes off a 16-byte boundary
    rb2, b2 = _operand(op, t, n, 45, 2)
    B2 = _dev(rb2)
    torch.cuda.synchronize()
    mxompi.reduce2_sync(op, t, A.data_ptr(), B2.data_ptr() + 2, n, s.cuda_stream)
    got = B2.cpu().numpy()
    assert mxompi.op_service_stats()[1] == served1
    sf.assert_equal(op, got[2:2 + 2 * n], sf.ref(op, t, b2, a), "declined")
    # the 3-buffer form through the service, complex PROD
    op, t, n = "PROD", "C_SHORT_FLOAT_COMPLEX", 2051
    ra, a = _operand(op, t, n, 43, 0)
    rb, b = _operand(op, t, n, 44, 0)
    A, B = _dev(ra), _dev(rb)
    OUT = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    served1 = mxompi.op_service_stats()[1]
    mxompi.reduce3_sync(op, t, A.data_ptr(), B.data_ptr(), OUT.data_ptr(), n, s.cuda_stream)
    got = OUT.cpu().numpy()
    assert mxompi.op_service_stats()[1] == served1 + 1
    sf.assert_equal(op, got, sf.ref(op, t, a, b), "served 3-buffer")
