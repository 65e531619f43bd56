"""The binary16 slots through the MCA components and the mini-host.

The mini-host models a reference configured without a 16-bit float unless
MXH_SHORT_FLOAT=1 is set when mxh_init runs (HAVE_OPAL_SHORT_FLOAT_T +
HAVE_OPAL_SHORT_FLOAT_COMPLEX_T).

CPU: with the opt-in off the op tables are today's (the oracle's pattern,
no MPIX datatypes); with it on the two datatypes exist, the six slots hold
the plain-C base functions in both tables, and MPI_Reduce_local on host
buffers agrees with numpy float16 (tests/short_float.py).
GPU: op/mi355x takes the six slots (2- and 3-buffer) and keeps the base
functions as fallbacks; MPI_Reduce_local through both routes and a
two-process MPI_Allreduce on MPIX_SHORT_FLOAT device buffers are bit-equal to
the helper; calls with one host and one device operand take the fallback
(small, host result) or the device (device result) and agree."""
import ctypes
import os

import numpy as np
import pytest

import minihost
import mxompi
import oracle_lib
import short_float as sf

vp = ctypes.c_void_p
SIX = [("MAX", "SHORT_FLOAT"), ("MIN", "SHORT_FLOAT"), ("SUM", "SHORT_FLOAT"), ("PROD", "SHORT_FLOAT"),
       ("SUM", "C_SHORT_FLOAT_COMPLEX"), ("PROD", "C_SHORT_FLOAT_COMPLEX")]
DT = {"SHORT_FLOAT": "MPIX_SHORT_FLOAT", "C_SHORT_FLOAT_COMPLEX": "MPIX_C_SHORT_FLOAT_COMPLEX"}


def _init(H, with_components, short_float):
    """Re-runs mxh_init (as minihost.host does when the mode changes)."""
    if short_float:
        os.environ["MXH_SHORT_FLOAT"] = "1"
    else:
        os.environ.pop("MXH_SHORT_FLOAT", None)
    O = oracle_lib.oracle()
    comp = os.path.join(mxompi.LIB_DIR, "libmx_ompi.so").encode() if with_components else b""
    rc = H.mxh_init(comp, ctypes.cast(O.mxo_reduce2, vp), ctypes.cast(O.mxo_supported, vp))
    assert rc == 0, rc
    minihost._state["mode"] = with_components
    H.mxh_op_slot_set.argtypes = [vp, ctypes.c_int, ctypes.c_int]


@pytest.fixture
def host_sf():
    """The harness without components, opt-in on; today's tables afterwards."""
    H = minihost.host(with_components=False)
    _init(H, False, True)
    try:
        yield H
    finally:
        _init(H, False, False)


def _mpi_op(H, k):
    name = mxompi.OPS[k]
    return minihost.op(H, "MPI_" + name if name != "NULL" else "MPI_OP_NULL")


def _table(H):
    return {(k, t, three) for k in range(15) for t in range(41) for three in (0, 1)
            if H.mxh_op_slot_set(_mpi_op(H, k), t, three)}


def test_opt_in_off_tables_are_todays():
    H = minihost.host(with_components=False)
    _init(H, False, False)
    O = oracle_lib.oracle()
    want = {(k, t, three) for k in range(15) for t in range(41) for three in (0, 1) if O.mxo_supported(k, t, 1)}
    assert _table(H) == want and len(want) == 2 * 176
    for name in ("MPIX_SHORT_FLOAT", "MPIX_C_FLOAT16", "MPIX_C_SHORT_FLOAT_COMPLEX"):
        assert not minihost.dtype(H, name)


def test_opt_in_adds_six_slots_and_the_datatypes(host_sf):
    H = host_sf
    O = oracle_lib.oracle()
    base = {(k, t, three) for k in range(15) for t in range(41) for three in (0, 1) if O.mxo_supported(k, t, 1)}
    six = {(mxompi.OP[o], mxompi.TYPE[t], three) for o, t in SIX for three in (0, 1)}
    assert _table(H) == base | six
    assert minihost.dtype(H, "MPIX_SHORT_FLOAT") and minihost.dtype(H, "MPIX_C_SHORT_FLOAT_COMPLEX")
    assert minihost.dtype(H, "MPIX_C_FLOAT16")
    # ompi_op_is_valid: an op outside the rows is still rejected
    a = np.zeros(4, np.uint16)
    assert H.mxh_reduce_local(a.ctypes.data, a.ctypes.data, 4, minihost.dtype(H, "MPIX_SHORT_FLOAT"),
                              minihost.op(H, "MPI_BAND")) == -1
    assert H.mxh_reduce_local(a.ctypes.data, a.ctypes.data, 2, minihost.dtype(H, "MPIX_C_SHORT_FLOAT_COMPLEX"),
                              minihost.op(H, "MPI_MAX")) == -1


@pytest.mark.parametrize("op,t", SIX)
def test_reduce_local_host_buffers_run_the_base_functions(host_sf, op, t):
    H = host_sf
    n = 1003
    a, b = sf.gen(op, t, n, 31), sf.gen(op, t, n, 32)
    io = b.copy()
    assert H.mxh_reduce_local(a.ctypes.data, io.ctypes.data, n, minihost.dtype(H, DT[t]),
                              minihost.op(H, "MPI_" + op)) == 0
    sf.assert_equal(op, io, sf.ref(op, t, b, a), f"host MPI_Reduce_local {op} {t}")
    out = np.zeros_like(a)
    assert H.mxh_3buff_op_reduce(minihost.op(H, "MPI_" + op), a.ctypes.data, b.ctypes.data, out.ctypes.data, n,
                                 minihost.dtype(H, DT[t])) == 0
    sf.assert_equal(op, out, sf.ref(op, t, a, b), f"host 3-buffer {op} {t}")


# ---------------------------------------------------------------------------
torch = pytest.importorskip("torch")


@pytest.fixture
def gpu_host_sf():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    mxompi.init(0)
    H = minihost.host(with_components=True)
    _init(H, True, True)
    try:
        yield H
    finally:
        _init(H, True, False)


def _dev(u16):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.uint8).copy()).cuda()


def _u16(tensor):
    return tensor.cpu().numpy().view(np.uint16)


@pytest.mark.gpu
def test_six_slots_taken_by_op_mi355x(gpu_host_sf):
    H = gpu_host_sf
    for op, t in SIX:
        o = minihost.op(H, "MPI_" + op)
        for three in (0, 1):
            assert H.mxh_op_slot_set(o, mxompi.TYPE[t], three)
            assert H.mxh_op_slot_owner(o, mxompi.TYPE[t], three) == 1, (op, t, three)
    # ops outside the rows stay NULL: the NULL pattern is the host's
    assert not H.mxh_op_slot_set(minihost.op(H, "MPI_BAND"), mxompi.TYPE["SHORT_FLOAT"], 0)
    assert not H.mxh_op_slot_set(minihost.op(H, "MPI_MAX"), mxompi.TYPE["C_SHORT_FLOAT_COMPLEX"], 0)
    # every slot of today's tables is still op/mi355x's
    O = oracle_lib.oracle()
    assert sum(H.mxh_op_slot_owner(_mpi_op(H, k), t, 0) == 1 and H.mxh_op_slot_set(_mpi_op(H, k), t, 0)
               for k in range(15) for t in range(41) if O.mxo_supported(k, t, 1)) == 176


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["coll_reduce_local", "op_component", "op_component_3buff"])
@pytest.mark.parametrize("op,t", SIX)
def test_reduce_local_device_buffers(gpu_host_sf, route, op, t):
    H = gpu_host_sf
    n = 5003
    a, b = sf.gen(op, t, n, 51), sf.gen(op, t, n, 52)
    A, B = _dev(a), _dev(b)
    torch.cuda.synchronize()
    o, d = minihost.op(H, "MPI_" + op), minihost.dtype(H, DT[t])
    if route == "coll_reduce_local":
        assert H.mxh_comm_slot_owner(H.mxh_comm_self(), b"reduce_local") == b"mi355x"
        assert H.mxh_reduce_local(A.data_ptr(), B.data_ptr(), n, d, o) == 0
        sf.assert_equal(op, _u16(B), sf.ref(op, t, b, a), f"{route} {op} {t}")
    elif route == "op_component":
        assert H.mxh_op_reduce(o, A.data_ptr(), B.data_ptr(), n, d) == 0
        sf.assert_equal(op, _u16(B), sf.ref(op, t, b, a), f"{route} {op} {t}")
    else:
        OUT = torch.zeros_like(B)
        assert H.mxh_3buff_op_reduce(o, A.data_ptr(), B.data_ptr(), OUT.data_ptr(), n, d) == 0
        sf.assert_equal(op, _u16(OUT), sf.ref(op, t, a, b), f"{route} {op} {t}")


@pytest.mark.gpu
@pytest.mark.parametrize("op,t", [("SUM", "SHORT_FLOAT"), ("MAX", "SHORT_FLOAT"), ("PROD", "C_SHORT_FLOAT_COMPLEX")])
def test_mixed_host_and_device_operands(gpu_host_sf, op, t):
    """ompi_op_reduce with one operand in host and one in device memory
    (op_mi355x.c's operand staging): a small call whose result is in host
    memory brings the device operand over and runs the retained base function;
    a device result is computed by the kernel.  Host buffers alone run the
    fallback too."""
    H = gpu_host_sf
    n = 1003
    a, b = sf.gen(op, t, n, 61), sf.gen(op, t, n, 62)
    o, d = minihost.op(H, "MPI_" + op), minihost.dtype(H, DT[t])
    exp = sf.ref(op, t, b, a)
    A = _dev(a)
    torch.cuda.synchronize()
    io = b.copy()                               # device source, host target: the fallback
    assert H.mxh_op_reduce(o, A.data_ptr(), io.ctypes.data, n, d) == 0
    sf.assert_equal(op, io, exp, f"device in, host inout {op} {t}")
    B = _dev(b)                                 # host source, device target: the kernel
    torch.cuda.synchronize()
    assert H.mxh_op_reduce(o, a.ctypes.data, B.data_ptr(), n, d) == 0
    sf.assert_equal(op, _u16(B), exp, f"host in, device inout {op} {t}")
    io = b.copy()                               # both host: the fallback
    assert H.mxh_op_reduce(o, a.ctypes.data, io.ctypes.data, n, d) == 0
    sf.assert_equal(op, io, exp, f"host buffers {op} {t}")
    out = np.zeros_like(a)                      # 3-buffer: device in1, host in2 and out
    assert H.mxh_3buff_op_reduce(o, A.data_ptr(), b.ctypes.data, out.ctypes.data, n, d) == 0
    sf.assert_equal(op, out, sf.ref(op, t, a, b), f"3-buffer mixed {op} {t}")


# ---- MPI_Allreduce, two processes ------------------------------------------
COUNT = 5003


def _x(rank):
    return sf.gen_spread(COUNT, 800 + rank)


def _allreduce_worker(rank, n, port, q):
    try:
        import torch.distributed as dist
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        os.environ["MXH_SHORT_FLOAT"] = "1"
        os.environ["OMPI_MCA_coll_mi355x_wait_timeout"] = "60"
        os.environ["OMPI_MCA_coll_mi355x_host_max_kb"] = "0"     # device buffers stay on the device path
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n)

        @minihost.AG
        def ag(send, recv, nbytes, ctx):
            out = [None] * n
            dist.all_gather_object(out, ctypes.string_at(send, nbytes))
            blob = b"".join(out)
            ctypes.memmove(recv, blob, len(blob))
            return 0

        torch.cuda.set_device(0)
        mxompi.init(0)
        H = minihost.host(with_components=True)
        comm = H.mxh_comm_create(rank, n, ag, None)
        d, SUM = minihost.dtype(H, "MPIX_SHORT_FLOAT"), minihost.op(H, "MPI_SUM")
        assert d
        X = _dev(_x(rank))
        R = torch.zeros(2 * COUNT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        owner = H.mxh_comm_slot_owner(comm, b"allreduce").decode()
        assert H.mxh_allreduce(X.data_ptr(), R.data_ptr(), COUNT, d, SUM, comm) == 0
        torch.cuda.synchronize()
        res = {"allreduce": R.cpu().numpy().tobytes(), "owner": owner}
        H.mxh_comm_free(comm)
        dist.destroy_process_group()
        q.put((rank, "ok", res))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc()))


@pytest.mark.gpu
def test_allreduce_two_processes_device_buffers():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from test_components_mp import _run_fn
    from test_short_float_coll_gpu import sym
    n = 2
    got = _run_fn(_allreduce_worker, n)
    alg = mxompi.allreduce_decision(n, COUNT, "SHORT_FLOAT")
    assert alg == mxompi.allreduce_decision(n, COUNT, "UINT16_T") == mxompi.ALLREDUCE["ring"]
    exp = sym("allreduce", alg, n, COUNT).evaluate("SUM", "SHORT_FLOAT", [_x(r) for r in range(n)])
    for r in range(n):
        assert got[r]["owner"] == "mi355x"
        sf.assert_equal("SUM", np.frombuffer(got[r]["allreduce"], np.uint16), exp[r][0].ravel(),
                        f"MPI_Allreduce rank {r}")
