"""MPI_Alltoall, MPI_Alltoallv and MPI_Allgatherv through the mini-host
(mxh_alltoall / mxh_alltoallv / mxh_allgatherv): the host stand-ins of the base
modules on host buffers (CPU, gloo), and coll/mi355x's three slots on device
buffers (GPU) -- the device path above coll_mi355x_host_max_kb, the saved
module for small calls and derived datatypes, device copies on a size-1
communicator.  Pure data movement: expected values come from numpy."""
import ctypes
import os
import socket

import numpy as np
import pytest

ci = ctypes.c_int
FILL = -7
VEC = (3, 2, 5)      # MPI_Type_vector(count 3, blocklength 2, stride 5) of MPI_INT


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _declare(H):
    """The three entry points on the handle tests/minihost.py returns."""
    vp = ctypes.c_void_p
    ip = ctypes.POINTER(ci)
    H.mxh_alltoall.argtypes = [vp, ci, vp, vp, ci, vp, vp]
    H.mxh_alltoallv.argtypes = [vp, ip, ip, vp, vp, ip, ip, vp, vp]
    H.mxh_allgatherv.argtypes = [vp, ci, vp, vp, ip, ip, vp, vp]


def _ints(v):
    return (ci * len(v))(*[int(x) for x in v])


def _layout(kind):
    """(int32 positions of one element, extent in int32s)."""
    if kind == "int":
        return np.array([0]), 1
    c, b, s = VEC
    return np.array([k * s + j for k in range(c) for j in range(b)]), (c - 1) * s + b


def _pos(kind, displ, count):
    """int32 positions of `count` elements starting `displ` extents in."""
    one, ext = _layout(kind)
    if count == 0:
        return np.zeros(0, dtype=np.int64)
    return (displ * ext + (np.arange(count)[:, None] * ext + one[None, :])).ravel()


def _data(seed, rank, n_int):
    return np.random.default_rng(seed * 1000 + rank).integers(-10**6, 10**6, n_int).astype(np.int32)


def _tables(n, count):
    """Ragged counts [sender][receiver] (one pair empty) and displacements
    with gaps, in elements; the same in every process."""
    rng = np.random.default_rng(5 + n + count)
    C = (count + rng.integers(0, 5, (n, n))).tolist()
    if n > 1:
        C[0][n - 1] = 0
    sd = [[sum(C[i][:j]) + 2 * j + 1 for j in range(n)] for i in range(n)]
    rd = [[sum(C[k][j] for k in range(i)) + 3 * i + 2 for i in range(n)] for j in range(n)]
    return C, sd, rd


def _run_case(H, comm, rank, n, to_dev, kind, count, dts):
    """alltoall (+ in place), alltoallv, allgatherv of `count`-element blocks
    of datatype `kind`; returns error strings."""
    dt = dts[kind]
    _, ext = _layout(kind)
    errs = []

    def check(name, R, exp):
        got = R.cpu().numpy()
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            errs.append(f"rank {rank} {name} {kind} x{count}: {bad.size} wrong, first at {bad[0]}")

    # -- alltoall
    blk = count * ext
    src = [_data(1, r, n * blk) for r in range(n)]
    exp = np.full(n * blk + 4, FILL, dtype=np.int32)
    for p in range(n):
        exp[_pos(kind, p * count, count)] = src[p][_pos(kind, rank * count, count)]
    S, R = to_dev(src[rank]), to_dev(np.full(n * blk + 4, FILL, dtype=np.int32))
    assert H.mxh_alltoall(S.data_ptr(), count, dt, R.data_ptr(), count, dt, comm) == 0
    check("alltoall", R, exp)
    # -- alltoall, MPI_IN_PLACE
    exp = src[rank].copy()
    for p in range(n):
        exp[_pos(kind, p * count, count)] = src[p][_pos(kind, rank * count, count)]
    R = to_dev(src[rank])
    assert H.mxh_alltoall(1, count, dt, R.data_ptr(), count, dt, comm) == 0   # MPI_IN_PLACE
    check("alltoall in place", R, exp)
    # -- alltoallv
    C, sd, rd = _tables(n, count)
    slen = max(sd[i][n - 1] + C[i][n - 1] for i in range(n)) * ext + 4
    rlen = max(rd[j][n - 1] + C[n - 1][j] for j in range(n)) * ext + 4
    src = [_data(2, r, slen) for r in range(n)]
    exp = np.full(rlen, FILL, dtype=np.int32)
    for p in range(n):
        exp[_pos(kind, rd[rank][p], C[p][rank])] = src[p][_pos(kind, sd[p][rank], C[p][rank])]
    S, R = to_dev(src[rank]), to_dev(np.full(rlen, FILL, dtype=np.int32))
    assert H.mxh_alltoallv(S.data_ptr(), _ints(C[rank]), _ints(sd[rank]), dt, R.data_ptr(),
                           _ints([C[p][rank] for p in range(n)]), _ints(rd[rank]), dt, comm) == 0
    check("alltoallv", R, exp)
    # -- allgatherv
    rc = [count + 2 * p for p in range(n)]
    rc[n - 1] = 0 if n > 2 else rc[n - 1]
    dp = [sum(rc[:p]) + 2 * p + 1 for p in range(n)]
    src = [_data(3, r, rc[r] * ext + 1) for r in range(n)]
    glen = (dp[n - 1] + rc[n - 1]) * ext + 4
    exp = np.full(glen, FILL, dtype=np.int32)
    for p in range(n):
        exp[_pos(kind, dp[p], rc[p])] = src[p][_pos(kind, 0, rc[p])]
    S, R = to_dev(src[rank]), to_dev(np.full(glen, FILL, dtype=np.int32))
    assert H.mxh_allgatherv(S.data_ptr(), rc[rank], dt, R.data_ptr(), _ints(rc), _ints(dp), dt, comm) == 0
    check("allgatherv", R, exp)
    return errs


_SLOTS = ("alltoall", "alltoallv", "allgatherv")


def _worker(rank, n, port, use_gpu, cases, q):
    try:
        import torch
        import torch.distributed as dist
        import minihost
        import mxompi
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        # the component's device communicator bounds its peer waits, so a stuck
        # rank ends the test instead of holding the GPU
        os.environ["OMPI_MCA_coll_mi355x_wait_timeout"] = "30"
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n)

        @minihost.AG
        def ag(send, recv, nbytes, ctx):
            out = [None] * n
            dist.all_gather_object(out, ctypes.string_at(send, nbytes))
            blob = b"".join(out)
            ctypes.memmove(recv, blob, len(blob))
            return 0

        if use_gpu:
            torch.cuda.set_device(0)
            mxompi.init(0)
        H = minihost.host(with_components=True)
        _declare(H)
        comm = H.mxh_comm_create(rank, n, ag, None)
        owners = {s: H.mxh_comm_slot_owner(comm, s.encode()).decode() for s in _SLOTS}
        i32 = minihost.dtype(H, "MPI_INT")
        dts = {"int": i32, "vec": H.mxh_dtype_vector(VEC[0], VEC[1], VEC[2], i32)}

        def to_dev(a):
            t = torch.from_numpy(np.ascontiguousarray(a).copy())
            return t.cuda() if use_gpu else t

        errs, calls = [], []
        for kind, count in cases:
            before = mxompi.exchange_stats_total()["calls"] if use_gpu else 0
            errs += _run_case(H, comm, rank, n, to_dev, kind, count, dts)
            calls.append((mxompi.exchange_stats_total()["calls"] if use_gpu else 0) - before)
        if use_gpu:
            torch.cuda.synchronize()
        H.mxh_comm_free(comm)
        dist.destroy_process_group()
        q.put((rank, "ok", {"owners": owners, "errs": errs, "calls": calls}))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc()))


def _run(n, use_gpu, cases):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, n, port, use_gpu, cases, q)) for r in range(n)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(n):
            rank, status, payload = q.get(timeout=300)
            assert status == "ok", payload
            out[rank] = payload
    finally:
        for p in procs:
            p.join(timeout=60 if len(out) == n else 5)
            if p.is_alive():      # a failed rank leaves its peers waiting: end them
                p.terminate()
                p.join(timeout=10)
    return out


@pytest.mark.parametrize("n", [2, 3])
def test_host_buffers_gloo_cpu(n):
    """Host buffers, MPI_INT and a vector datatype, MPI_IN_PLACE alltoall: the
    base modules' stand-ins give numpy's bytes."""
    got = _run(n, use_gpu=False, cases=[("int", 37), ("vec", 5)])
    import torch
    for r in range(n):
        assert not got[r]["errs"], "\n".join(got[r]["errs"])
        if not torch.cuda.is_available():     # no component without a device: the base module owns the slots
            assert got[r]["owners"] == {s: "tuned" for s in _SLOTS}, got[r]["owners"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_device_buffers_through_components(n):
    """Device buffers.  30000-int blocks are above coll_mi355x_host_max_kb (64):
    the device path runs (the process's exchange calls rise by the four calls
    of a case).  16-int blocks (64 B) run on the saved module through host
    views, a vector datatype falls through whatever its size: no exchange call,
    the same bytes."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    got = _run(n, use_gpu=True, cases=[("int", 30000), ("int", 16), ("vec", 4000)])
    for r in range(n):
        assert got[r]["owners"] == {s: "mi355x" for s in _SLOTS}, got[r]["owners"]
        assert not got[r]["errs"], "\n".join(got[r]["errs"])
        assert got[r]["calls"] == [4, 0, 0], got[r]["calls"]


@pytest.mark.gpu
def test_size_one_communicator_device_copies():
    """MPI_COMM_SELF: the three slots are coll/mi355x's and copy device
    buffers on the device (no call reaches coll/self's host copies)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import minihost
    import mxompi
    mxompi.init(0)
    H = minihost.host(with_components=True)
    _declare(H)
    comm = H.mxh_comm_self()
    for s in _SLOTS:
        assert H.mxh_comm_slot_owner(comm, s.encode()).decode() == "mi355x", s
    i32 = minihost.dtype(H, "MPI_INT")
    dts = {"int": i32, "vec": H.mxh_dtype_vector(VEC[0], VEC[1], VEC[2], i32)}
    before = H.mxh_self_calls()
    errs = []
    for kind, count in (("int", 1000), ("vec", 50)):
        errs += _run_case(H, comm, 0, 1, lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda(),
                          kind, count, dts)
    torch.cuda.synchronize()
    assert not errs, "\n".join(errs)
    assert H.mxh_self_calls() == before
