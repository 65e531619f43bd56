"""MPI_Alltoall and MPI_Alltoallv of vector datatypes on device buffers through
the mini-host and coll/mi355x: above coll_mi355x_host_max_kb the component
hands them to the library's strided forms (the strided call counter rises, the
byte forms' counters stay), small calls and vectors the kernel does not take
(2-byte blocks) run on the saved module through host views.  Pure data
movement: expected values come from numpy."""
import ctypes
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ci = ctypes.c_int
FILL = -7
# (name, MPI element type, numpy type, (count, blocklength, stride) of MPI_Type_vector, elements per block)
CASES = [
    ("int vector, large", "MPI_INT", np.int32, (3, 2, 5), 4000),      # 96 000 bytes a pair: the device
    ("int vector, small", "MPI_INT", np.int32, (3, 2, 5), 4),         # under host_max_kb: the saved module
    ("short vector, large", "MPI_SHORT", np.int16, (3, 1, 5), 8000),  # 2-byte blocks: refused, the saved module
]
EXPECT_DDT_CALLS = [3, 0, 0]      # alltoall, alltoall in place and alltoallv of the first case only


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _pos(vec, displ, count):
    """element positions of `count` vectors starting `displ` extents in"""
    c, b, s = vec
    one, ext = np.array([k * s + j for k in range(c) for j in range(b)]), (c - 1) * s + b
    if count == 0:
        return np.zeros(0, dtype=np.int64)
    return (displ * ext + (np.arange(count)[:, None] * ext + one[None, :])).ravel()


def _data(seed, rank, n_el, npt):
    return np.random.default_rng(seed * 1000 + rank).integers(-30000, 30000, n_el).astype(npt)


def _tables(n, count):
    """Ragged counts [sender][receiver] (one pair empty) and displacements with gaps."""
    rng = np.random.default_rng(9 + n + count)
    C = (count + rng.integers(0, 5, (n, n))).tolist()
    C[0][n - 1] = 0
    sd = [[sum(C[i][:j]) + 2 * j + 1 for j in range(n)] for i in range(n)]
    rd = [[sum(C[k][j] for k in range(i)) + 3 * i + 2 for i in range(n)] for j in range(n)]
    return C, sd, rd


def _ints(v):
    return (ci * len(v))(*[int(x) for x in v])


def _run_case(H, comm, rank, n, to_dev, dt, npt, vec, count):
    ext = (vec[0] - 1) * vec[2] + vec[1]
    errs = []

    def check(name, R, exp):
        got = R.cpu().numpy()
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            errs.append(f"rank {rank} {name} x{count}: {bad.size} wrong, first at {bad[0]}")

    blk = count * ext
    src = [_data(1, r, n * blk, npt) for r in range(n)]
    exp = np.full(n * blk + 8, FILL, dtype=npt)       # gaps and the tail keep the fill
    for p in range(n):
        exp[_pos(vec, p * count, count)] = src[p][_pos(vec, rank * count, count)]
    S, R = to_dev(src[rank]), to_dev(np.full(n * blk + 8, FILL, dtype=npt))
    assert H.mxh_alltoall(S.data_ptr(), count, dt, R.data_ptr(), count, dt, comm) == 0
    check("alltoall", R, exp)
    exp = src[rank].copy()
    for p in range(n):
        exp[_pos(vec, p * count, count)] = src[p][_pos(vec, rank * count, count)]
    R = to_dev(src[rank])
    assert H.mxh_alltoall(1, count, dt, R.data_ptr(), count, dt, comm) == 0   # MPI_IN_PLACE
    check("alltoall in place", R, exp)
    C, sd, rd = _tables(n, count)
    slen = max(sd[i][n - 1] + C[i][n - 1] for i in range(n)) * ext + 8
    rlen = max(rd[j][n - 1] + C[n - 1][j] for j in range(n)) * ext + 8
    src = [_data(2, r, slen, npt) for r in range(n)]
    exp = np.full(rlen, FILL, dtype=npt)
    for p in range(n):
        exp[_pos(vec, rd[rank][p], C[p][rank])] = src[p][_pos(vec, sd[p][rank], C[p][rank])]
    S, R = to_dev(src[rank]), to_dev(np.full(rlen, FILL, dtype=npt))
    assert H.mxh_alltoallv(S.data_ptr(), _ints(C[rank]), _ints(sd[rank]), dt, R.data_ptr(),
                           _ints([C[p][rank] for p in range(n)]), _ints(rd[rank]), dt, comm) == 0
    check("alltoallv", R, exp)
    return errs


def _worker(rank, n, port, q):
    try:
        import torch
        import torch.distributed as dist
        import minihost
        import mxompi
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        os.environ["OMPI_MCA_coll_mi355x_wait_timeout"] = "30"
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
        vp, ip = ctypes.c_void_p, ctypes.POINTER(ci)
        H.mxh_alltoall.argtypes = [vp, ci, vp, vp, ci, vp, vp]
        H.mxh_alltoallv.argtypes = [vp, ip, ip, vp, vp, ip, ip, vp, vp]
        comm = H.mxh_comm_create(rank, n, ag, None)
        owners = {s: H.mxh_comm_slot_owner(comm, s.encode()).decode() for s in ("alltoall", "alltoallv")}

        def to_dev(a):
            return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()

        errs, ddt_calls, byte_calls = [], [], []
        for name, mpi_t, npt, vec, count in CASES:
            dt = H.mxh_dtype_vector(vec[0], vec[1], vec[2], minihost.dtype(H, mpi_t))
            d0, b0 = mxompi.exchange_ddt_stats_total()["calls"], mxompi.exchange_stats_total()
            errs += [f"{name}: {e}" for e in _run_case(H, comm, rank, n, to_dev, dt, npt, vec, count)]
            ddt_calls.append(mxompi.exchange_ddt_stats_total()["calls"] - d0)
            byte_calls.append(mxompi.exchange_stats_total() == b0)
        torch.cuda.synchronize()
        H.mxh_comm_free(comm)
        dist.destroy_process_group()
        q.put((rank, "ok", {"owners": owners, "errs": errs, "ddt": ddt_calls, "bytes_still": byte_calls}))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 3])
def test_vector_datatypes_through_components(n):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, n, port, q)) for r in range(n)]
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
    for r in range(n):
        assert out[r]["owners"] == {"alltoall": "mi355x", "alltoallv": "mi355x"}, out[r]["owners"]
        assert not out[r]["errs"], "\n".join(out[r]["errs"])
        assert out[r]["ddt"] == EXPECT_DDT_CALLS, out[r]["ddt"]      # the route each case took
        assert out[r]["bytes_still"] == [True] * len(CASES)          # the byte forms' counters never move
