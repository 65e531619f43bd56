"""MPI_Gather, MPI_Gatherv, MPI_Scatter and MPI_Scatterv on device buffers
through the mini-host and coll/mi355x (n = 2 and 3, MPI_INT): large blocks go
to the library's rooted forms (the rooted call counter rises), small blocks,
vectors the kernels do not take (2-byte words) and calls in which one rank has
a host buffer run on the saved module through host views, with the right bytes
and the counter still; a vector type at the root only -- contiguous elements
elsewhere -- is taken on the device.  Pure data movement: expected values come
from numpy, and every element of every buffer is checked (gaps and the tail
keep the fill)."""
import ctypes
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ci = ctypes.c_int
FILL = -7
VEC = (3, 2, 5)          # MPI_Type_vector(count, blocklength, stride): 6 elements in an extent of 13
LARGE = 24000            # MPI_INT elements: 96 000 bytes a block, above coll_mi355x_host_max_kb
SMALL = 4                # 16 bytes a block
BLOCKING = ("allreduce", "reduce_scatter", "allgather", "bcast", "reduce", "reduce_scatter_block", "scan", "exscan",
            "alltoall", "alltoallv", "allgatherv")
ROOTED = ("gather", "gatherv", "scatter", "scatterv")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _pos(vec, displ, count):
    """element positions of `count` vectors starting `displ` extents in (None: contiguous elements)"""
    if vec is None:
        return displ + np.arange(count, dtype=np.int64)
    c, b, s = vec
    one, ext = np.array([k * s + j for k in range(c) for j in range(b)]), (c - 1) * s + b
    if count == 0:
        return np.zeros(0, dtype=np.int64)
    return (displ * ext + (np.arange(count)[:, None] * ext + one[None, :])).ravel()


def _per(vec):
    """(elements, extent in elements) of one instance"""
    return (1, 1) if vec is None else (vec[0] * vec[1], (vec[0] - 1) * vec[2] + vec[1])


def _data(seed, rank, n_el, npt):
    return np.random.default_rng(seed * 1000 + rank).integers(-30000, 30000, n_el).astype(npt)


def _ints(v):
    return (ci * len(v))(*[int(x) for x in v])


class Ctx:
    def __init__(self, H, comm, rank, n, el_dt, vec_dt, npt):
        self.H, self.comm, self.rank, self.n, self.el_dt, self.vec_dt, self.npt = H, comm, rank, n, el_dt, vec_dt, npt
        self.errs = []

    def buf(self, a, host):
        """a device tensor, or the numpy array itself for a host buffer: (keep-alive, pointer, read-back)"""
        import torch
        if host:
            a = np.ascontiguousarray(a).copy()
            return a, a.ctypes.data, lambda: a
        t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
        return t, t.data_ptr(), lambda: t.cpu().numpy()

    def check(self, name, got, exp):
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            self.errs.append(f"rank {self.rank} {name}: {bad.size} wrong, first at {bad[0]}")


def _rooted(cx, kind, v, count, root, seed, vec=None, inplace=False, host_rank=None):
    """One call.  Every rank's single side is `count` contiguous elements (the
    v-forms: count + rank); the root's side holds one block per rank --
    contiguous, or (vec) as many vectors as hold the block -- with gaps between
    the blocks in the v-forms."""
    H, n, rank, npt = cx.H, cx.n, cx.rank, cx.npt
    per, ext = _per(vec)
    c1 = [count + (p if v else 0) * per for p in range(n)]         # elements of rank p's block
    mc = [c // per for c in c1]                                     # instances of it on the root's side
    md = [sum(mc[:p]) + (3 * p + 2 if v else 0) for p in range(n)]  # in extents
    mlen = (md[-1] + mc[-1]) * ext + 8
    mdt = cx.vec_dt if vec is not None else cx.el_dt
    is_root, gather = rank == root, kind == "gather"
    name = f"{kind}{'v' if v else ''} x{count}" + (" vec" if vec else "") + (" in place" if inplace else "") + \
        (" host" if host_rank is not None else "")
    host_here = host_rank == rank
    if gather:
        src = [_data(seed, p, c1[p], npt) for p in range(n)]
        exp = np.full(mlen, FILL, dtype=npt)
        for p in range(n):
            exp[_pos(vec, md[p], mc[p])] = src[p]
        init = np.full(mlen, FILL, dtype=npt)
        if inplace:
            init[_pos(vec, md[root], mc[root])] = src[root]
        sk, sp, sget = cx.buf(src[rank], host_here)
        mk, mp, mget = cx.buf(init, False) if is_root else (None, None, None)
        if inplace and is_root:
            sp = 1                                                   # MPI_IN_PLACE
        if v:
            rc = H.mxh_gatherv(sp, c1[rank], cx.el_dt, mp, _ints(mc) if is_root else None, _ints(md) if is_root else None,
                               mdt if is_root else None, root, cx.comm)
        else:
            rc = H.mxh_gather(sp, c1[rank], cx.el_dt, mp, mc[0] if is_root else 0, mdt if is_root else None, root, cx.comm)
        if rc:
            cx.errs.append(f"rank {rank} {name}: returned {rc}")
        cx.check(name + " (send buffer)", sget(), src[rank])
        if is_root:
            cx.check(name, mget(), exp)
    else:
        rootdata = _data(seed, root, mlen, npt)
        exp = np.full(c1[rank] + 8, FILL, dtype=npt)
        exp[:c1[rank]] = rootdata[_pos(vec, md[rank], mc[rank])]
        mk, mp, mget = cx.buf(rootdata, False) if is_root else (None, None, None)
        rk, rp, rget = cx.buf(np.full(c1[rank] + 8, FILL, dtype=npt), host_here)
        if inplace and is_root:
            rp, exp = 1, np.full(c1[rank] + 8, FILL, dtype=npt)      # MPI_IN_PLACE: nothing lands in the spare buffer
        if v:
            rc = H.mxh_scatterv(mp, _ints(mc) if is_root else None, _ints(md) if is_root else None,
                                mdt if is_root else None, rp, c1[rank], cx.el_dt, root, cx.comm)
        else:
            rc = H.mxh_scatter(mp, mc[0] if is_root else 0, mdt if is_root else None, rp, c1[rank], cx.el_dt, root, cx.comm)
        if rc:
            cx.errs.append(f"rank {rank} {name}: returned {rc}")
        cx.check(name, rget(), exp)
        if is_root:
            cx.check(name + " (send buffer)", mget(), rootdata)


# (name, element type, numpy type, calls) -- calls: (kind, v-form, count, vector at the root, in place, host rank);
# then the rooted calls the library must count for the case
def _cases(n):
    last = n - 1
    return [
        ("large", "MPI_INT", np.int32, [("gather", False, LARGE, None, False, None), ("gather", True, LARGE, None, False, None),
                                        ("scatter", False, LARGE, None, False, None), ("scatter", True, LARGE, None, False, None)], 4),
        ("small", "MPI_INT", np.int32, [("gather", False, SMALL, None, False, None), ("gather", True, SMALL, None, False, None),
                                        ("scatter", False, SMALL, None, False, None), ("scatter", True, SMALL, None, False, None)], 0),
        ("vector at the root", "MPI_INT", np.int32, [("gather", False, LARGE, VEC, False, None), ("scatter", False, LARGE, VEC, False, None),
                                                     ("gather", True, LARGE, VEC, False, None)], 3),
        ("short vector at the root", "MPI_SHORT", np.int16, [("gather", False, 2 * LARGE, VEC, False, None),
                                                             ("scatter", False, 2 * LARGE, VEC, False, None)], 0),
        ("a host buffer on a rank that is not the root", "MPI_INT", np.int32,
         [("gather", False, LARGE, None, False, last), ("scatter", False, LARGE, None, False, last),
          ("gather", True, LARGE, None, False, last)], 0),
        ("in place at the root", "MPI_INT", np.int32, [("gather", False, LARGE, None, True, None), ("scatter", False, LARGE, None, True, None),
                                                       ("gather", False, LARGE, VEC, True, None)], 3),
    ]


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
        H.mxh_gather.argtypes = [vp, ci, vp, vp, ci, vp, ci, vp]
        H.mxh_scatter.argtypes = [vp, ci, vp, vp, ci, vp, ci, vp]
        H.mxh_gatherv.argtypes = [vp, ci, vp, vp, ip, ip, vp, ci, vp]
        H.mxh_scatterv.argtypes = [vp, ip, ip, vp, vp, ci, vp, ci, vp]
        comm = H.mxh_comm_create(rank, n, ag, None)
        owners = {s: H.mxh_comm_slot_owner(comm, s.encode()).decode() for s in BLOCKING + ROOTED}
        errs, counted = [], []
        for ci_, (name, mpi_t, npt, calls, _) in enumerate(_cases(n)):
            el = minihost.dtype(H, mpi_t)
            cx = Ctx(H, comm, rank, n, el, H.mxh_dtype_vector(VEC[0], VEC[1], VEC[2], el), npt)
            r0, b0, d0 = mxompi.rooted_stats_total()["calls"], mxompi.exchange_stats_total(), mxompi.exchange_ddt_stats_total()
            for k, (kind, v, count, vec, inplace, host_rank) in enumerate(calls):
                _rooted(cx, kind, v, count, root=(ci_ + k) % n if host_rank is None else 0, seed=10 * ci_ + k, vec=vec,
                        inplace=inplace, host_rank=host_rank)
            errs += [f"{name}: {e}" for e in cx.errs]
            counted.append(mxompi.rooted_stats_total()["calls"] - r0)
            if mxompi.exchange_stats_total() != b0 or mxompi.exchange_ddt_stats_total() != d0:
                errs.append(f"{name}: the exchange counters moved")
        torch.cuda.synchronize()
        H.mxh_comm_free(comm)
        # a communicator of one rank: device copies, nothing for the library to count
        me = H.mxh_comm_self()
        self_owners = {s: H.mxh_comm_slot_owner(me, s.encode()).decode() for s in ROOTED}
        el = minihost.dtype(H, "MPI_INT")
        cx = Ctx(H, me, 0, 1, el, H.mxh_dtype_vector(VEC[0], VEC[1], VEC[2], el), np.int32)
        for k, (kind, v, vec, inplace) in enumerate([("gather", False, None, False), ("gather", True, VEC, False),
                                                     ("scatter", False, VEC, False), ("scatter", True, None, False),
                                                     ("gather", False, None, True), ("scatter", True, None, True)]):
            _rooted(cx, kind, v, 600, root=0, seed=90 + k, vec=vec, inplace=inplace)
        errs += [f"size 1: {e}" for e in cx.errs]
        torch.cuda.synchronize()
        dist.destroy_process_group()
        q.put((rank, "ok", {"owners": owners, "self_owners": self_owners, "errs": errs, "counted": counted}))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc()))


@pytest.mark.parametrize("n", [2, 3])
def test_rooted_slots_through_components(n):
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
    want = [c[4] for c in _cases(n)]
    for r in range(n):
        assert out[r]["owners"] == {s: "mi355x" for s in BLOCKING + ROOTED}, out[r]["owners"]
        assert out[r]["self_owners"] == {s: "mi355x" for s in ROOTED}, out[r]["self_owners"]
        assert not out[r]["errs"], "\n".join(out[r]["errs"])
        assert out[r]["counted"] == want, (out[r]["counted"], want)      # the route each case took, on every rank
