"""GPU parity of the collective data path vs the reference's algorithms.

The all-peer kernels evaluate, per element, the reduction tree of the
selected coll/base algorithm; the oracle (oracle/mx_oracle_coll.c) runs the
reference's algorithms step by step with the op oracle.  Results must be
bit-identical -- including floating-point SUM/PROD, whose value depends on
the order -- for every algorithm, rank count and ragged size.

* local communicators (n virtual ranks, one process, one GPU);
* multi-process communicators (n processes sharing the one GPU, IPC-mapped
  staging, cross-process flags) through torch.distributed(gloo) bootstrap.
"""
import ctypes
import os
import socket

import numpy as np
import pytest

import golden_io
import mxompi
import oracle_lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def _oracle():
    L = oracle_lib.oracle()
    L.mxo_allreduce.argtypes = [ci, ci, ci, ci, sz, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.mxo_allreduce_segring.argtypes = [ci, ci, ci, sz, ctypes.POINTER(vp), sz]
    L.mxo_reduce_scatter.argtypes = [ci, ci, ci, ci, ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    return L


def gen(t, op, count, seed):
    """Adversarial inputs: magnitudes spanning 16 decades (so FP order
    matters), NaN/-0 for MAX/MIN, ties for MAXLOC, 0/1 for bool.

    Types not named below get raw random bytes.  New cases should take their
    operands from op_values.edge_values, which knows every (op, type) pair
    (tests/test_pair_matrix_gpu.py); this generator stays as it is for the
    cases that already use it."""
    rng = np.random.default_rng(seed)
    es = mxompi.type_size(t)
    if t in ("FLOAT", "DOUBLE"):
        dt = np.float32 if t == "FLOAT" else np.float64
        v = (rng.uniform(-1, 1, count) * 10.0 ** rng.uniform(-8, 8, count)).astype(dt)
        if op in ("MAX", "MIN"):
            k = rng.integers(0, count, max(1, count // 16))
            v[k] = rng.choice(np.array([np.nan, -0.0, 0.0, np.inf, -np.inf], dt), len(k))
        if op == "PROD":
            v = rng.uniform(0.5, 2.0, count).astype(dt)
        return v.view(np.uint8)
    if t == "C_FLOAT_COMPLEX":
        v = rng.uniform(0.7, 1.4, 2 * count).astype(np.float32)
        return v.view(np.uint8)
    if t == "LONG_DOUBLE":
        v = (rng.uniform(-1, 1, count) * 10.0 ** rng.uniform(-8, 8, count)).astype(np.longdouble)
        return v.view(np.uint8).copy()
    if t == "FLOAT_INT":
        p = np.zeros(count, dtype=[("v", "<f4"), ("k", "<i4")])
        p["v"] = rng.integers(0, 3, count)
        p["k"] = rng.integers(-5, 5, count)
        return p.view(np.uint8)
    if t == "BOOL":
        return rng.integers(0, 2, count * es, dtype=np.uint8)
    return rng.integers(0, 256, count * es, dtype=np.uint8)


def _tree_oracle():
    from test_coll_tree import _oracle as tree_oracle
    return tree_oracle()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


CASES = [("SUM", "FLOAT"), ("SUM", "DOUBLE"), ("MAX", "FLOAT"), ("MIN", "DOUBLE"), ("SUM", "INT32_T"),
         ("PROD", "INT8_T"), ("MAXLOC", "FLOAT_INT"), ("PROD", "C_FLOAT_COMPLEX"), ("SUM", "LONG_DOUBLE"),
         ("BXOR", "UINT16_T"), ("LAND", "BOOL"), ("MAXLOC", "DOUBLE_INT"), ("MINLOC", "SHORT_INT"),
         ("MAXLOC", "LONG_DOUBLE_INT")]
ALGS = ["auto", "basic_linear", "recursive_doubling", "ring", "segmented_ring", "rabenseifner"]
ALG_ID = {"auto": 0, "basic_linear": 1, "recursive_doubling": 3, "ring": 4, "segmented_ring": 5,
          "rabenseifner": 6}


@pytest.fixture(scope="module", autouse=True)
def _init():
    assert torch.cuda.is_available()
    mxompi.init(0)


def _check_allreduce_local(n, count, op, t, alg, inplace=False, seed=0):
    L = _oracle()
    es = mxompi.type_size(t)
    xs = [gen(t, op, count, seed * 100 + r) for r in range(n)]
    exp = [np.zeros(count * es, np.uint8) for _ in range(n)]
    sp = (vp * n)(*[x.ctypes.data for x in xs])
    rp = (vp * n)(*[e.ctypes.data for e in exp])
    assert L.mxo_allreduce(ALG_ID[alg], mxompi.OP[op], mxompi.TYPE[t], n, count, sp, rp) == 0
    comm = mxompi.Comm.local(n)
    S = [_dev(x) for x in xs]
    R = [torch.zeros(count * es, dtype=torch.uint8, device="cuda") for _ in range(n)]
    if inplace:
        comm.allreduce_local([mxompi.IN_PLACE] * n, [s.data_ptr() for s in S], count, t, op, alg, _stream())
        R = S
    else:
        comm.allreduce_local([s.data_ptr() for s in S], [r.data_ptr() for r in R], count, t, op, alg, _stream())
    for r in range(n):
        golden_io.assert_coll_equal(R[r].cpu().numpy(), exp[r], mxompi.OP[op], mxompi.TYPE[t],
                                  f"allreduce {alg} n={n} count={count} {op} {t} rank {r}")
    comm.close()


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8])
@pytest.mark.parametrize("op,t", CASES)
def test_allreduce_local_bitexact(alg, n, op, t):
    for count in (1, 3, n, 7, 100, 1001):
        _check_allreduce_local(n, count, op, t, alg, seed=count)


@pytest.mark.parametrize("alg", ["ring", "rabenseifner", "recursive_doubling"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_allreduce_local_inplace(alg, n):
    _check_allreduce_local(n, 4099, "SUM", "FLOAT", alg, inplace=True, seed=5)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_allreduce_auto_segmented_large(n):
    """auto at > n * 1 MiB selects the segmented ring (tuned :72-85)."""
    count = (n * (1 << 20)) // 4 + 12345
    assert mxompi.allreduce_decision(n, count, "FLOAT") == 5
    _check_allreduce_local(n, count, "SUM", "FLOAT", "auto", seed=11)


RS_ALGS = {"auto": 0, "recursive_halving": 2, "ring": 3}


@pytest.mark.parametrize("alg", list(RS_ALGS))
@pytest.mark.parametrize("n", [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize("op,t", [("SUM", "FLOAT"), ("MAX", "DOUBLE"), ("MAXLOC", "FLOAT_INT"), ("SUM", "INT64_T")])
@pytest.mark.parametrize("inplace", [False, True])
def test_reduce_scatter_local_bitexact(alg, n, op, t, inplace):
    L = _oracle()
    es = mxompi.type_size(t)
    rng = np.random.default_rng(n * 13 + len(op))
    for rc in ([0] * (n - 1) + [5], [int(x) for x in rng.integers(0, 300, n)], [1000] * n):
        total = sum(rc)
        if total == 0:
            continue
        xs = [gen(t, op, total, 50 + r) for r in range(n)]
        exp = [np.zeros(max(1, c) * es, np.uint8) for c in rc]
        assert L.mxo_reduce_scatter(RS_ALGS[alg], mxompi.OP[op], mxompi.TYPE[t], n, (sz * n)(*rc),
                                    (vp * n)(*[x.ctypes.data for x in xs]),
                                    (vp * n)(*[e.ctypes.data for e in exp])) == 0
        comm = mxompi.Comm.local(n)
        S = [_dev(x) for x in xs]
        if inplace:
            comm.reduce_scatter_local(None, [s.data_ptr() for s in S], rc, t, op, alg, _stream())
            R = S
        else:
            R = [torch.zeros(max(1, c) * es, dtype=torch.uint8, device="cuda") for c in rc]
            comm.reduce_scatter_local([s.data_ptr() for s in S], [r.data_ptr() for r in R], rc, t, op, alg,
                                      _stream())
        for r in range(n):
            got = R[r].cpu().numpy()[: rc[r] * es]
            golden_io.assert_coll_equal(got, exp[r][: rc[r] * es], mxompi.OP[op], mxompi.TYPE[t],
                                      f"reduce_scatter {alg} n={n} rc={rc} rank {r}")
        comm.close()


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("nbytes", [1, 13, 4096, 100003])
def test_allgather_and_bcast_local(n, nbytes):
    rng = np.random.default_rng(nbytes + n)
    xs = [rng.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(n)]
    comm = mxompi.Comm.local(n)
    S = [_dev(x) for x in xs]
    R = [torch.zeros(n * nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)]
    comm.allgather_local([s.data_ptr() for s in S], [r.data_ptr() for r in R], nbytes, _stream())
    full = np.concatenate(xs)
    for r in range(n):
        np.testing.assert_array_equal(R[r].cpu().numpy(), full)
    root = n - 1
    comm.bcast_local([s.data_ptr() for s in S], nbytes, root, _stream())
    for r in range(n):
        np.testing.assert_array_equal(S[r].cpu().numpy(), xs[root])
    comm.close()


# ---------------------------------------------------------------------------
# multi-process: n processes on the one GPU, IPC staging + flags
# ---------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _mp_worker(rank, n, port, staging, jobs, q, env=None):
    import torch.distributed as dist
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    os.environ.update(env or {})
    try:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n)
        torch.cuda.set_device(0)
        mxompi.init(0)

        def ag(b):
            out = [None] * n
            dist.all_gather_object(out, b)
            return out

        comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=staging, heap_bytes=160 << 20)
        comm.set_timeout(30.0)
        results = []
        st = torch.cuda.current_stream().cuda_stream
        for kind, count, op, t, alg in jobs:
            es = mxompi.type_size(t)
            if kind == "allreduce":
                x = _dev(gen(t, op, count, 7000 + rank))
                out = torch.zeros(count * es, dtype=torch.uint8, device="cuda")
                comm.allreduce(x.data_ptr(), out.data_ptr(), count, t, op, alg, st)
                results.append(out.cpu().numpy().tobytes())
            elif kind == "allreduce_inplace":
                x = _dev(gen(t, op, count, 7000 + rank))
                comm.allreduce(mxompi.IN_PLACE, x.data_ptr(), count, t, op, alg, st)
                results.append(x.cpu().numpy().tobytes())
            elif kind == "allreduce_mis":
                # this rank's buffers at a rank-dependent misalignment mod 16:
                # the registered path must decline on every rank together
                x = _dev(gen(t, op, count, 7000 + rank))
                sh = (rank % (16 // es)) * es if 16 % es == 0 else 0   # < 16: inside the padding
                xs = torch.zeros(count * es + 16, dtype=torch.uint8, device="cuda")
                xs[sh:sh + count * es].copy_(x)
                out = torch.zeros(count * es + 16, dtype=torch.uint8, device="cuda")
                comm.allreduce(xs.data_ptr() + sh, out.data_ptr() + sh, count, t, op, alg, st)
                results.append(out[sh:sh + count * es].cpu().numpy().tobytes())
            elif kind in ("stats", "stats_reset"):
                sts = comm.stats(reset=kind == "stats_reset")
                results.append((sts["zero_copy_calls"], sts["staged_calls"]))
            elif kind == "direct_stats":
                results.append(comm.stats()["direct_calls"])
            elif kind == "zc_direct":
                # zero-copy results straight into the peers' rbufs, or through the gather areas
                comm.set_zc_direct(alg == "on")
                results.append(None)
            elif kind == "path":
                # force the data path of the next allreduces (same on every rank)
                comm.set_autotune(alg == "autotune")
                comm.set_oneshot_max({"one_shot": 1 << 20, "autotune": 128 << 10}.get(alg, 0))
                comm.set_reg_min({"zero_copy": 1, "autotune": 256 << 10}.get(alg, 0))
                comm.set_protocol({"pull": "pull", "push": "push"}.get(alg, "auto"))
                results.append(None)
            elif kind == "recreate":
                # free the communicator and make a new one over the same ranks
                # (MPI_Comm_free + MPI_Comm_dup): its regions come from the pool
                comm.close()
                comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=staging, heap_bytes=160 << 20)
                comm.set_timeout(30.0)
                results.append(None)
            elif kind.startswith("tuning"):   # tuning[_<coll>]: the kept choice for that size class
                results.append(comm.tuning(count * es, kind[7:] or "allreduce"))
            elif kind == "reduce_scatter":
                rc = [count + 3 * r for r in range(n)]
                x = _dev(gen(t, op, sum(rc), 7000 + rank))
                out = torch.zeros(rc[rank] * es + 1, dtype=torch.uint8, device="cuda")
                comm.reduce_scatter(x.data_ptr(), out.data_ptr(), rc, t, op, alg, st)
                results.append(out.cpu().numpy()[: rc[rank] * es].tobytes())
            elif kind == "reduce_scatter_inplace":
                rc = [count + 3 * r for r in range(n)]
                x = _dev(gen(t, op, sum(rc), 7000 + rank))
                comm.reduce_scatter(mxompi.IN_PLACE, x.data_ptr(), rc, t, op, alg, st)
                results.append(x.cpu().numpy()[: rc[rank] * es].tobytes())
            elif kind == "allgather":
                x = _dev(gen("UINT8_T", "BAND", count, 7000 + rank))
                out = torch.zeros(n * count, dtype=torch.uint8, device="cuda")
                comm.allgather(x.data_ptr(), out.data_ptr(), count, st)
                results.append(out.cpu().numpy().tobytes())
            elif kind == "shmem":
                # shmem_float_max_to_all (examples/oshmem_max_reduction.c:46) -> MPI_MAX / MPI_FLOAT
                x = _dev(gen("FLOAT", "MAX", count, 7000 + rank))
                out = torch.zeros(count * 4, dtype=torch.uint8, device="cuda")
                comm.shmem_reduce("MAX", "FLOAT", 4, out.data_ptr(), x.data_ptr(), count, st)
                results.append(out.cpu().numpy().tobytes())
            elif kind == "shmem_basic":
                # scoll/basic's recursive-doubling shmem_<t>_<op>_to_all (alg = the shmem type)
                mt = _SHMEM_MPI[alg]
                es = mxompi.type_size(mt)
                x = _dev(gen(mt, op, count, 7000 + rank))
                out = torch.zeros(count * es, dtype=torch.uint8, device="cuda")
                comm.shmem_reduce_basic(op, alg, es, out.data_ptr(), x.data_ptr(), count, st)
                results.append(out.cpu().numpy().tobytes())
            elif kind == "shmem_big":
                # > INT_MAX elements: scoll/mpi falls back to scoll/basic
                # (shmem_short_max_to_all; inputs made on the device from
                # per-rank seeds, the result checked there)
                def src_of(r):
                    g = torch.Generator(device="cuda").manual_seed(99 + r)
                    return torch.randint(-32768, 32768, (count,), dtype=torch.int16, device="cuda", generator=g)
                x = src_of(rank)
                out = torch.empty(count, dtype=torch.int16, device="cuda")
                comm.shmem_reduce("MAX", "SHORT", 2, out.data_ptr(), x.data_ptr(), count, st)
                exp = src_of(0)
                for r in range(1, n):
                    exp = torch.maximum(exp, src_of(r))
                results.append(int((out != exp).sum().item()))
                del x, out, exp
                torch.cuda.empty_cache()
            elif kind == "oshmem_max_example":
                # examples/oshmem_max_reduction.c:36-46: long src[N] = my_pe + i,
                # shmem_long_max_to_all(dst, src, N, 0, 0, num_pes, ...) -- through
                # scoll/mpi (MPI_LONG MAX allreduce) and on the device symmetric heap
                src = torch.tensor([rank + i for i in range(count)], dtype=torch.int64, device="cuda")
                dst = torch.full((count,), -1, dtype=torch.int64, device="cuda")
                comm.shmem_reduce("MAX", "LONG", 8, dst.data_ptr(), src.data_ptr(), count, st)
                heap = mxompi.Heap(comm, 1 << 20)
                hs, hd = heap.alloc(count * 8), heap.alloc(count * 8)
                mxompi.lib().mx_copy(hs, src.data_ptr(), count * 8, None)
                mxompi.sync()
                heap.barrier_all()
                heap.reduce("MAX", "LONG", 8, hd, hs, count)
                hdst = torch.empty(count, dtype=torch.int64, device="cuda")
                mxompi.lib().mx_copy(hdst.data_ptr(), hd, count * 8, None)
                mxompi.sync()
                heap.barrier_all()
                heap.free(hd)
                heap.free(hs)
                heap.close()
                results.append((dst.cpu().tolist(), hdst.cpu().tolist()))
            elif kind in ("bcast", "bcast_root0"):
                x = _dev(gen("UINT8_T", "BAND", count, 7000 + rank))
                comm.bcast(x.data_ptr(), count, n - 1 if kind == "bcast" else 0, st)
                results.append(x.cpu().numpy().tobytes())
            elif kind in ("reduce", "reduce_inplace"):
                root = n - 1 if kind == "reduce" else 0
                x = _dev(gen(t, op, count, 7000 + rank))
                out = torch.zeros(count * es, dtype=torch.uint8, device="cuda")
                if kind == "reduce_inplace" and rank == root:
                    comm.reduce(mxompi.IN_PLACE, x.data_ptr(), count, t, op, root, alg, st)
                    out = x
                else:
                    comm.reduce(x.data_ptr(), out.data_ptr() if rank == root else 0, count, t, op, root, alg, st)
                results.append(out.cpu().numpy().tobytes() if rank == root else b"")
            elif kind in ("scan", "exscan"):
                x = _dev(gen(t, op, count, 7000 + rank))
                out = torch.zeros(count * es, dtype=torch.uint8, device="cuda")
                getattr(comm, kind)(x.data_ptr(), out.data_ptr(), count, t, op, alg, st)
                results.append(out.cpu().numpy().tobytes())
            elif kind == "symheap":
                # device symmetric heap: put / get / barrier / shmem_<t>_<op>_to_all
                heap = mxompi.Heap(comm, 64 << 20)
                nb = count * es
                src = heap.alloc(nb)
                tgt = heap.alloc(nb)
                scratch = heap.alloc(nb)
                x = _dev(gen(t, op, count, 7000 + rank))
                ctypes.memmove  # noqa: B018 (keeps the import used)
                torch.cuda.synchronize()
                mxompi.lib().mx_copy(src, x.data_ptr(), nb, None)
                mxompi.sync()
                heap.barrier_all()
                heap.put(scratch, src, nb, (rank + 1) % n)       # my source -> right neighbour's scratch
                heap.barrier_all()
                got_put = torch.empty(nb, dtype=torch.uint8, device="cuda")
                mxompi.lib().mx_copy(got_put.data_ptr(), scratch, nb, None)
                got_get = torch.empty(nb, dtype=torch.uint8, device="cuda")
                heap.get(got_get.data_ptr(), src, nb, (rank + n - 1) % n)   # left neighbour's source
                sops = {"SUM": "SUM", "MAX": "MAX", "MIN": "MIN", "PROD": "PROD", "BAND": "AND", "BXOR": "XOR"}
                sts = {"FLOAT": "FLOAT", "DOUBLE": "DOUBLE", "INT32_T": "INT32", "INT64_T": "INT64"}
                heap.reduce(sops[op], sts[t], es, tgt, src, count)                      # all PEs
                red_all = torch.empty(nb, dtype=torch.uint8, device="cuda")
                mxompi.lib().mx_copy(red_all.data_ptr(), tgt, nb, None)
                mxompi.sync()
                if n >= 3 and rank >= 1:                                             # active set 1..n-1
                    heap.reduce(sops[op], sts[t], es, src, src, count, 1, 0, n - 1)      # in place
                red_sub = torch.empty(nb, dtype=torch.uint8, device="cuda")
                mxompi.lib().mx_copy(red_sub.data_ptr(), src, nb, None)
                mxompi.sync()
                heap.barrier_all()
                results.append((got_put.cpu().numpy().tobytes(), got_get.cpu().numpy().tobytes(),
                                red_all.cpu().numpy().tobytes(), red_sub.cpu().numpy().tobytes()))
                heap.free(scratch)
                heap.free(tgt)
                heap.free(src)
                heap.close()
            elif kind == "reduce_scatter_block":
                x = _dev(gen(t, op, count * n, 7000 + rank))
                comm.reduce_scatter_block(mxompi.IN_PLACE, x.data_ptr(), count, t, op, alg, st)
                results.append(x.cpu().numpy()[: count * es].tobytes())
            elif kind == "reduce_scatter_block_oop":
                x = _dev(gen(t, op, count * n, 7000 + rank))
                out = torch.zeros(count * es, dtype=torch.uint8, device="cuda")
                comm.reduce_scatter_block(x.data_ptr(), out.data_ptr(), count, t, op, alg, st)
                results.append(out.cpu().numpy().tobytes())
        comm.close()
        dist.destroy_process_group()
        q.put((rank, "ok", results))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc() + str(e)))


def _run_mp(n, jobs, staging=1 << 20, env=None):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mp_worker, args=(r, n, port, staging, jobs, q, env)) for r in range(n)]
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


_JOBS = [("allreduce", 100003, "SUM", "FLOAT", "auto"),          # > staging: chunked
        ("allreduce", 777, "MAX", "DOUBLE", "rabenseifner"),
        ("allreduce", 5, "SUM", "FLOAT", "recursive_doubling"),
        ("allreduce_inplace", 4099, "SUM", "DOUBLE", "ring"),
        ("allreduce", 3001, "MAXLOC", "FLOAT_INT", "auto"),
        ("reduce_scatter", 1000, "SUM", "FLOAT", "ring"),
        ("reduce_scatter", 10, "SUM", "DOUBLE", "recursive_halving"),
        ("reduce_scatter", 300001, "SUM", "FLOAT", "ring"),              # blocks > staging: chunked
        ("reduce_scatter_inplace", 200003, "SUM", "DOUBLE", "recursive_halving"),
        ("allgather", 300001, None, None, None),
        ("shmem", 5003, "MAX", "FLOAT", "auto"),
        ("bcast", 2000003, None, None, None),
        ("bcast_root0", 5, None, None, None),        # fewer bytes than non-roots: empty parts
        ("bcast_root0", 1000001, None, None, None),
        # back-to-back one-shot calls (both staging parities, every fold shape)
        ("allreduce", 1000, "SUM", "FLOAT", "auto"),
        ("allreduce", 3000, "SUM", "FLOAT", "ring"),
        ("allreduce_inplace", 333, "PROD", "LONG_DOUBLE", "auto"),
        ("allreduce", 1999, "MAXLOC", "DOUBLE_INT", "rabenseifner"),
        ("allreduce", 1, "MIN", "INT64_T", "auto"),
        ("allreduce", 17, "SUM", "DOUBLE", "basic_linear"),
        ("allreduce", 200003, "SUM", "FLOAT", "segmented_ring"),   # chunked path in between
        ("allreduce", 2500, "BXOR", "UINT16_T", "auto"),
        ("allreduce_inplace", 4000, "SUM", "FLOAT", "auto"),
        # above the one-shot range within one staging round: every fold
        # shape, element path (x87, pair types) and 16-byte path, in place
        ("allreduce", 30001, "SUM", "FLOAT", "auto"),
        ("allreduce", 20011, "MAX", "DOUBLE", "rabenseifner"),
        ("allreduce_inplace", 40000, "SUM", "FLOAT", "ring"),
        ("allreduce", 9001, "MAXLOC", "FLOAT_INT", "segmented_ring"),
        ("allreduce", 50001, "BAND", "UINT16_T", "auto"),
        ("allreduce", 5001, "SUM", "LONG_DOUBLE", "recursive_doubling"),
        ("allreduce", 12345, "PROD", "C_FLOAT_COMPLEX", "basic_linear"),
        ("allreduce", 30001, "SUM", "FLOAT", "auto"),                  # back to back
        # rooted reduce / scan / exscan / reduce_scatter_block (VM fold)
        ("reduce", 100003, "SUM", "FLOAT", "auto"),                 # chunked
        ("reduce", 3001, "MAX", "DOUBLE", "binary"),
        ("reduce_inplace", 5000, "MAX", "FLOAT", "binomial"),       # root's IN_PLACE variant
        ("reduce_inplace", 777, "MAXLOC", "FLOAT_INT", "pipeline"),
        ("reduce", 999, "SUM", "DOUBLE", "in_order_binary"),
        ("scan", 20001, "SUM", "FLOAT", "auto"),
        ("exscan", 4097, "SUM", "DOUBLE", "recursive_doubling"),
        ("scan", 333, "MIN", "FLOAT", "recursive_doubling"),
        ("reduce_scatter_block", 3000, "SUM", "FLOAT", "auto"),
        ("symheap", 30001, "SUM", "FLOAT", "auto"),
        ("symheap", 777, "MAX", "DOUBLE", "auto")]
_JOBS = [(k, c, o or "BAND", t or "UINT8_T", a or "auto") for k, c, o, t, a in _JOBS]


def _check_jobs(n, jobs, got):
    L = _oracle()
    for j, (kind, count, op, t, alg) in enumerate(jobs):
        es = mxompi.type_size(t)
        if kind in ("stats", "direct_stats", "zc_direct") or kind.startswith("tuning"):
            continue
        if kind.startswith("allreduce") or kind == "shmem":
            xs = [gen(t, op, count, 7000 + r) for r in range(n)]
            exp = [np.zeros(count * es, np.uint8) for _ in range(n)]
            assert L.mxo_allreduce(ALG_ID[alg], mxompi.OP[op], mxompi.TYPE[t], n, count,
                                   (vp * n)(*[x.ctypes.data for x in xs]),
                                   (vp * n)(*[e.ctypes.data for e in exp])) == 0
            for r in range(n):
                golden_io.assert_coll_equal(np.frombuffer(got[r][j], np.uint8), exp[r], mxompi.OP[op],
                                          mxompi.TYPE[t], f"{kind} {alg} rank {r}")
        elif kind in ("reduce_scatter", "reduce_scatter_inplace"):
            rc = [count + 3 * r for r in range(n)]
            xs = [gen(t, op, sum(rc), 7000 + r) for r in range(n)]
            exp = [np.zeros(c * es, np.uint8) for c in rc]
            assert L.mxo_reduce_scatter({"ring": 3, "recursive_halving": 2}[alg], mxompi.OP[op], mxompi.TYPE[t],
                                        n, (sz * n)(*rc), (vp * n)(*[x.ctypes.data for x in xs]),
                                        (vp * n)(*[e.ctypes.data for e in exp])) == 0
            for r in range(n):
                golden_io.assert_coll_equal(np.frombuffer(got[r][j], np.uint8), exp[r], mxompi.OP[op],
                                          mxompi.TYPE[t], f"reduce_scatter {alg} rank {r}")
        elif kind in ("reduce", "reduce_inplace"):
            root = n - 1 if kind == "reduce" else 0
            xs = [gen(t, op, count, 7000 + r) for r in range(n)]
            exp = np.zeros(count * es, np.uint8)
            sp = [x.ctypes.data for x in xs]
            if kind == "reduce_inplace":
                exp[:] = xs[root]
                sp[root] = None
            T = _tree_oracle()
            assert T.mxo_reduce({"auto": 0, "binary": 4, "binomial": 5, "pipeline": 3, "in_order_binary": 6}[alg],
                                mxompi.OP[op], mxompi.TYPE[t], n, count, root, (vp * n)(*sp), exp.ctypes.data) == 0
            golden_io.assert_coll_equal(np.frombuffer(got[root][j], np.uint8), exp, mxompi.OP[op], mxompi.TYPE[t],
                                        f"{kind} {alg} root {root}")
        elif kind in ("scan", "exscan"):
            xs = [gen(t, op, count, 7000 + r) for r in range(n)]
            exp = [np.zeros(count * es, np.uint8) for _ in range(n)]
            T = _tree_oracle()
            fn = T.mxo_scan if kind == "scan" else T.mxo_exscan
            assert fn(mxompi.SCAN[alg], mxompi.OP[op], mxompi.TYPE[t], n, count,
                      (vp * n)(*[x.ctypes.data for x in xs]), (vp * n)(*[e.ctypes.data for e in exp])) == 0
            for r in range(1 if kind == "exscan" else 0, n):
                golden_io.assert_coll_equal(np.frombuffer(got[r][j], np.uint8), exp[r], mxompi.OP[op],
                                            mxompi.TYPE[t], f"{kind} {alg} rank {r}")
        elif kind == "symheap":
            xs = [gen(t, op, count, 7000 + r) for r in range(n)]
            exp = [np.zeros(count * es, np.uint8) for _ in range(n)]
            assert L.mxo_allreduce(0, mxompi.OP[op], mxompi.TYPE[t], n, count, (vp * n)(*[x.ctypes.data for x in xs]),
                                   (vp * n)(*[e.ctypes.data for e in exp])) == 0
            sub = None
            if n >= 3:
                sub = [np.zeros(count * es, np.uint8) for _ in range(n - 1)]
                assert L.mxo_allreduce(0, mxompi.OP[op], mxompi.TYPE[t], n - 1, count,
                                       (vp * (n - 1))(*[x.ctypes.data for x in xs[1:]]),
                                       (vp * (n - 1))(*[e.ctypes.data for e in sub])) == 0
            for r in range(n):
                put_b, get_b, all_b, sub_b = got[r][j]
                np.testing.assert_array_equal(np.frombuffer(put_b, np.uint8), xs[(r + n - 1) % n])
                np.testing.assert_array_equal(np.frombuffer(get_b, np.uint8), xs[(r + n - 1) % n])
                golden_io.assert_coll_equal(np.frombuffer(all_b, np.uint8), exp[r], mxompi.OP[op], mxompi.TYPE[t],
                                            f"symheap reduce rank {r}")
                if sub is not None and r >= 1:
                    golden_io.assert_coll_equal(np.frombuffer(sub_b, np.uint8), sub[r - 1], mxompi.OP[op],
                                                mxompi.TYPE[t], f"symheap active-set reduce rank {r}")
                elif sub is not None:
                    np.testing.assert_array_equal(np.frombuffer(sub_b, np.uint8), xs[0])   # PE 0 not in the set
        elif kind in ("reduce_scatter_block", "reduce_scatter_block_oop"):
            xs = [gen(t, op, count * n, 7000 + r) for r in range(n)]
            exp = [np.zeros(count * es, np.uint8) for _ in range(n)]
            T = _tree_oracle()
            assert T.mxo_reduce_scatter_block(0, mxompi.OP[op], mxompi.TYPE[t], n, count,
                                              (vp * n)(*[x.ctypes.data for x in xs]),
                                              (vp * n)(*[e.ctypes.data for e in exp])) == 0
            for r in range(n):
                golden_io.assert_coll_equal(np.frombuffer(got[r][j], np.uint8), exp[r], mxompi.OP[op],
                                            mxompi.TYPE[t], f"reduce_scatter_block rank {r}")
        elif kind == "allgather":
            full = np.concatenate([gen("UINT8_T", "BAND", count, 7000 + r) for r in range(n)])
            for r in range(n):
                np.testing.assert_array_equal(np.frombuffer(got[r][j], np.uint8), full)
        elif kind in ("bcast", "bcast_root0"):
            root = gen("UINT8_T", "BAND", count, 7000 + (n - 1 if kind == "bcast" else 0))
            for r in range(n):
                np.testing.assert_array_equal(np.frombuffer(got[r][j], np.uint8), root)


@pytest.mark.parametrize("n", [2, 3, 4])
def test_multiprocess_ipc_bitexact(n):
    _check_jobs(n, _JOBS, _run_mp(n, _JOBS))


# the driver's 8-GPU run reaches these at n = 8: every slot's 8-rank masks,
# one-shot and chunked allreduce, scatter + allgather bcast from two roots
_JOBS8 = [j for j in _JOBS if (j[0], j[1]) in {
    ("allreduce", 100003), ("allreduce", 777), ("allreduce", 1000), ("reduce_scatter", 300001),
    ("allgather", 300001), ("bcast", 2000003), ("bcast_root0", 5), ("bcast_root0", 1000001),
    ("reduce", 100003), ("scan", 20001), ("shmem", 5003), ("allreduce", 3001), ("allreduce", 30001),
    ("allreduce", 20011)}]


def test_multiprocess_ipc_bitexact_8_ranks():
    assert len(_JOBS8) >= 10
    _check_jobs(8, _JOBS8, _run_mp(8, _JOBS8))


# the staged protocols (mx_comm_set_protocol; PULL is the default): same fold
# programs, PULL reads the peers' parts over IPC from their own staging, PUSH
# writes them into the owner's staging first.  Every staged allreduce
# shape of _JOBS (chunked, in place, element / 16-byte paths, every algorithm)
# plus a rooted reduce between them (same staging, other layout)
_JOBS_PULL = [j for j in _JOBS if j[0].startswith("allreduce")] + [("reduce", 100003, "SUM", "FLOAT", "auto"),
                                                                   ("allreduce", 100003, "SUM", "FLOAT", "auto")]


# zero-copy allreduce between registered user buffers (mx_comm_set_reg_min):
# every staged shape of _JOBS folded straight between the ranks' own buffers,
# in place, chunk-sized counts, and a call whose ranks disagree on alignment
# (every rank falls back to the staged path together)
_JOBS_ZC = [j for j in _JOBS if j[0].startswith(("allreduce", "reduce_scatter", "allgather", "bcast", "reduce",
                                                  "scan", "exscan"))
            and j[0] != "reduce_scatter_block"] + [
    ("allreduce_mis", 30001, "SUM", "FLOAT", "auto"),
    ("allreduce_mis", 20011, "MAX", "DOUBLE", "ring"),
    ("allreduce", 100003, "SUM", "FLOAT", "auto"),
    ("allgather", 65536, "BAND", "UINT8_T", "auto"),
    ("reduce_scatter_block_oop", 4096, "SUM", "FLOAT", "auto"),
    ("reduce_scatter_block", 3000, "SUM", "FLOAT", "auto"),      # IN_PLACE: staged
    ("stats", 0, "SUM", "FLOAT", "auto")]


@pytest.mark.parametrize("n,direct", [(2, True), (3, True), (8, True), (2, False), (8, False)],
                         ids=["2-direct", "3-direct", "8-direct", "2-gather", "8-gather"])
def test_multiprocess_allreduce_zero_copy(n, direct):
    """direct: every zero-copy allreduce's results go straight into the peers'
    rbufs (the default); gather: through the peers' uncached gather areas and a
    local gather copy (round 4's path, mx_comm_set_zc_direct(0))."""
    import glob
    before = set(glob.glob("/dev/shm/mx_reg_*"))
    env = {"MX_REG_MIN": "1", "MX_ONESHOT_MAX": "0"}
    jobs = [("zc_direct", 0, "SUM", "FLOAT", "on" if direct else "off")] + _JOBS_ZC + \
        [("direct_stats", 0, "SUM", "FLOAT", "auto")]
    got = _run_mp(n, jobs, env=env)
    assert set(glob.glob("/dev/shm/mx_reg_*")) <= before, "registration page left in /dev/shm"
    _check_jobs(n, jobs, got)
    zc, staged = got[0][-2]
    n_direct = got[0][-1]
    if direct:
        # every zero-copy allreduce of the list whose sbuf and rbuf share a
        # misalignment (all of them here) took the direct path
        n_ar = sum(1 for j in _JOBS_ZC if j[0] in ("allreduce", "allreduce_inplace") and "nonoverlapping" not in j[4])
        assert n_direct == n_ar, (n_direct, n_ar)
    else:
        assert n_direct == 0

    def eligible(kind, count, t):
        # registered path: every rank's blocks at one misalignment mod 16
        # (IN_PLACE reduce_scatter stays staged; neither counts it)
        if kind in ("allreduce", "allreduce_inplace", "bcast", "bcast_root0", "reduce", "reduce_inplace", "scan",
                    "exscan"):
            return True
        if kind == "reduce_scatter":
            rc, es = [count + 3 * r for r in range(n)], mxompi.type_size(t)
            return all(sum(rc[:r]) * es % 16 == 0 for r in range(n))
        if kind == "allgather":
            return count % 16 == 0
        if kind == "reduce_scatter_block_oop":
            return count * mxompi.type_size(t) % 16 == 0
        return False
    n_mis = sum(1 for j in _JOBS_ZC if j[0] == "allreduce_mis")
    n_zc = sum(1 for j in _JOBS_ZC if eligible(j[0], j[1], j[3]))
    assert staged == n_mis and zc == n_zc, (zc, staged, n_zc)
    for r in range(n):
        assert got[r][-2:] == got[0][-2:]


# autotuning (mx_comm_set_autotune, on by default): five allreduces of one
# size class -- warm-up, zero-copy, PULL and PUSH trials, then the kept choice
# -- all bit-exact, every rank keeping the same choice
_JOBS_TUNE = [("allreduce", 1_500_001, "SUM", "FLOAT", "auto"),
              ("allreduce_inplace", 1_500_001, "SUM", "FLOAT", "auto"),
              ("allreduce", 1_500_001, "MAX", "FLOAT", "rabenseifner"),
              ("allreduce", 1_500_001, "SUM", "FLOAT", "ring"),
              ("allreduce", 1_500_001, "BAND", "UINT16_T", "auto"),      # another size class: untuned
              ("tuning", 1_500_001, "SUM", "FLOAT", "auto"),
              ("allreduce", 1_500_001, "SUM", "FLOAT", "auto"),
              ("tuning", 1_500_001, "SUM", "FLOAT", "auto"),
              # reduce_scatter and allgather: warm-up, zero-copy and staged trials, kept choice
              *[("reduce_scatter", 600_000, "SUM", "FLOAT", "ring")] * 4,
              *[("allgather", 2_500_000, "BAND", "UINT8_T", "auto")] * 4]


@pytest.mark.parametrize("n", [2, 8])
def test_multiprocess_allreduce_autotune(n):
    got = _run_mp(n, _JOBS_TUNE, staging=64 << 20)
    _check_jobs(n, _JOBS_TUNE, got)
    for r in range(n):
        assert got[r][5] in ("zero_copy", "pull", "push"), got[r][5]   # the fp32 size class: 4 calls done
        assert got[r][5] == got[0][5] and got[r][7] == got[0][5]


# autotuning of the crossovers below 4 MiB: one-shot / zero-copy / PULL /
# PUSH for allreduces from 64 KiB (each candidate 3 times: 13 calls per size
# class), zero-copy / scatter / direct for bcasts from 64 KiB (n > 2: 10
# calls); every trial bit-exact, every rank keeping the same choice
_JOBS_TUNE_SMALL = [*[("allreduce", 40_000, "SUM", "FLOAT", "auto")] * 13,            # 160 KB
                    ("tuning", 40_000, "SUM", "FLOAT", "auto"),
                    *[("allreduce", 200_000, "SUM", "FLOAT", "auto")] * 13,           # 800 KB
                    ("tuning", 200_000, "SUM", "FLOAT", "auto"),
                    *[("bcast", 300_000, "BAND", "UINT8_T", "auto")] * 10,
                    ("tuning_bcast", 300_000, "BAND", "UINT8_T", "auto"),
                    ("allreduce", 200_000, "SUM", "FLOAT", "auto")]


@pytest.mark.parametrize("n", [2, 8])
def test_multiprocess_autotune_crossovers(n):
    got = _run_mp(n, _JOBS_TUNE_SMALL, staging=64 << 20)
    _check_jobs(n, _JOBS_TUNE_SMALL, got)
    idx = [j for j, job in enumerate(_JOBS_TUNE_SMALL) if job[0].startswith("tuning")]
    for r in range(n):
        for j in idx[:2]:
            assert got[r][j] in ("zero_copy", "pull", "push", "one_shot"), got[r][j]
        assert got[r][idx[2]] in (("zero_copy", "scatter", "direct") if n > 2 else (None,)), got[r][idx[2]]
        assert [got[r][j] for j in idx] == [got[0][j] for j in idx]


@pytest.mark.parametrize("env", [{"MX_FAST_SYNC_SPINS": "0"}, {"MX_FAST_SYNC": "0"}], ids=["fallback", "runtime"])
def test_multiprocess_blocking_completion_paths(env):
    """Blocking calls complete through the marker kernel's mapped word; with no
    polling budget every call takes the fallback (the runtime's wait), and
    MX_FAST_SYNC=0 uses the runtime's wait only: same results either way."""
    jobs = [j for j in _JOBS_ZC if j[0] != "stats"]
    _check_jobs(2, jobs, _run_mp(2, jobs, env=dict(env, MX_REG_MIN="1")))


@pytest.mark.parametrize("proto", ["push", "pull"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_multiprocess_allreduce_staged_protocols(n, proto):
    """Both staged data movements with registration off (the default path
    takes zero-copy above 256 KiB)."""
    env = {"MX_ALLREDUCE_PROTO": proto, "MX_ONESHOT_MAX": "0", "MX_REG_MIN": "0"}   # every call staged
    _check_jobs(n, _JOBS_PULL, _run_mp(n, _JOBS_PULL, env=env))


# ---------------------------------------------------------------------------
# round 4: the 8-rank wrong part of round 3
# ---------------------------------------------------------------------------
# The same 40001-float recursive-doubling allreduce (160,004 B per rank, the
# failing call of test_tuned_forced_rules_and_basic_orders[8-device]) on one
# communicator, its data path switched call to call: one-shot -> PULL ->
# zero-copy -> PUSH, twice, then autotuning on (warm-up + 12 trials + the
# kept choice).  Every call bit-exact vs the recursive-doubling oracle
# (coll_base_allreduce.c:130-274); the per-call counters prove each path ran.
_AR40K = ("allreduce", 40001, "SUM", "FLOAT", "recursive_doubling")
# shmem type -> the MPI type scoll/mpi maps it to (scoll_mpi_dtypes.h; FINT2 by size)
_SHMEM_MPI = {"FLOAT": "FLOAT", "DOUBLE": "DOUBLE", "FINT2": "INT16_T", "LONG": "INT64_T"}
_PATHS = ["one_shot", "pull", "zero_copy", "push"]
_JOBS_SWITCH = [j for _ in range(2) for p in _PATHS
                for j in (("path", 0, "SUM", "FLOAT", p), _AR40K, ("stats_reset", 0, "SUM", "FLOAT", "auto"))]
_JOBS_SWITCH += [("path", 0, "SUM", "FLOAT", "autotune")] + [_AR40K] * 14 + [("tuning", 40001, "SUM", "FLOAT", "auto")]


def test_allreduce_path_switching_8_ranks():
    got = _run_mp(8, _JOBS_SWITCH, staging=64 << 20)
    _check_jobs(8, _JOBS_SWITCH, got)
    counts = {"one_shot": (0, 0), "pull": (0, 1), "zero_copy": (1, 0), "push": (0, 1)}
    for r in range(8):
        seen = [got[r][j] for j, job in enumerate(_JOBS_SWITCH) if job[0] == "stats_reset"]
        assert seen == [counts[p] for p in _PATHS] * 2, (r, seen)
        assert got[r][-1] in ("zero_copy", "pull", "push", "one_shot") and got[r][-1] == got[0][-1]


# Communicators freed and re-made back to back (MPI_Comm_free + MPI_Comm_dup,
# what test_tuned_forced_rules_and_basic_orders does per configuration):
# the last call on each is a staged rooted reduce, whose non-roots never wait
# for the peers' PUSHED(g); one rank's trailing signals are held back 50 ms
# (fault injection, MX_DEBUG_LAG_*), so they land after every other rank has
# freed the communicator and made the next one.  Round 3 reused the freed
# flags at once and zeroed them at creation: the late PUSHED passed the next
# staged allreduce's PUSHED wait, and the lagging rank's part was gathered
# before it was written.  Now the regions stay in quarantine until every
# peer said BYE (mx_comm_destroy), so the new communicator gets others.
#  The op changes per cycle, so a part gathered early shows the previous
#  cycle's bytes instead of the same values again.
_JOBS_RECYCLE = [j for op in ("SUM", "MAX", "MIN", "SUM") for j in (
    ("allreduce", 3001, op, "FLOAT", "recursive_doubling"),          # one-shot
    ("allreduce", 40001, op, "FLOAT", "recursive_doubling"),         # staged PULL: waits PUSHED(2)
    ("reduce", 30001, "SUM", "FLOAT", "auto"),                       # staged VM, root n-1
    ("recreate", 0, "SUM", "FLOAT", "auto"))]


_JOBS_SHMEM_BASIC = [("shmem_basic", c, op, _SHMEM_MPI[st], st) for c, op, st in (
    (3001, "MAX", "FLOAT"), (20011, "SUM", "DOUBLE"), (5003, "MIN", "DOUBLE"), (4099, "SUM", "FINT2"),
    (3, "MAX", "LONG"), (300001, "SUM", "FLOAT"))]


def _check_shmem_basic(n, jobs, got):
    L = _oracle()
    L.mxo_shmem_basic_reduce.argtypes = [ci, ci, ci, sz, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    for j, (kind, count, op, _, st) in enumerate(jobs):
        if kind != "shmem_basic":
            continue
        mt = _SHMEM_MPI[st]
        es = mxompi.type_size(mt)
        xs = [gen(mt, op, count, 7000 + r) for r in range(n)]
        exp = [np.zeros(count * es, np.uint8) for _ in range(n)]
        assert L.mxo_shmem_basic_reduce(mxompi.OP[op], mxompi.TYPE[mt], n, count, (vp * n)(*[x.ctypes.data for x in xs]),
                                        (vp * n)(*[e.ctypes.data for e in exp])) == 0
        for r in range(n):
            golden_io.assert_coll_equal(np.frombuffer(got[r][j], np.uint8), exp[r], mxompi.OP[op], mxompi.TYPE[mt],
                                        f"shmem_basic {st} {op} n={n} PE {r}")


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_shmem_reduce_scoll_basic_order(n):
    """scoll/basic's recursive doubling (scoll_basic_reduce.c:374-542) on the
    device, every PE's result bit-exact vs the oracle's step-by-step
    restatement -- including MAX / MIN with NaNs and signed zeros, where the
    two PEs of a pair keep different values (each is the target of its own
    fold), non-powers of two (extras), FINT2 as 2-byte integers, and a
    zero-copy size."""
    _check_shmem_basic(n, _JOBS_SHMEM_BASIC, _run_mp(n, _JOBS_SHMEM_BASIC, staging=16 << 20))


def test_shmem_reduce_above_int_max_falls_back_to_scoll_basic():
    """2^31 + 5 shorts per PE (> INT_MAX elements, 4 GiB): mca_scoll_mpi_reduce
    hands such a count to scoll/basic (scoll_mpi_ops.c:246-259); the call
    completes and every element is the maximum over the PEs."""
    got = _run_mp(2, [("shmem_big", 2 ** 31 + 5, "MAX", "INT16_T", "auto")], staging=512 << 20)
    assert got[0][0] == 0 and got[1][0] == 0, got


@pytest.mark.parametrize("n", [2, 3, 8])
def test_oshmem_max_reduction_example(n):
    """The reference's one OpenSHMEM known answer (examples/oshmem_max_reduction.c:
    36-46, N = 3): after shmem_long_max_to_all every PE holds dst[i] = npes-1+i."""
    got = _run_mp(n, [("oshmem_max_example", 3, "MAX", "INT64_T", "auto")], staging=16 << 20)
    for r in range(n):
        staged, heap = got[r][0]
        assert staged == [n - 1 + i for i in range(3)], (r, staged)
        assert heap == [n - 1 + i for i in range(3)], (r, heap)


def test_communicator_recycling_with_a_late_peer_8_ranks():
    env = {"MX_AUTOTUNE": "0", "MX_DEBUG_LAG_RANK": "3", "MX_DEBUG_LAG_US": "50000"}
    _check_jobs(8, _JOBS_RECYCLE, _run_mp(8, _JOBS_RECYCLE, staging=64 << 20, env=env))



# ---------------------------------------------------------------------------
# a peer later than the wait timeout: poisoned communicator, no stale data
# ---------------------------------------------------------------------------
def _late_worker(rank, n, port, q):
    import time
    import torch.distributed as dist
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    try:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n)
        torch.cuda.set_device(0)
        mxompi.init(0)

        def ag(b):
            out = [None] * n
            dist.all_gather_object(out, b)
            return out

        comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=4 << 20)
        comm.set_timeout(2.0)
        st = torch.cuda.current_stream().cuda_stream
        count = 400_003                                   # staged path (> one-shot range)
        x = _dev(gen("FLOAT", "SUM", count, 7000 + rank))
        out = torch.zeros(count * 4, dtype=torch.uint8, device="cuda")
        comm.allreduce(x.data_ptr(), out.data_ptr(), count, "FLOAT", "SUM", "auto", st)   # both on time
        first = out.cpu().numpy().tobytes()
        dist.barrier()
        if rank == 1:
            time.sleep(5.0)                               # arrives after rank 0's wait gave up
        rcs = []
        for _ in range(2):
            t0 = time.time()
            try:
                comm.allreduce(x.data_ptr(), out.data_ptr(), count, "FLOAT", "SUM", "auto", st)
                rcs.append((0, time.time() - t0))
            except mxompi.MxError as e:
                rcs.append((e.rc, time.time() - t0))
        dist.barrier()
        comm.close()
        dist.destroy_process_group()
        q.put((rank, "ok", {"first": first, "rcs": rcs}))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc() + str(e)))


def test_late_peer_poisons_instead_of_corrupting():
    """Rank 1 enters the second allreduce 5 s late with a 2 s wait timeout.
    Rank 0's wait for rank 1's contribution times out: the copy / fold /
    signal kernels queued behind it do nothing, it returns MX_ERR_TIMEOUT,
    and its next call fails at once.  Rank 1 then finds rank 0's PUSHED
    signal never raised (rank 0 folded nothing) and times out too, instead
    of copying stale gather data and returning success."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_late_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(2):
            rank, status, payload = q.get(timeout=120)
            assert status == "ok", payload
            out[rank] = payload
    finally:
        for p in procs:
            p.join(timeout=30 if len(out) == 2 else 5)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    TIMEOUT = -5
    assert out[0]["first"] == out[1]["first"]
    (rc0a, _), (rc0b, t0b) = out[0]["rcs"]
    (rc1a, _), (rc1b, t1b) = out[1]["rcs"]
    assert rc0a == TIMEOUT and rc1a == TIMEOUT, out
    assert rc0b == TIMEOUT and rc1b == TIMEOUT, out          # poisoned: every later call fails
    assert t0b < 1.0 and t1b < 1.0, (t0b, t1b)               # ... without waiting again


# ---------------------------------------------------------------------------
# coll/tuned's forced algorithms beyond the fixed decision (round 3):
# allreduce 2 nonoverlapping (coll_base_allreduce.c:54-86: coll_reduce to 0 +
# bcast), reduce_scatter 1 nonoverlapping (coll_base_reduce_scatter.c:47-110:
# coll_reduce to 0 + scatterv) and 4 butterfly (:691-880), with the reduce
# algorithm and chain fanout coll_reduce would run carried in the word
# ---------------------------------------------------------------------------
WORDS_AR = [mxompi.alg_word(2, ra, fo) for ra, fo in ((0, 0), (1, 0), (2, 0), (2, 2), (3, 0), (4, 0), (5, 0),
                                                      (6, 0))]


@pytest.mark.parametrize("word", WORDS_AR, ids=lambda w: f"w{w:x}")
@pytest.mark.parametrize("n", [2, 3, 5, 8])
@pytest.mark.parametrize("op,t", [("SUM", "FLOAT"), ("MAX", "DOUBLE"), ("MAXLOC", "FLOAT_INT")])
@pytest.mark.parametrize("inplace", [False, True])
def test_allreduce_nonoverlapping_local(word, n, op, t, inplace):
    L = _oracle()
    es = mxompi.type_size(t)
    for count in (1, 5, 1001, 70001):
        xs = [gen(t, op, count, 700 + r) for r in range(n)]
        exp = [x.copy() if inplace else np.zeros(count * es, np.uint8) for x in xs]
        sp = None if inplace else (vp * n)(*[x.ctypes.data for x in xs])
        assert L.mxo_allreduce(word, mxompi.OP[op], mxompi.TYPE[t], n, count, sp,
                               (vp * n)(*[e.ctypes.data for e in exp])) == 0
        comm = mxompi.Comm.local(n)
        S = [_dev(x) for x in xs]
        if inplace:
            comm.allreduce_local([mxompi.IN_PLACE] * n, [s.data_ptr() for s in S], count, t, op, word, _stream())
            R = S
        else:
            R = [torch.zeros(count * es, dtype=torch.uint8, device="cuda") for _ in range(n)]
            comm.allreduce_local([s.data_ptr() for s in S], [r.data_ptr() for r in R], count, t, op, word, _stream())
        for r in range(n):
            golden_io.assert_coll_equal(R[r].cpu().numpy(), exp[r], mxompi.OP[op], mxompi.TYPE[t],
                                        f"allreduce word {word:#x} n={n} count={count} rank {r}")
        comm.close()


@pytest.mark.parametrize("word", [4, mxompi.alg_word(1), mxompi.alg_word(1, 1), mxompi.alg_word(1, 2, 3),
                                  mxompi.alg_word(1, 3), mxompi.alg_word(1, 5), mxompi.alg_word(1, 6)],
                         ids=lambda w: f"w{w:x}")
@pytest.mark.parametrize("n", [2, 3, 5, 8])
@pytest.mark.parametrize("op,t", [("SUM", "FLOAT"), ("MAXLOC", "FLOAT_INT"), ("SUM", "INT64_T")])
@pytest.mark.parametrize("inplace", [False, True])
def test_reduce_scatter_forced_local(word, n, op, t, inplace):
    L = _oracle()
    es = mxompi.type_size(t)
    rng = np.random.default_rng(n * 31 + word)
    for rc in ([0] * (n - 1) + [5], [int(x) for x in rng.integers(0, 300, n)], [2000] * n):
        total = sum(rc)
        xs = [gen(t, op, total, 90 + r) for r in range(n)]
        exp = [x.copy() if inplace else np.zeros(max(1, c) * es, np.uint8) for x, c in zip(xs, rc)]
        assert L.mxo_reduce_scatter(word, mxompi.OP[op], mxompi.TYPE[t], n, (sz * n)(*rc),
                                    None if inplace else (vp * n)(*[x.ctypes.data for x in xs]),
                                    (vp * n)(*[e.ctypes.data for e in exp])) == 0
        comm = mxompi.Comm.local(n)
        S = [_dev(x) for x in xs]
        if inplace:
            comm.reduce_scatter_local(None, [s.data_ptr() for s in S], rc, t, op, word, _stream())
            R = S
        else:
            R = [torch.zeros(max(1, c) * es, dtype=torch.uint8, device="cuda") for c in rc]
            comm.reduce_scatter_local([s.data_ptr() for s in S], [r.data_ptr() for r in R], rc, t, op, word,
                                      _stream())
        for r in range(n):
            golden_io.assert_coll_equal(R[r].cpu().numpy()[: rc[r] * es], exp[r][: rc[r] * es], mxompi.OP[op],
                                        mxompi.TYPE[t], f"reduce_scatter word {word:#x} n={n} rc={rc} rank {r}")
        comm.close()


# ---------------------------------------------------------------------------
# registration fast path (round 5): consecutive zero-copy calls on the same
# buffers skip the verdict round; new contents every call, and an rbuf freed
# and re-made (a new runtime buffer id, possibly at the same address) takes
# the full exchange again -- every result exact
# ---------------------------------------------------------------------------
def _fast_x(rank, i, count):
    return np.random.default_rng(9000 + 97 * i + rank).integers(-(1 << 31), 1 << 31, count,
                                                                 dtype=np.int64).astype(np.int32)


def _reg_fast_worker(rank, n, port, q):
    import ctypes
    import torch.distributed as dist
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    try:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=n)
        torch.cuda.set_device(0)
        mxompi.init(0)

        def ag(b):
            out = [None] * n
            dist.all_gather_object(out, b)
            return out

        comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=16 << 20)
        comm.set_timeout(30.0)
        comm.set_autotune(False)
        comm.set_reg_min(1)                       # zero-copy at every size
        st = torch.cuda.current_stream().cuda_stream
        count = 1 << 20
        X = torch.empty(count, dtype=torch.int32, device="cuda")
        Y = torch.zeros(count, dtype=torch.int32, device="cuda")
        res, diag = [], []
        for i in range(8):
            X.copy_(torch.from_numpy(_fast_x(rank, i, count)).cuda())   # new contents on the stream
            comm.allreduce(X.data_ptr(), Y.data_ptr(), count, "INT32_T", "SUM", "auto", st)
            res.append(Y.cpu().numpy().tobytes())
        diag.append({"x": X.data_ptr(), "y": Y.data_ptr()})
        s1 = comm.stats()
        L = mxompi.lib()
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        for i in range(8, 11):                    # rbuf re-made every call: full exchanges
            p = vp()
            assert L.mx_alloc(sz(4 * count), ctypes.byref(p)) == 0
            X.copy_(torch.from_numpy(_fast_x(rank, i, count)).cuda())
            torch.cuda.synchronize()
            before = comm.stats()
            comm.allreduce(X.data_ptr(), p.value, count, "INT32_T", "SUM", "auto", st)
            after = comm.stats()
            # where each rank's rbuf was, and which path the call took (kept
            # for the failure message: a wrong block names the peer that wrote it)
            diag.append({"i": i, "rbuf": p.value, **{k: after[k] - before[k] for k in
                                                    ("zero_copy_calls", "direct_calls", "staged_calls",
                                                     "reg_fast_calls")}})
            host = np.empty(count, np.int32)
            assert L.mx_memcpy(vp(host.ctypes.data), p, sz(4 * count), None) == 0
            res.append(host.tobytes())
            torch.cuda.synchronize()
            assert L.mx_free(p) == 0
        s2 = comm.stats()
        comm.close()
        dist.destroy_process_group()
        q.put((rank, "ok", {"res": res, "diag": diag, "fast1": s1["reg_fast_calls"], "zc1": s1["zero_copy_calls"],
                            "fast2": s2["reg_fast_calls"], "zc2": s2["zero_copy_calls"],
                            "refused": s2["reg_stale_refused"]}))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc()))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_registration_fast_path_reused_and_remade_buffers(n):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reg_fast_worker, args=(r, n, port, q)) for r in range(n)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(n):
            rank, status, payload = q.get(timeout=240)
            assert status == "ok", payload
            out[rank] = payload
    finally:
        for p in procs:
            p.join(timeout=60 if len(out) == n else 5)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    count = 1 << 20
    for i in range(11):
        exp = sum(_fast_x(r, i, count).astype(np.int64) for r in range(n)).astype(np.int32).tobytes()
        for r in range(n):
            if out[r]["res"][i] != exp:
                # which peers' parts are wrong (zero-copy direct: peer j stores
                # part j into every rank's rbuf), how, and where every rank's
                # buffers were
                got = np.frombuffer(out[r]["res"][i], np.int32)
                want = np.frombuffer(exp, np.int32)
                base, rem = divmod(count, n)
                parts, lo = [], 0
                for j in range(n):
                    hi = lo + base + (1 if j < rem else 0)
                    bad = np.nonzero(got[lo:hi] != want[lo:hi])[0]
                    parts.append((j, len(bad), int(bad[0]) if len(bad) else -1,
                                  int(np.count_nonzero(got[lo:hi][bad] == 0))))
                    lo = hi
                raise AssertionError(f"iteration {i} rank {r}: (part, wrong, first, zeros) {parts}; "
                                     f"diag {[out[k]['diag'] for k in range(n)]}")
    for r in range(n):
        assert out[r]["zc1"] == 8 and out[r]["fast1"] == 7, out[r]      # the first call registers
        # an rbuf re-made at a freed one's address is not exported (DESIGN 7.5:
        # a peer's import of it can reach the freed memory): those calls run
        # staged; the first re-made rbuf is zero-copy only if its address is new
        assert 8 <= out[r]["zc2"] <= 9, out[r]
        assert out[r]["fast2"] == 7, out[r]                             # re-made rbufs: never the fast path
