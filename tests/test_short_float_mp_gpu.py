"""GPU, two and three processes sharing the GPU: the binary16 slots through
the multi-process data paths.

* MPI_Allreduce SUM on SHORT_FLOAT at 5 elements (one-shot),
  40,003 (staged, the pull protocol forced as tests/test_coll_gpu.py's path
  switch does) and 300,001 (above the 256 KiB zero-copy threshold); the
  per-call counters tell which path ran.  Expected values: the collective
  oracle's symbolic trees for the algorithm AUTO decides (the decision is
  UINT16_T's), evaluated in numpy float16 (tests/short_float.py).
* a 13-element complex PROD allreduce: 4-byte elements are served by the
  small-allreduce service with two ranks (launched with three); the 2-byte
  real type is declined to the launch;
* one mx_accumulate SUM and two mx_fetch_and_op MAX on the symmetric heap
  (a NaN source comes through bit for bit: compare and select).

Every device wait is bounded by the communicator's 30 s timeout and every
queue read by its own, as in the existing workers."""
import os

import numpy as np
import pytest

import mxompi
import short_float as sf
from test_coll_gpu import _free_port
from test_short_float_coll_gpu import sym

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

T = "SHORT_FLOAT"
COUNTS = [(5, "default"), (40003, "pull"), (300001, "zero_copy")]
N_ACC = 4099
N_SVC = 13


def _x(rank, count):
    return sf.gen_spread(count, 7000 + rank + count)


def _worker(rank, n, port, q):
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

        def dev(u16):
            return torch.from_numpy(np.ascontiguousarray(u16).view(np.uint8).copy()).to("cuda")

        comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=64 << 20, heap_bytes=64 << 20)
        comm.set_timeout(30.0)
        st = torch.cuda.current_stream().cuda_stream
        res = {"allreduce": [], "paths": []}
        # the small-allreduce service: 4-byte elements travel as tagged words
        # and are served (two ranks per device), 2-byte elements are declined
        x = dev(sf.gen_unit(N_SVC, 7100 + rank))
        out = torch.zeros(4 * N_SVC, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        comm.stats(reset=True)
        comm.allreduce(x.data_ptr(), out.data_ptr(), N_SVC, "C_SHORT_FLOAT_COMPLEX", "PROD", "auto", st)
        res["svc_cplx"] = (out.cpu().numpy().tobytes(), comm.stats()["service_calls"])
        for count, path in COUNTS:
            if path != "default":
                comm.set_autotune(False)
                comm.set_oneshot_max(0 if path == "pull" else 128 << 10)
                comm.set_reg_min(0 if path == "pull" else 256 << 10)
                comm.set_protocol("pull" if path == "pull" else "auto")
            x = dev(_x(rank, count))
            out = torch.zeros(2 * count, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            comm.stats(reset=True)
            comm.allreduce(x.data_ptr(), out.data_ptr(), count, T, "SUM", "auto", st)
            torch.cuda.synchronize()
            s = comm.stats()
            res["allreduce"].append(out.cpu().numpy().tobytes())
            res["paths"].append((s["zero_copy_calls"], s["staged_calls"], s["service_calls"]))

        heap = mxompi.Heap(comm, 8 << 20)

        def to_heap(addr, u16):
            t = dev(u16)
            torch.cuda.synchronize()
            mxompi.lib().mx_copy(addr, t.data_ptr(), t.numel(), None)
            mxompi.sync()

        def from_heap(addr, nbytes):
            t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            mxompi.lib().mx_copy(t.data_ptr(), addr, nbytes, None)
            mxompi.sync()
            return t.cpu().numpy().tobytes()

        # accumulate SUM: rank 0's origin into PE n-1's window
        win = heap.alloc(2 * N_ACC)
        to_heap(win, sf.gen("SUM", T, N_ACC, 500 + rank))
        heap.barrier_all()
        if rank == 0:
            o = dev(sf.gen("SUM", T, N_ACC, 900))
            heap.accumulate(o.data_ptr(), N_ACC, T, "SUM", n - 1, win)
        heap.barrier_all()
        if rank == n - 1:
            res["acc"] = from_heap(win, 2 * N_ACC)
        # fetch_and_op MAX on PE 0's word: 1.5 <- 2.5 by rank 1, then <- NaN (payload 1) by rank 0
        word = heap.alloc(16)
        to_heap(word, np.array([0x3E00] * 8, np.uint16))
        heap.barrier_all()
        got = torch.zeros(2, dtype=torch.uint8, device="cuda")
        if rank == 1:
            heap.fetch_and_op(dev(np.array([0x4100], np.uint16)).data_ptr(), got.data_ptr(), T, "MAX", 0, word)
            res["fop1"] = got.cpu().numpy().tobytes()
        heap.barrier_all()
        if rank == 0:
            res["after1"] = from_heap(word, 4)
            heap.fetch_and_op(dev(np.array([0x7E01], np.uint16)).data_ptr(), got.data_ptr(), T, "MAX", 0, word)
            res["fop2"] = got.cpu().numpy().tobytes()
            res["after2"] = from_heap(word, 4)
        heap.barrier_all()
        heap.free(word)
        heap.free(win)
        heap.close()
        comm.close()
        dist.destroy_process_group()
        q.put((rank, "ok", res))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc() + str(e)))


def _run(n):
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
            rank, status, payload = q.get(timeout=120)
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
def test_allreduce_and_one_sided(n):
    got = _run(n)
    for j, (count, path) in enumerate(COUNTS):
        alg = mxompi.allreduce_decision(n, count, T)
        assert alg == mxompi.allreduce_decision(n, count, "UINT16_T")
        # (orders that do not depend on the element size)
        assert alg in (mxompi.ALLREDUCE["recursive_doubling"], mxompi.ALLREDUCE["ring"])
        exp = sym("allreduce", alg, n, count).evaluate("SUM", T, [_x(r, count) for r in range(n)])
        for r in range(n):
            sf.assert_equal("SUM", np.frombuffer(got[r]["allreduce"][j], np.uint16), exp[r][0].ravel(),
                            f"allreduce n={n} count={count} rank {r}")
            # (zero-copy, staged, served) calls; default: one-shot, the 2-byte type is not served
            want = {"pull": (0, 1, 0), "zero_copy": (1, 0, 0), "default": (0, 0, 0)}[path]
            assert got[r]["paths"][j] == want, (r, got[r]["paths"])
    # complex PROD, 13 elements: served by the small-allreduce service with two ranks, launched with three
    alg = mxompi.allreduce_decision(n, N_SVC, "C_SHORT_FLOAT_COMPLEX")
    assert alg == mxompi.ALLREDUCE["recursive_doubling"]
    exp = sym("allreduce", alg, n, N_SVC).evaluate("PROD", "C_SHORT_FLOAT_COMPLEX",
                                                   [sf.gen_unit(N_SVC, 7100 + r) for r in range(n)])
    for r in range(n):
        sf.assert_equal("PROD", np.frombuffer(got[r]["svc_cplx"][0], np.uint16), exp[r][0].ravel(),
                        f"complex PROD allreduce n={n} rank {r}")
        assert got[r]["svc_cplx"][1] == (1 if n == 2 else 0), (r, got[r]["svc_cplx"][1])
    # accumulate: target = target SUM origin (x = target, y = origin)
    exp = sf.ref("SUM", T, sf.gen("SUM", T, N_ACC, 500 + n - 1), sf.gen("SUM", T, N_ACC, 900))
    sf.assert_equal("SUM", np.frombuffer(got[n - 1]["acc"], np.uint16), exp, "accumulate")
    # fetch_and_op: the old value comes back; MAX is (target > source) ? target : source
    assert np.frombuffer(got[1]["fop1"], np.uint16)[0] == 0x3E00
    assert list(np.frombuffer(got[0]["after1"], np.uint16)) == [0x4100, 0x3E00]
    assert np.frombuffer(got[0]["fop2"], np.uint16)[0] == 0x4100
    assert list(np.frombuffer(got[0]["after2"], np.uint16)) == [0x7E01, 0x3E00]
