"""GPU: rooted reductions between processes at every root, and libnbc's orders
past four ranks, bit for bit against the oracle.

n = 3, 5, 8 processes share the one GPU (one spawn per n).  In a
multi-process rooted reduce the part owners run a program that carries both
MPI_IN_PLACE variants of the root's combination, guarded by a bit they read
from the root's READY word; tests/test_rooted_roots_host.py shows that on these
operands the oracle's result changes by at least 50 of 1031 elements with the
bit and with the root, so a launch path that read another rank's word, or
folded for another root, fails here.

  * blocking reduce: linear, chain, pipeline, binary, binomial, in-order binary,
    every root, in place at the root and not, (MAXLOC, FLOAT_INT) at 1 and 1031
    elements and (MAX, FLOAT) at 1031; chain and binomial again on the
    zero-copy path (registered user buffers, counted from zero_copy_calls) at
    the smallest count the communicator's reg_min admits; one chunked call
    (pipeline, root n // 2, in place): each chunk carries the bit anew;
  * blocking reduce_scatter, (MINLOC, DOUBLE_INT), ragged counts with an empty
    block, in place and not, recursive halving, ring and butterfly: in place,
    the ranks whose block is not the first fold into a spare staging slot and
    copy it back, and the padding bytes must still be the buffer's own;
  * ireduce chain, binomial, Rabenseifner (and below pof2(n) elements, where
    it falls back to the chain): every root, in place and not; a persistent
    chain reduce, root n // 2, in place, started twice on fresh data;
  * n = 5, 8 only -- the orders the suite ran at 2..4 ranks only: iallreduce
    binomial, ring, Rabenseifner, recursive doubling at 1031 and n - 1 elements
    (empty ring segments); ireduce_scatter with ragged counts and an empty
    block, ireduce_scatter_block; iscan and iexscan, both algorithms.

Receive buffers are pre-filled with 0xA5 between 64-byte guards: guards,
padding bytes and a non-root's receive buffer must come back untouched.  The
non-blocking calls of a group are all posted before the first wait.
"""
import os
from collections import namedtuple

import numpy as np
import pytest

import golden_io
import mxompi
import op_values as ov
import rooted_roots_util as U
from test_coll_gpu import _free_port

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL, GUARD = ov.PREFILL, 64
STAGING = 1 << 20
COUNT = U.COUNT
CHUNKED = 100003            # floats: more than one chunk of a 1 MiB staging (asserted from fold_launches)
MAXF, MAXLOC = ("MAX", "FLOAT"), ("MAXLOC", "FLOAT_INT")

# kind: reduce | reduce_scatter | ireduce | preduce | iallreduce | ireduce_scatter | ireduce_scatter_block | iscan | iexscan,
# or a control step: reg_min (count = bytes) | zc_calls | prof (count = on) | folds
Job = namedtuple("Job", "kind alg op t count root inplace base", defaults=("auto", "SUM", "FLOAT", 0, 0, False, 0))


def _pof2(n):
    return 1 << (n.bit_length() - 1)


def _rcounts(n, count):
    rc = [count + 3 * p for p in range(n)]
    rc[1] = 0
    return rc


def _groups(n):
    """The calls of the n-process spawn, in groups: the non-blocking calls of a
    group are posted before any is waited for."""
    G = [[Job("reg_min", count=0)]]
    for root in range(n):
        for inplace in (False, True):
            G.append([Job("reduce", alg, op, t, c, root, inplace) for alg in U.REDUCE_ALGS
                      for (op, t), c in ((MAXLOC, 1), (MAXLOC, COUNT), (MAXF, COUNT))])
    # zero-copy: exactly at reg_min
    es = mxompi.type_size(MAXLOC[1])
    G.append([Job("reg_min", count=COUNT * es), Job("zc_calls")])
    for root in range(n):
        G.append([Job("reduce", alg, *MAXLOC, COUNT, root, inplace) for alg in ("chain", "binomial")
                  for inplace in (False, True)])
    G.append([Job("zc_calls"), Job("reg_min", count=0)])
    # chunked: every chunk's READY word carries the bit
    G.append([Job("prof", count=1), Job("folds"), Job("reduce", "pipeline", *MAXF, CHUNKED, n // 2, True),
              Job("folds"), Job("prof", count=0)])
    # blocking reduce_scatter of a padded type: in place, a block that starts inside the range its
    # result overwrites is folded into a spare staging slot and copied back -- padding and all
    G.append([Job("reduce_scatter", alg, "MINLOC", "DOUBLE_INT", 37, inplace=ip)
              for alg in ("recursive_halving", "ring", "butterfly") for ip in (False, True)])
    for root in range(n):
        G.append([Job("ireduce", alg, op, t, c, root, inplace)
                  for alg, c in (("chain", COUNT), ("binomial", COUNT), ("rabenseifner", COUNT),
                                 ("rabenseifner", _pof2(n) - 1))
                  for op, t in (MAXLOC, MAXF) for inplace in (False, True)])
    G.append([Job("preduce", "chain", *MAXLOC, COUNT, n // 2, True)])
    if n > 4:
        g = []
        for alg in ("binomial", "ring", "rabenseifner", "recursive_doubling"):
            g += [Job("iallreduce", alg, op, "FLOAT", c) for op in ("SUM", "MAX") for c in (COUNT, n - 1)]
            g.append(Job("iallreduce", alg, "MAX", "FLOAT", COUNT, inplace=True))
        G.append(g)
        G.append([Job(kind, "auto", op, t, 37, inplace=ip) for kind in ("ireduce_scatter", "ireduce_scatter_block")
                  for op, t in (("SUM", "DOUBLE"), ("MINLOC", "DOUBLE_INT")) for ip in (False, True)] +
                 [Job(kind, alg, "SUM", "FLOAT", COUNT) for kind in ("iscan", "iexscan")
                  for alg in ("linear", "recursive_doubling")])
    return G


def _scount(job, n):
    """elements of a rank's send side"""
    if job.kind in ("reduce_scatter", "ireduce_scatter"):
        return sum(_rcounts(n, job.count))
    return job.count * n if job.kind == "ireduce_scatter_block" else job.count


def _rcount(job, n, rank):
    return _rcounts(n, job.count)[rank] if job.kind in ("reduce_scatter", "ireduce_scatter") else job.count


class _Buf:
    """nbytes on the device between guards, pre-filled with 0xA5 or holding `data`"""

    def __init__(self, nbytes, data=None):
        self.nbytes = nbytes
        self.t = torch.from_numpy(_image(nbytes, data)).to("cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + GUARD

    def refill(self, data):
        self.t.copy_(torch.from_numpy(_image(self.nbytes, data)))

    def image(self):
        return self.t.cpu().numpy().tobytes()


def _image(nbytes, data=None):
    host = np.full(GUARD + nbytes + GUARD, FILL, np.uint8)
    if data is not None:
        host[GUARD:GUARD + nbytes] = data
    return host


def _post(comm, rank, n, job, st):
    """Start one call; returns (request or None, send buffer, receive buffer, writes here)."""
    es = mxompi.type_size(job.t)
    x = ov.inputs(job.op, job.t, n, _scount(job, n), job.base)[rank]
    rooted = job.kind in ("reduce", "ireduce", "preduce")
    in_place_here = job.inplace and (not rooted or rank == job.root)
    if in_place_here:
        S, R = None, _Buf(len(x), x)
    else:
        S, R = _Buf(len(x), x), _Buf(_rcount(job, n, rank) * es)
    sp = mxompi.IN_PLACE if in_place_here else S.ptr
    a = (sp, R.ptr, job.count, job.t, job.op)
    if job.kind == "reduce":
        comm.reduce(*a, job.root, job.alg, st)
        req = None
    elif job.kind in ("ireduce", "preduce"):
        req = comm.ireduce(*a, job.root, job.alg, st, persistent=job.kind == "preduce")
    elif job.kind == "reduce_scatter":
        comm.reduce_scatter(sp, R.ptr, _rcounts(n, job.count), job.t, job.op, job.alg, st)
        req = None
    elif job.kind == "ireduce_scatter":
        req = comm.ireduce_scatter(sp, R.ptr, _rcounts(n, job.count), job.t, job.op, st)
    elif job.kind == "ireduce_scatter_block":
        req = comm.ireduce_scatter_block(*a, st)
    else:
        req = getattr(comm, job.kind)(*a, job.alg, st)
    writes = not rooted or rank == job.root
    if job.kind == "iexscan" and rank == 0:
        writes = False
    return req, S, R, writes


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

        comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=STAGING)
        comm.set_timeout(30.0)
        st = torch.cuda.current_stream().cuda_stream
        results, keep = [], []
        for group in _groups(n):
            posted = []
            for job in group:
                if job.kind == "reg_min":
                    comm.set_reg_min(job.count)
                    posted.append(None)
                elif job.kind == "prof":
                    comm.set_profiling(bool(job.count))
                    posted.append(None)
                elif job.kind in ("zc_calls", "folds"):
                    posted.append(comm.stats()["zero_copy_calls" if job.kind == "zc_calls" else "fold_launches"])
                elif job.kind == "preduce":
                    # one persistent request, started twice on fresh data
                    req, S, R, writes = _post(comm, rank, n, job, st)
                    assert not req.active and req.test()
                    reps = []
                    for rep in range(2):
                        x = ov.inputs(job.op, job.t, n, job.count, 100 * rep)[rank]
                        (R if S is None else S).refill(x)
                        if S is not None:
                            R.refill(None)
                        req.start()
                        req.wait()
                        reps.append(R.image() if writes else bool((R.t == FILL).all()))
                    req.free()
                    posted.append(reps)
                else:
                    posted.append(_post(comm, rank, n, job, st))
            for p in posted:
                if not isinstance(p, tuple):
                    results.append(p)
                    continue
                req, S, R, writes = p
                if req is not None:
                    req.wait()
                    req.free()
                # a buffer this rank's call must not write: still the fill, checked here
                results.append(R.image() if writes else bool((R.t == FILL).all()))
                keep.append((S, R))          # registered buffers stay allocated while zero-copy calls follow
        comm.close()
        dist.destroy_process_group()
        q.put((rank, "ok", results))
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


def _pad_mask(t, count):
    slot = mxompi.TYPE[t]
    if slot not in golden_io._DATA_BYTES:
        return None
    es, keep = golden_io._DATA_BYTES[slot]
    m = np.ones(es, bool)
    m[keep] = False
    return np.tile(m, count)


def _check_image(img, count, exp, op, t, what, before=None):
    """Guards untouched; the first `count` elements the oracle's, their padding
    bytes as they were (`before`: the buffer's bytes before an in-place call).
    An in-place reduce_scatter, ireduce_scatter or ireduce_scatter_block hands
    in the whole send vector: what follows its first `count` elements is not
    compared with anything -- MPI leaves it undefined after the call."""
    host = np.frombuffer(img, np.uint8)
    nb = count * mxompi.type_size(t)
    size = len(host) - 2 * GUARD
    assert (host[:GUARD] == FILL).all() and (host[GUARD + size:] == FILL).all(), f"{what}: guard written"
    got = host[GUARD:GUARD + nb]
    golden_io.assert_coll_equal(got, exp[:nb], mxompi.OP[op], mxompi.TYPE[t], what)
    mask = _pad_mask(t, count)
    if mask is not None:
        ref = np.full(nb, FILL, np.uint8) if before is None else before[:nb]
        np.testing.assert_array_equal(got[mask], ref[mask], err_msg=f"{what}: padding bytes written")
    if before is None:
        assert size == nb, f"{what}: buffer of {size} bytes for {nb}"


def _expected(job, n):
    """The oracle's result per rank (None: the rank's buffer stays as it was)."""
    L = U.oracle()
    vp, sz = U.vp, U.sz
    o, ty, es = mxompi.OP[job.op], mxompi.TYPE[job.t], mxompi.type_size(job.t)
    xs = ov.inputs(job.op, job.t, n, _scount(job, n), job.base)
    if job.kind in ("reduce", "ireduce", "preduce"):
        exp = U.rooted("reduce" if job.kind == "reduce" else "ireduce", job.alg, n, job.count, job.op, job.t, job.root,
                       job.inplace, job.base)
        return [exp if r == job.root else None for r in range(n)]
    rc = [_rcount(job, n, r) for r in range(n)]
    out = [x.copy() if job.inplace else np.full(rc[r] * es, FILL, np.uint8) for r, x in enumerate(xs)]
    sp = None if job.inplace else (vp * n)(*[x.ctypes.data for x in xs])
    rp = (vp * n)(*[e.ctypes.data for e in out])
    if job.kind == "iallreduce":
        assert L.mxo_iallreduce(mxompi.IALLREDUCE[job.alg], o, ty, n, job.count, sp, rp) == 0
    elif job.kind == "reduce_scatter":
        assert L.mxo_reduce_scatter(mxompi.REDUCE_SCATTER[job.alg], o, ty, n, (sz * n)(*rc), sp, rp) == 0
    elif job.kind in ("ireduce_scatter", "ireduce_scatter_block"):
        assert L.mxo_ireduce_scatter(o, ty, n, (sz * n)(*rc), sp, rp) == 0
    else:
        fn = L.mxo_scan if job.kind == "iscan" else L.mxo_exscan
        assert fn(mxompi.SCAN[job.alg], o, ty, n, job.count, sp, rp) == 0
    if job.kind == "iexscan":
        out[0] = None
    return out


@pytest.mark.parametrize("n", U.NS)
def test_every_root_and_libnbc_orders_bitexact(n):
    got = _run(n)
    jobs = [j for g in _groups(n) for j in g]
    for r in range(n):
        assert len(got[r]) == len(jobs)
    zc, folds = [], []
    for i, job in enumerate(jobs):
        if job.kind in ("reg_min", "prof"):
            continue
        if job.kind in ("zc_calls", "folds"):
            (zc if job.kind == "zc_calls" else folds).append([got[r][i] for r in range(n)])
            continue
        what = f"{job.kind} {job.alg} {job.op} {job.t} count {job.count} root {job.root} in place {job.inplace} n={n}"
        starts = (0, 100) if job.kind == "preduce" else (job.base,)
        for k, base in enumerate(starts):
            jb = job._replace(base=base)
            exp = _expected(jb, n)
            xs = ov.inputs(job.op, job.t, n, _scount(job, n), base)
            for r in range(n):
                res = got[r][i][k] if job.kind == "preduce" else got[r][i]
                if exp[r] is None:
                    assert res is True, f"{what}: rank {r}'s receive buffer was written"
                else:
                    in_place_here = job.inplace and (r == job.root or job.kind not in ("reduce", "ireduce", "preduce"))
                    _check_image(res, _rcount(job, n, r), exp[r], job.op, job.t, f"{what} start {k} rank {r}",
                                 before=xs[r] if in_place_here else None)
    # the zero-copy block: every call of it, on every rank, went between registered buffers
    assert len(zc) == 2 and [b - a for a, b in zip(*zc)] == [2 * 2 * n] * n, zc     # chain, binomial x in place or not x roots
    # the chunked call took at least two chunks on every rank
    assert len(folds) == 2 and all(b - a >= 2 for a, b in zip(*folds)), folds
