"""GPU: alltoall, alltoallv and allgatherv on the exchange kernel
(csrc/mx_exchange.hip).  Pure data movement: expected bytes come from numpy
on seeded inputs.  Local communicators drive the kernel through every pair of
byte alignments, the sizes where its paths change and ragged tables;
multi-process communicators (ranks as processes on the one GPU) run the
staged and the zero-copy data paths."""
import os
import socket

import numpy as np
import pytest

import mxompi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ready():
    mxompi.init(0)
    return True


def _alltoallv_local(n, sbytes, soffs, rbytes, roffs, slen, rlen, seed, inplace=False):
    """One alltoallv_local call on fresh buffers; checks EVERY byte of every
    receive buffer: the ranges against numpy, the rest still the fill (in
    place: still what it was).  Matrices are [owner][peer]; slen / rlen: bytes
    per send / receive buffer."""
    rng = np.random.default_rng(seed)
    comm = mxompi.Comm.local(n)
    try:
        if inplace:
            old = [rng.integers(0, 256, rlen, dtype=np.uint8) for _ in range(n)]
            exp = [o.copy() for o in old]
            for i in range(n):
                for j in range(n):
                    ln = min(rbytes[i][j], rbytes[j][i])
                    exp[j][roffs[j][i]:roffs[j][i] + ln] = old[i][roffs[i][j]:roffs[i][j] + ln]
            R = [_dev(o) for o in old]
            sp = None
        else:
            src = [rng.integers(0, 256, slen, dtype=np.uint8) for _ in range(n)]
            exp = [np.full(rlen, FILL, dtype=np.uint8) for _ in range(n)]
            for i in range(n):
                for j in range(n):
                    ln = min(sbytes[i][j], rbytes[j][i])
                    exp[j][roffs[j][i]:roffs[j][i] + ln] = src[i][soffs[i][j]:soffs[i][j] + ln]
            S = [_dev(s) for s in src]
            R = [_dev(np.full(rlen, FILL, dtype=np.uint8)) for _ in range(n)]
            assert all(t.data_ptr() % 16 == 0 for t in S + R)
            sp = [t.data_ptr() for t in S]
        flat = lambda m: [v for row in m for v in row]   # noqa: E731
        comm.alltoallv_local(sp, None if inplace else flat(sbytes), None if inplace else flat(soffs),
                             [t.data_ptr() for t in R], flat(rbytes), flat(roffs), _stream())
        torch.cuda.synchronize()
        for j in range(n):
            got = R[j].cpu().numpy()
            bad = np.nonzero(got != exp[j])[0]
            assert bad.size == 0, (f"rank {j}: {bad.size} wrong bytes, first at {bad[0]} "
                                   f"(got {got[bad[0]]:#x}, expected {exp[j][bad[0]]:#x})")
    finally:
        comm.close()


# -- 1. every pair of byte alignments ------------------------------------------
@pytest.mark.parametrize("size", [0, 1, 15, 16, 17, 31, 33, 64, 65, 257])
def test_alignment_matrix(ready, size):
    """n = 16: pair (i, j) reads at an address = i and writes at an address
    = j (mod 16), so one call holds all 256 alignment pairs."""
    n = 16
    stride = (size + 15) // 16 * 16 + 32
    sb = [[size] * n for _ in range(n)]
    so = [[j * stride + i for j in range(n)] for i in range(n)]        # rank i's block for j
    ro = [[i * stride + j for i in range(n)] for j in range(n)]        # rank j's block from i
    _alltoallv_local(n, sb, so, sb, ro, n * stride + 32, n * stride + 32, seed=100 + size)


# -- 2. one byte below, at and above a workgroup's and a wave's share ----------
@pytest.mark.parametrize("unit", ["workgroup", "wave"])
def test_block_boundaries(ready, unit):
    block, wave = mxompi.exchange_geometry()
    base = block if unit == "workgroup" else wave
    n = 2
    for size in (base - 1, base, base + 1):
        for ms, md in ((0, 0), (0, 5), (4, 0), (3, 9), (15, 15)):
            stride = (size + 15) // 16 * 16 + 48
            sb = [[size] * n for _ in range(n)]
            so = [[j * stride + ms for j in range(n)] for _ in range(n)]
            ro = [[i * stride + md for i in range(n)] for _ in range(n)]
            _alltoallv_local(n, sb, so, sb, ro, n * stride + 32, n * stride + 32, seed=size * 31 + ms * 16 + md)


# -- 3. ragged tables -----------------------------------------------------------
def _ragged(n, seed, big):
    rng = np.random.default_rng(seed)
    sb = rng.integers(0, 5000, (n, n)).tolist()
    sb[n - 1] = [0] * n                          # a rank that sends nothing
    sb[0][n - 1] = big                           # one pair far larger than the rest
    sb[1][0] = 0
    rb = [[sb[i][j] for i in range(n)] for j in range(n)]
    rb[1][0] = max(0, sb[0][1] - 7)              # a receiver with less room than its sender announces
    so, ro, slen, rlen = [], [], 0, 0
    for i in range(n):
        o, row = int(rng.integers(0, 16)), []
        for j in range(n):
            row.append(o)
            o += sb[i][j] + int(rng.integers(0, 40))
        so.append(row)
        slen = max(slen, o + 16)
    for j in range(n):
        o, row = int(rng.integers(0, 16)), []
        for i in range(n):
            row.append(o)
            o += max(rb[j][i], sb[i][j]) + int(rng.integers(0, 40))   # room to see a write past rbytes
        ro.append(row)
        rlen = max(rlen, o + 16)
    return sb, so, rb, ro, slen, rlen


@pytest.mark.parametrize("n", [3, 8])
def test_ragged(ready, n):
    sb, so, rb, ro, slen, rlen = _ragged(n, 4242 + n, (1 << 20) + 3)
    _alltoallv_local(n, sb, so, rb, ro, slen, rlen, seed=n)


@pytest.mark.parametrize("n", [2, 5])
def test_ragged_in_place(ready, n):
    rng = np.random.default_rng(77 + n)
    rb = rng.integers(0, 3000, (n, n)).tolist()
    rb[0][n - 1] = 40000
    rb[n - 1][0] = 39990
    ro, rlen = [], 0
    for j in range(n):
        o, row = int(rng.integers(0, 16)), []
        for i in range(n):
            row.append(o)
            o += rb[j][i] + int(rng.integers(0, 40))
        ro.append(row)
        rlen = max(rlen, o + 16)
    _alltoallv_local(n, None, None, rb, ro, 0, rlen, seed=n, inplace=True)


# -- 4. alltoall_local / allgatherv_local ----------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_alltoall_and_allgatherv_local(ready, n):
    comm = mxompi.Comm.local(n)
    try:
        for size in (1, 13, 4096, 100003):
            rng = np.random.default_rng(size + n)
            # alltoall, out of place then in place
            src = [rng.integers(0, 256, n * size, dtype=np.uint8) for _ in range(n)]
            exp = [np.concatenate([src[i][j * size:(j + 1) * size] for i in range(n)]) for j in range(n)]
            S = [_dev(s) for s in src]
            R = [_dev(np.full(n * size + 16, FILL, dtype=np.uint8)) for _ in range(n)]
            comm.alltoall_local([t.data_ptr() for t in S], [t.data_ptr() for t in R], size, _stream())
            for j in range(n):
                got = R[j].cpu().numpy()
                assert np.array_equal(got[:n * size], exp[j]), f"alltoall n={n} size={size} rank {j}"
                assert (got[n * size:] == FILL).all(), f"alltoall n={n} size={size} rank {j}: wrote past rbuf"
            comm.alltoall_local(None, [t.data_ptr() for t in S], size, _stream())
            for j in range(n):
                assert np.array_equal(S[j].cpu().numpy(), exp[j]), f"alltoall in place n={n} size={size} rank {j}"
            # allgatherv: ragged blocks (one empty) at odd offsets with gaps
            rbytes = [max(0, size - 7 * i) for i in range(n)]
            if n > 2:
                rbytes[1] = 0
            roffs, o = [], 3
            for i in range(n):
                roffs.append(o)
                o += rbytes[i] + 5
            blocks = [rng.integers(0, 256, rbytes[i], dtype=np.uint8) for i in range(n)]
            want = np.full(o + 16, FILL, dtype=np.uint8)
            for i in range(n):
                want[roffs[i]:roffs[i] + rbytes[i]] = blocks[i]
            B = [_dev(np.concatenate([b, np.zeros(1, np.uint8)])) for b in blocks]   # never an empty tensor
            R = [_dev(np.full(o + 16, FILL, dtype=np.uint8)) for _ in range(n)]
            comm.allgatherv_local([t.data_ptr() for t in B], [t.data_ptr() for t in R], rbytes, roffs, _stream())
            for j in range(n):
                assert np.array_equal(R[j].cpu().numpy(), want), f"allgatherv n={n} size={size} rank {j}"
            # in place: every rank holds only its own block
            R = []
            for i in range(n):
                a = np.full(o + 16, FILL, dtype=np.uint8)
                a[roffs[i]:roffs[i] + rbytes[i]] = blocks[i]
                R.append(_dev(a))
            comm.allgatherv_local(None, [t.data_ptr() for t in R], rbytes, roffs, _stream())
            for j in range(n):
                assert np.array_equal(R[j].cpu().numpy(), want), f"allgatherv in place n={n} size={size} rank {j}"
        st = comm.exchange_stats()
        assert st["calls"] == 16 and st["zero_copy_calls"] == 0 and st["staged_calls"] == 0, st
    finally:
        comm.close()


def test_table_memory_goes_back_with_the_communicator(ready):
    """A local communicator of more than 16 jobs takes table memory (pinned
    host + device slots) at its first such launch and gives it back when it
    is destroyed; one of 16 jobs or fewer never takes any."""
    before = mxompi.exchange_tables_live()
    for n, takes in ((8, 1), (4, 0)):
        for _ in range(3):
            comm = mxompi.Comm.local(n)
            S = [_dev(np.arange(n * 64, dtype=np.uint8)) for _ in range(n)]
            R = [_dev(np.zeros(n * 64, dtype=np.uint8)) for _ in range(n)]
            comm.alltoall_local([t.data_ptr() for t in S], [t.data_ptr() for t in R], 64, _stream())
            comm.alltoall_local([t.data_ptr() for t in S], [t.data_ptr() for t in R], 64, _stream())
            assert mxompi.exchange_tables_live() == before + takes
            comm.close()
            assert mxompi.exchange_tables_live() == before


# -- multi-process: ranks as processes on the one GPU ---------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_bytes(job, rank, nbytes):
    return np.random.default_rng(9000 + 131 * job + rank).integers(0, 256, nbytes, dtype=np.uint8)


def _v_tables(n, job, big=0, empty=False):
    """alltoallv tables of every rank, the same in every process: sizes
    [sender][receiver] with zeros, offsets at odd addresses with gaps.
    empty: the last rank sends nothing and rank 0 receives nothing."""
    rng = np.random.default_rng(600 + job * 17 + n)
    sb = rng.integers(0, 3000, (n, n)).tolist()
    sb[0][n - 1] = 0
    sb[n - 1] = [0 if j % 2 else v for j, v in enumerate(sb[n - 1])]
    if big:
        sb[0][1] = big
    if empty:
        sb[n - 1] = [0] * n
        for i in range(n):
            sb[i][0] = 0
        sb[0][n - 1] = 1234
    so, ro = [], []
    for i in range(n):
        o, row = 1 + i, []
        for j in range(n):
            row.append(o)
            o += sb[i][j] + 3 + j
        so.append(row)
    for j in range(n):
        o, row = 2 + j, []
        for i in range(n):
            row.append(o)
            o += sb[i][j] + 1 + i
        ro.append(row)
    slen = max(so[i][n - 1] + sb[i][n - 1] for i in range(n)) + 32
    rlen = max(ro[j][n - 1] + sb[n - 1][j] for j in range(n)) + 32
    return sb, so, ro, slen, rlen


def _mp_job(comm, rank, n, idx, kind, arg, st):
    """Runs one exchange; returns (error text or None, largest pair)."""
    if kind in ("alltoall", "alltoall_inplace"):
        size = arg
        src = [_rank_bytes(idx, r, n * size) for r in range(n)]
        exp = np.concatenate([src[i][rank * size:(rank + 1) * size] for i in range(n)])
        if kind == "alltoall":
            S = _dev(src[rank])
            R = _dev(np.full(n * size + 16, FILL, dtype=np.uint8))
            comm.alltoall(S.data_ptr(), R.data_ptr(), size, st)
        else:
            R = _dev(np.concatenate([src[rank], np.full(16, FILL, dtype=np.uint8)]))
            comm.alltoall(mxompi.IN_PLACE, R.data_ptr(), size, st)
        got = R.cpu().numpy()
        ok = np.array_equal(got[:n * size], exp) and (got[n * size:] == FILL).all()
        return (None if ok else f"{kind} {size}: wrong bytes"), size
    if kind in ("alltoallv", "alltoallv_big", "alltoallv_empty"):
        sb, so, ro, slen, rlen = _v_tables(n, idx, big=arg, empty=kind == "alltoallv_empty")
        src = [_rank_bytes(idx, r, slen) for r in range(n)]
        exp = np.full(rlen, FILL, dtype=np.uint8)
        for i in range(n):
            exp[ro[rank][i]:ro[rank][i] + sb[i][rank]] = src[i][so[i][rank]:so[i][rank] + sb[i][rank]]
        S = _dev(src[rank])
        R = _dev(np.full(rlen, FILL, dtype=np.uint8))
        # a rank with nothing to send (receive) passes no send (receive) buffer at all
        sp = S.data_ptr() if kind != "alltoallv_empty" or any(sb[rank]) else None
        rp = R.data_ptr() if kind != "alltoallv_empty" or any(sb[i][rank] for i in range(n)) else None
        comm.alltoallv(sp, sb[rank], so[rank], rp, [sb[i][rank] for i in range(n)], ro[rank], st)
        ok = np.array_equal(R.cpu().numpy(), exp)
        return (None if ok else f"{kind}: wrong bytes"), max(max(row) for row in sb)
    if kind == "alltoallv_inplace":
        rng = np.random.default_rng(40 + idx)
        m = rng.integers(0, 2000, (n, n))
        m = np.minimum(m, m.T).tolist()        # in place both sides of a pair use one size
        ro = []
        for j in range(n):
            o, row = 5 + j, []
            for i in range(n):
                row.append(o)
                o += m[j][i] + 2 + i
            ro.append(row)
        rlen = max(ro[j][n - 1] + m[j][n - 1] for j in range(n)) + 32
        old = [_rank_bytes(idx, r, rlen) for r in range(n)]
        exp = old[rank].copy()
        for i in range(n):
            exp[ro[rank][i]:ro[rank][i] + m[rank][i]] = old[i][ro[i][rank]:ro[i][rank] + m[i][rank]]
        R = _dev(old[rank])
        comm.alltoallv(mxompi.IN_PLACE, None, None, R.data_ptr(), m[rank], ro[rank], st)
        ok = np.array_equal(R.cpu().numpy(), exp)
        return (None if ok else "alltoallv in place: wrong bytes"), max(max(row) for row in m)
    if kind in ("allgatherv", "allgatherv_inplace"):
        rng = np.random.default_rng(70 + idx + n)
        rbytes = rng.integers(1, 4000, n).tolist()
        rbytes[n - 1] = 0
        rbytes[0] = arg
        roffs, o = [], 3
        for i in range(n):
            roffs.append(o)
            o += rbytes[i] + 5 + i
        blocks = [_rank_bytes(idx, r, rbytes[r] + 1)[:rbytes[r]] for r in range(n)]
        exp = np.full(o + 16, FILL, dtype=np.uint8)
        for i in range(n):
            exp[roffs[i]:roffs[i] + rbytes[i]] = blocks[i]
        if kind == "allgatherv":
            S = _dev(np.concatenate([np.zeros(1, np.uint8), blocks[rank], np.zeros(1, np.uint8)]))
            R = _dev(np.full(o + 16, FILL, dtype=np.uint8))
            comm.allgatherv(S.data_ptr() + 1, rbytes[rank], R.data_ptr(), rbytes, roffs, st)   # an odd source address
        else:
            a = np.full(o + 16, FILL, dtype=np.uint8)
            a[roffs[rank]:roffs[rank] + rbytes[rank]] = blocks[rank]
            R = _dev(a)
            comm.allgatherv(mxompi.IN_PLACE, 0, R.data_ptr(), rbytes, roffs, st)
        ok = np.array_equal(R.cpu().numpy(), exp)
        return (None if ok else f"{kind}: wrong bytes"), max(rbytes)
    raise ValueError(kind)


_MP_JOBS = [("alltoall", 13), ("alltoall", 4096 + 4), ("alltoall_inplace", 1000), ("alltoallv", 0),
            ("alltoallv_inplace", 0), ("allgatherv", 2500), ("allgatherv_inplace", 777),
            ("alltoallv_empty", 0), ("alltoallv_big", 100 << 10)]
_STAGING = 256 << 10


def _mp_worker(rank, n, port, q):
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

        comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=_STAGING)
        comm.set_timeout(30.0)
        st = torch.cuda.current_stream().cuda_stream
        errs = []
        for reg_min in (0, 1):            # staged, then zero-copy from one byte
            comm.set_reg_min(reg_min)
            for idx, (kind, arg) in enumerate(_MP_JOBS):
                before = comm.exchange_stats()
                err, max_pair = _mp_job(comm, rank, n, idx, kind, arg, st)
                after = comm.exchange_stats()
                d = {k: after[k] - before[k] for k in after}
                what = f"rank {rank} reg_min {reg_min} job {idx} {kind}"
                if err:
                    errs.append(f"{what}: {err}")
                if d["calls"] != 1:
                    errs.append(f"{what}: {d['calls']} calls counted")
                planned = comm.exchange_rounds(max_pair)
                # pairs of a few KiB fit any slot of this staging split 8 ways: one round
                if kind != "alltoallv_big" and planned != 1:
                    errs.append(f"{what}: {planned} rounds planned for a {max_pair}-byte pair")
                if kind == "alltoallv_big" and not (planned > 1 and planned >= -(-max_pair * n // _STAGING)):
                    errs.append(f"{what}: {planned} rounds planned for a {max_pair}-byte pair")
                if reg_min == 0 or kind.endswith("_inplace"):     # staged, exactly as planned
                    if (d["zero_copy_calls"], d["staged_calls"], d["staged_rounds"]) != (0, 1, planned):
                        errs.append(f"{what}: stats {d}, planned {planned} rounds")
                else:   # zero-copy, or staged where the registration was refused (re-made allocations)
                    if d["zero_copy_calls"] + d["staged_calls"] != 1 or \
                            d["staged_rounds"] != d["staged_calls"] * planned:
                        errs.append(f"{what}: stats {d}, planned {planned} rounds")
        total = comm.exchange_stats()
        comm.close()
        dist.destroy_process_group()
        q.put((rank, "ok", (errs, total)))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc() + str(e)))


@pytest.mark.parametrize("n", [2, 3, 8])
def test_multi_process(n):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mp_worker, args=(r, n, port, q)) for r in range(n)]
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
    errs = [e for r in range(n) for e in out[r][0]]
    assert not errs, "\n".join(errs[:20])
    # the zero-copy pull ran: the jobs' buffers are live allocations of the
    # ranks' caching allocators, which registration takes (the refusal of a
    # re-made allocation is accepted per call above, not for all of them)
    assert out[0][1]["zero_copy_calls"] > 0, out[0][1]
    # every rank saw the same data paths (the decisions are collective)
    assert len({tuple(sorted(out[r][1].items())) for r in range(n)}) == 1, {r: out[r][1] for r in range(n)}
