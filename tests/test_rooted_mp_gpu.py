"""GPU: gather, gatherv, scatter and scatterv between processes (ranks as
processes on the one GPU, n = 2 and 3, a staging of 40 KiB): the staged path
in one round and in rounds, the zero-copy pulls, ranks that describe their
sides differently (the root receives into a vector type while the others send
bytes -- what alltoall cannot express), in place at the root, roots other than
0, a rank that cannot take part, the exchange minimum, and a sequence of
collectives that shares the flag generations.  Expected bytes come from numpy
index maps (tests/ddt_gen.py); every rank builds every rank's source buffer
from seeds, so the expectation needs no communication.  Every byte of every
buffer a rank handed in is checked."""
import os
import socket
import time

import numpy as np
import pytest

import ddt_gen as G
import mxompi
from rooted_util import FILL, GATHER, SCATTER, UNSUPPORTED, Buf, Side, block_len, host_image, move_block, side, span

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_STAGING = 40 << 10      # small: three and more rounds for blocks of a few tens of KiB


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_rng(idx, rank):
    return np.random.default_rng(2000 * idx + rank)


def _b40s56():
    """blen 40 / stride 56: for the staging whose round is a multiple of 24 bytes"""
    sd = Side.__new__(Side)
    sd.name = "b40s56"
    sd.lay = G.Layout([G.Elem(8, 3, 5, 56, 0)], 0, 168, 1)
    sd.dt = mxompi.Datatype(sd.lay.desc, sd.lay.nrec, sd.lay.size, sd.lay.lb, sd.lay.ub)
    sd.size, sd.extent = sd.lay.size, sd.lay.extent
    return sd


def _even(n, count):
    return [count] * n, [p * count for p in range(n)]


def _call(comm, rank, n, idx, kind, root, singles, multi, c1, mc, md, st, inplace=False):
    """One gatherv / scatterv of this rank.  singles[p]: rank p's single side
    (they may differ), c1[p] its instances; multi: the root's side.  Returns an
    error text or None."""
    gather = kind == GATHER
    mine = singles[rank]
    in_place_here = inplace and rank == root
    sing = None if in_place_here else Buf(*span(mine, [c1[rank]], [0]), rng=_rank_rng(idx, rank) if gather else None)
    # the side that is significant on the root only: elsewhere a decoy that must keep its fill
    mult = Buf(*span(multi, mc, md), rng=None if gather or rank != root else _rank_rng(idx, n + root))
    exp_s = None if sing is None else sing.host.copy()
    exp_m = mult.host.copy()
    if gather and rank == root:
        for p in range(n):
            if inplace and p == root:
                continue
            img, base = host_image(*span(singles[p], [c1[p]], [0]), rng=_rank_rng(idx, p))
            move_block(kind, singles[p], multi, c1[p], mc[p], md[p], img, base, exp_m, mult.base)
    if not gather and not in_place_here:
        img, base = host_image(*span(multi, mc, md), rng=_rank_rng(idx, n + root))
        move_block(kind, mine, multi, c1[rank], mc[rank], md[rank], exp_s, sing.base, img, base)
    su = mxompi.IN_PLACE if in_place_here else sing.user
    # what is read on the root only may be anything elsewhere: None, or tables of another call
    on_root = rank == root or rank % 2 == 0
    cm, dm, dtm = (mc, md, multi.dt) if on_root else (None, None, None)
    if gather:
        comm.gatherv(su, c1[rank], mine.dt, mult.user, cm, dm, dtm, root, st)
    else:
        comm.scatterv(mult.user, cm, dm, dtm, su, c1[rank], mine.dt, root, st)
    errs = []
    if sing is not None and sing.wrong(exp_s):
        errs.append("single side: " + sing.wrong(exp_s))
    if mult.wrong(exp_m):
        errs.append(("multi side: " if rank == root else "a buffer that is not significant here: ") + mult.wrong(exp_m))
    return "; ".join(errs) or None


def _max_block(n, root, singles, multi, c1, mc, inplace):
    return max([block_len(singles[p], multi, c1[p], mc[p]) for p in range(n) if not (inplace and p == root)] + [0])


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

        comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=_STAGING)
        comm.set_timeout(30.0)
        st = torch.cuda.current_stream().cuda_stream
        errs, routes = [], {}
        F, V, D, B24, NEG, B16 = side("flat"), side("vec"), side("dispm8"), side("b24s40"), side("negstride"), side("b16s48")
        cap = {k: max(p for p in range(256, _STAGING, 256) if comm.rooted_rounds(k == SCATTER, p) == 1)
               for k in (GATHER, SCATTER)}      # what a round carries of a block
        assert cap[GATHER] % 24, cap                # a gather round's cut falls inside a 24-byte block
        assert cap[GATHER] == max(p for p in range(256, _STAGING, 256) if comm.exchange_rounds(p) == 1)
        assert cap[SCATTER] > cap[GATHER] * (n - 1)  # one sender: the whole staging, not a 1/n slot

        def rounds_case(kind, L, root):
            inst = -(-(3 * cap[kind] + cap[kind] // 2) // L.size)      # the fourth round is half full
            return (f"staged_rounds_{kind}_{L.name}", kind, root, 0, [L] * n, L, [inst] * n, *_even(n, inst), False)

        cases = [
            ("staged_gather", GATHER, 0, 0, [V] * n, D, [20] * n, *_even(n, 20), False),
            ("staged_scatter", SCATTER, n - 1, 0, [side("resized")] * n, B24, [27] * n, *_even(n, 3), False),
            rounds_case(GATHER, B24, 1),
            rounds_case(SCATTER, B24, n - 1),
            ("zero_copy_gather", GATHER, 0, 1, [B24] * n, D, [300] * n, *_even(n, 900), False),
            ("zero_copy_scatter", SCATTER, n - 1, 1, [F] * n, NEG, [50 * 48] * n, *_even(n, 50), False),
            # the root receives into a vector type, every other rank sends bytes (the root too: its own block)
            ("asym_gather", GATHER, 1, 0, [F] * n, V, [24 * 31] * n, *_even(n, 31), False),
            ("asym_gather_zero_copy", GATHER, 0, 1, [F] * n, V, [24 * 500] * n, *_even(n, 500), False),
            # the converse: the root sends from a vector type, the others receive bytes
            ("asym_scatter", SCATTER, 0, 0, [F] * n, V, [24 * 31] * n, *_even(n, 31), False),
            # the sides differ rank by rank: byte pairs and strided pairs in one call
            ("mixed_gather", GATHER, n - 1, 0, [F, B16, F][:n], F, [480, 10, 480][:n], *_even(n, 480), False),
            ("mixed_scatter", SCATTER, 0, 0, [B16, F, D][:n], F, [10, 480, 20][:n], *_even(n, 480), False),
            ("inplace_gather", GATHER, 1, 1, [B24] * n, D, [300] * n, *_even(n, 900), True),
            ("inplace_scatter", SCATTER, 0, 1, [F] * n, F, [4099] * n, [4099] * n, [1 + 4101 * p for p in range(n)], True),
        ]
        if cap[SCATTER] % 24 == 0:                  # this staging cuts a scatter at whole 24-byte blocks:
            assert cap[SCATTER] % 40                # 40-byte blocks are cut inside
            cases.append(rounds_case(SCATTER, _b40s56(), 0))
        for idx, (name, kind, root, reg_min, singles, multi, c1, mc, md, inplace) in enumerate(cases):
            comm.set_reg_min(reg_min)
            by0, dd0, r0 = comm.exchange_stats(), comm.exchange_ddt_stats(), comm.rooted_stats()
            err = _call(comm, rank, n, idx, kind, root, singles, multi, c1, mc, md, st, inplace)
            r1 = comm.rooted_stats()
            d = {k: r1[k] - r0[k] for k in r1}
            what = f"rank {rank} {name}"
            if err:
                errs.append(f"{what}: {err}")
            if comm.exchange_stats() != by0 or comm.exchange_ddt_stats() != dd0:
                errs.append(f"{what}: the exchange counters moved")
            big = _max_block(n, root, singles, multi, c1, mc, inplace)
            planned = comm.rooted_rounds(kind == SCATTER, big)
            if name.startswith("staged_rounds"):
                if planned < 3:
                    errs.append(f"{what}: only {planned} rounds planned")
                if kind == SCATTER and not planned < comm.exchange_rounds(big):
                    errs.append(f"{what}: {planned} rounds, an exchange takes {comm.exchange_rounds(big)}")
            if reg_min == 0 or inplace:              # staged, exactly as planned
                if d != {"calls": 1, "zero_copy_calls": 0, "staged_calls": 1, "staged_rounds": planned}:
                    errs.append(f"{what}: stats {d}, planned {planned} rounds")
            else:   # zero-copy, or staged where the registration was refused (re-made allocations)
                if d["calls"] != 1 or d["zero_copy_calls"] + d["staged_calls"] != 1 or \
                        d["staged_rounds"] != d["staged_calls"] * planned:
                    errs.append(f"{what}: stats {d}, planned {planned} rounds")
            routes[name] = d

        # a rank that is not the root cannot describe its datatype: every rank
        # is told so, soon, nothing is written or counted, and the next call works
        comm.set_reg_min(0)
        for kind in (GATHER, SCATTER):
            root, other = 0, n - 1
            sb, mb = Buf(0, 20 * 48), Buf(0, n * 20 * 48)
            r0, t0 = comm.rooted_stats(), time.monotonic()
            dt = mxompi.DDT_NONE if rank == other else V.dt
            try:
                if kind == GATHER:
                    comm.gather(sb.user, 20, dt, mb.user, 20, V.dt, root, st)
                else:
                    comm.scatter(mb.user, 20, V.dt, sb.user, 20, dt, root, st)
                errs.append(f"rank {rank}: a {kind} with a refusing rank succeeded")
            except mxompi.MxError as e:
                if e.rc != UNSUPPORTED:
                    errs.append(f"rank {rank}: {kind} with a refusing rank gives {e}")
            if time.monotonic() - t0 > 10:
                errs.append(f"rank {rank}: the refusal took {time.monotonic() - t0:.1f} s")
            torch.cuda.synchronize()
            if not bool((sb.dev == FILL).all()) or not bool((mb.dev == FILL).all()) or comm.rooted_stats() != r0:
                errs.append(f"rank {rank}: a refused {kind} moved bytes or was counted")
            err = _call(comm, rank, n, 40, kind, root, [V] * n, D, [30] * n, *_even(n, 30), st)
            if err:
                errs.append(f"rank {rank} {kind} after the refusal: {err}")
        # at or under the exchange minimum: declined alike
        comm.set_exchange_min(1 << 30)
        sb, mb = Buf(0, 20 * 48), Buf(0, n * 20 * 48)
        r0 = comm.rooted_stats()
        for kind in (GATHER, SCATTER):
            try:
                if kind == GATHER:
                    comm.gather(sb.user, 20, V.dt, mb.user, 20, V.dt, 0, st)
                else:
                    comm.scatter(mb.user, 20, V.dt, sb.user, 20, V.dt, 0, st)
                errs.append(f"rank {rank}: a {kind} under the exchange minimum ran")
            except mxompi.MxError as e:
                if e.rc != UNSUPPORTED:
                    errs.append(f"rank {rank}: exchange minimum gives {e}")
        torch.cuda.synchronize()
        if not bool((sb.dev == FILL).all()) or not bool((mb.dev == FILL).all()) or comm.rooted_stats() != r0:
            errs.append(f"rank {rank}: a call under the exchange minimum moved bytes or was counted")
        comm.set_exchange_min(0)

        # one sequence with nothing between the calls: gather (root 0), scatter
        # (root n - 1), alltoall, allreduce, gather (root 1) share the flag generations
        blk = 4096
        a2a_s = torch.from_numpy(_rank_rng(70, rank).integers(0, 256, n * blk, dtype=np.uint8)).to("cuda:0")
        a2a_r = torch.zeros(n * blk, dtype=torch.uint8, device="cuda:0")
        ar_s = torch.full((1024,), float(rank + 1), dtype=torch.float32, device="cuda:0")
        ar_r = torch.zeros(1024, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        seq = [_call(comm, rank, n, 60, GATHER, 0, [B24] * n, D, [40] * n, *_even(n, 120), st),
               _call(comm, rank, n, 61, SCATTER, n - 1, [F] * n, V, [24 * 90] * n, *_even(n, 90), st)]
        comm.alltoall(a2a_s.data_ptr(), a2a_r.data_ptr(), blk, st)
        comm.allreduce(ar_s.data_ptr(), ar_r.data_ptr(), 1024, "FLOAT", "SUM", stream=st)
        seq.append(_call(comm, rank, n, 62, GATHER, 1, [F] * n, B16, [48 * 33] * n, *_even(n, 33), st))
        torch.cuda.synchronize()
        for k, err in enumerate(seq):
            if err:
                errs.append(f"rank {rank} sequence call {k}: {err}")
        want = np.concatenate([_rank_rng(70, p).integers(0, 256, n * blk, dtype=np.uint8)[rank * blk:(rank + 1) * blk]
                               for p in range(n)])
        if not np.array_equal(a2a_r.cpu().numpy(), want):
            errs.append(f"rank {rank}: the alltoall of the sequence is wrong")
        if not bool((ar_r == float(n * (n + 1) // 2)).all()):
            errs.append(f"rank {rank}: the allreduce of the sequence is wrong")
        comm.close()
        dist.destroy_process_group()
        q.put((rank, "ok", (errs, routes)))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc() + str(e)))


@pytest.mark.parametrize("n", [2, 3])
def test_multi_process(n):
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
    errs = [e for r in range(n) for e in out[r][0]]
    assert not errs, "\n".join(errs[:20])
    # every rank saw the same data paths (the decisions are collective), and a
    # zero-copy pull ran (fresh allocations of the caching allocator register)
    for r in range(1, n):
        assert out[r][1] == out[0][1], (out[r][1], out[0][1])
    zc = sum(d["zero_copy_calls"] for d in out[0][1].values())
    assert zc > 0, out[0][1]
