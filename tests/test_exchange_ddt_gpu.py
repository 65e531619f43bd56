"""GPU: alltoall and alltoallv of strided datatypes on the fused exchange
kernel (csrc/mx_exchange_vec.hip).  Pure data movement: expected bytes come
from numpy index maps of the datatypes' description trees (tests/ddt_gen.py),
never from the library.  Every test checks EVERY byte of every receive buffer:
the layout's bytes against numpy, gap bytes and bytes past the end still the
fill.  Local communicators (n = 2..4) drive the kernel through a matrix of
send and receive layouts, the stream sizes where its paths change, ragged
tables and the declined layouts; multi-process communicators (ranks as
processes on the one GPU) run the staged and the zero-copy data paths."""
import os
import socket
import time

import numpy as np
import pytest

import ddt_gen as G
import mxompi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 0xA5
PAD = 512          # bytes kept around every buffer's span (they must keep the fill)
UNSUPPORTED = -2


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ready():
    mxompi.init(0)
    return True


# ---- the layouts -----------------------------------------------------------------
# name: (nodes, lb, extent); blen / stride / extent in bytes as the comments say
def _nodes(name):
    E = G.Elem
    return {
        "b4s8": ([E(4, 6, 1, 8, 0)], 0, 48),             # blen 4 / stride 8
        "vec": ([E(4, 3, 2, 20, 0)], 0, 48),             # blen 8 / stride 20 / extent 48 (the mini-host's VEC)
        "b12s20": ([E(4, 4, 3, 20, 0)], 0, 80),          # blen 12 / stride 20
        "b24s40": ([E(8, 3, 3, 40, 0)], 0, 120),         # blen 24 / stride 40
        "b16s48": ([E(16, 3, 1, 48, 0)], 0, 144),        # blen 16 / stride 48
        "b48s64": ([E(16, 2, 3, 64, 0)], 0, 128),        # blen 48 / stride 64
        "resized": ([E(8, 1, 1, 8, 0)], 0, 24),          # resized contiguous: blen 8, extent 24, cnt1 1
        "dispm8": ([E(8, 3, 1, 24, -8)], -8, 72),        # disp -8
        "negstride": ([E(8, 3, 2, -32, 64)], 0, 96),     # blen 16, stride -32: a send side only
        # the declined ones
        "struct2": ([E(4, 2, 1, 8, 0), E(8, 1, 1, 8, 32)], 0, 40),
        "twolevel": ([G.Loop(3, 64, [E(4, 2, 1, 8, 0)])], 0, 192),
        "b2s4": ([E(2, 4, 1, 4, 0)], 0, 16),
        "bigblen": ([E(16, 1, (1 << 22) // 16 + 1, (1 << 22) + 16, 0)], 0, 2 * ((1 << 22) + 16)),   # blen 4 MiB + 16
    }[name]


class Side:
    """One side of a call: a datatype (or None: bytes) with its numpy map."""

    def __init__(self, name):
        self.name = name
        if name == "flat":
            self.lay, self.dt, self.size, self.extent = None, None, 1, 1
        else:
            nodes, lb, ext = _nodes(name)
            self.lay = G.Layout(nodes, lb, ext, 1)
            self.dt = mxompi.Datatype(self.lay.desc, self.lay.nrec, self.lay.size, self.lay.lb, self.lay.ub)
            self.size, self.extent = self.lay.size, self.lay.extent

    def map(self, count, displ):
        """user offset of every stream byte of `count` instances `displ` extents in"""
        if self.lay is None:
            return np.arange(count, dtype=np.int64) + displ
        return self.lay.map_all(count) + displ * self.extent

    def unit(self):
        """the access unit of the layout alone (buffers here are 256-byte aligned)"""
        if self.lay is None:
            return 16
        e = self.lay.nodes[0]
        u = 16
        for v in (e.blk, abs(e.disp), abs(e.extent) if e.count > 1 else 0, abs(self.extent)):
            while v % u:
                u //= 2
        return u


_SIDES = {}


def side(name):
    if name not in _SIDES:
        _SIDES[name] = Side(name)
    return _SIDES[name]


def _span(sd, counts, displs):
    """[lo, hi) of the user offsets a rank's row touches (0, 0 for an empty row)"""
    lo, hi = 0, 0
    for c, d in zip(counts, displs):
        if c:
            m = sd.map(c, d)
            lo, hi = min(lo, int(m.min())), max(hi, int(m.max()) + 1)
    return lo, hi


class Buf:
    """A device buffer around a span: `user` is the address the call gets."""

    def __init__(self, lo, hi, data=None):
        self.base = PAD + (-lo + 255) // 256 * 256 if lo < 0 else PAD      # the user pointer stays 256-byte aligned
        self.n = self.base + hi + PAD
        self.host = np.full(self.n, FILL, np.uint8) if data is None else data(self.n)
        self.dev = torch.from_numpy(self.host.copy()).to("cuda:0")
        assert self.dev.data_ptr() % 256 == 0
        self.user = self.dev.data_ptr() + self.base


def _expected(n, S, R, sc, sd, rc, rd, sbufs, rbufs):
    """numpy's receive buffers: pair i -> j moves min(send, room) stream bytes"""
    exp = [b.host.copy() for b in rbufs]
    for i in range(n):
        for j in range(n):
            ln = min(sc[i][j] * S.size, rc[j][i] * R.size)
            if ln:
                sm = S.map(sc[i][j], sd[i][j])[:ln] + sbufs[i].base
                rm = R.map(rc[j][i], rd[j][i])[:ln] + rbufs[j].base
                exp[j][rm] = sbufs[i].host[sm]
    return exp


def _check(rbufs, exp, what):
    torch.cuda.synchronize()
    for j, (b, e) in enumerate(zip(rbufs, exp)):
        got = b.dev.cpu().numpy()
        bad = np.nonzero(got != e)[0]
        assert bad.size == 0, (f"{what} rank {j}: {bad.size} wrong bytes, first at user offset {bad[0] - b.base} "
                               f"(got {got[bad[0]]:#x}, expected {e[bad[0]]:#x})")


def _local_v(n, S, R, sc, sd, rc, rd, seed, what, expect_w="auto"):
    """One alltoallv_ddt_local call on fresh buffers, every byte checked; the
    word width the launch took is read back from the library's job counters."""
    rng = np.random.default_rng(seed)
    comm = mxompi.Comm.local(n)
    try:
        sbufs = [Buf(*_span(S, sc[i], sd[i]), data=lambda k: rng.integers(0, 256, k, dtype=np.uint8)) for i in range(n)]
        rbufs = [Buf(*_span(R, rc[j], rd[j])) for j in range(n)]
        exp = _expected(n, S, R, sc, sd, rc, rd, sbufs, rbufs)
        flat = lambda m: [v for row in m for v in row]   # noqa: E731
        w0, st0, by0 = mxompi.exchange_vec_widths(), comm.exchange_ddt_stats(), comm.exchange_stats()
        comm.alltoallv_ddt_local([b.user for b in sbufs], flat(sc), flat(sd), S.dt, [b.user for b in rbufs], flat(rc),
                                 flat(rd), R.dt, _stream())
        _check(rbufs, exp, what)
        w1, st1 = mxompi.exchange_vec_widths(), comm.exchange_ddt_stats()
        assert st1["calls"] - st0["calls"] == 1 and comm.exchange_stats() == by0, (what, st0, st1)
        jobs = sum(1 for i in range(n) for j in range(n) if min(sc[i][j] * S.size, rc[j][i] * R.size))
        took = {w: w1[w] - w0[w] for w in w1}
        if expect_w == "auto":
            expect_w = None if S.lay is None and R.lay is None else min(S.unit(), R.unit())
        want = {w: (jobs if w == expect_w else 0) for w in (4, 8, 16)}
        assert took == want, f"{what}: jobs by width {took}, expected {want}"
    finally:
        comm.close()


def _alltoall_tables(n, scount, rcount):
    sc = [[scount] * n for _ in range(n)]
    rc = [[rcount] * n for _ in range(n)]
    sd = [[j * scount for j in range(n)] for _ in range(n)]
    rd = [[i * rcount for i in range(n)] for _ in range(n)]
    return sc, sd, rc, rd


# -- 1. the layout matrix -----------------------------------------------------------
SEND = ["flat", "b4s8", "vec", "b12s20", "b24s40", "b16s48", "b48s64", "resized", "dispm8", "negstride"]
RECV = SEND[:-1]
PAIR = 288         # lcm of the layouts' instance sizes, and a multiple of 16 (a flat side counts bytes)


@pytest.mark.parametrize("sname", SEND)
def test_layout_matrix(ready, sname):
    """Every send layout against every receive layout, alltoall on n = 2..4:
    together W = 4, 8 and 16 and the three flat / strided combinations (flat
    to flat goes to the byte kernel: no strided job is counted)."""
    S = side(sname)
    seen = set()
    for k, rname in enumerate(RECV):
        R = side(rname)
        n = 2 + (k + len(sname)) % 3
        pair = PAIR * (1 + k % 3)
        assert pair % S.size == 0 and pair % R.size == 0
        _local_v(n, S, R, *_alltoall_tables(n, pair // S.size, pair // R.size), seed=7 * k + len(sname),
                 what=f"{sname} -> {rname} n={n}")
        seen.add(None if S.lay is None and R.lay is None else min(S.unit(), R.unit()))
    if sname in ("flat", "b16s48", "b48s64", "negstride"):
        assert {4, 8, 16} <= seen, seen       # the widths the matrix promises
    assert side("vec").unit() == 4 and side("dispm8").unit() == 8 and side("b48s64").unit() == 16


def test_alltoall_form_matches_v_form(ready):
    """mx_alltoall_ddt_local lays its blocks out as MPI_Alltoall does."""
    n, S, R = 3, side("b24s40"), side("dispm8")
    sc, sd, rc, rd = _alltoall_tables(n, 8, 24)
    rng = np.random.default_rng(3)
    comm = mxompi.Comm.local(n)
    try:
        sbufs = [Buf(*_span(S, sc[i], sd[i]), data=lambda k: rng.integers(0, 256, k, dtype=np.uint8)) for i in range(n)]
        rbufs = [Buf(*_span(R, rc[j], rd[j])) for j in range(n)]
        exp = _expected(n, S, R, sc, sd, rc, rd, sbufs, rbufs)
        comm.alltoall_ddt_local([b.user for b in sbufs], 8, S.dt, [b.user for b in rbufs], 24, R.dt, _stream())
        _check(rbufs, exp, "alltoall_ddt_local")
    finally:
        comm.close()


# -- 2. one word below, at and above a workgroup's and a wave step's share ------------
@pytest.mark.parametrize("unit", ["workgroup", "wave"])
@pytest.mark.parametrize("shape", ["strided_to_flat", "flat_to_strided", "strided_to_strided"])
def test_stream_boundaries(ready, unit, shape):
    """b24s40 moves by 8-byte words and its 24-byte blocks divide neither
    share.  The strided side announces whole instances, the other side has
    room for exactly the stream under test, so the pair is cut there."""
    W = 8
    block, wave = mxompi.exchange_vec_geometry(W)
    base = block if unit == "workgroup" else wave
    assert base % 24 and wave == 64 * W and block % wave == 0
    V, n = side("b24s40"), 2
    for stream in (base - W, base, base + W):
        whole = -(-stream // V.size) + 1                       # instances: more than the stream
        if shape == "strided_to_flat":
            S, R, scount, rcount = V, side("flat"), whole, stream
        elif shape == "flat_to_strided":
            S, R, scount, rcount = side("flat"), V, stream, whole
        else:
            S, R, scount, rcount = V, side("resized"), whole, stream // 8
        _local_v(n, S, R, *_alltoall_tables(n, scount, rcount), seed=stream, what=f"{shape} {stream}", expect_w=W)


# -- 3. ragged alltoallv ---------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4])
def test_ragged_alltoallv(ready, n):
    """Zero counts, a rank that sends nothing, displacements with gaps, one
    pair far larger than the rest, a receiver with less room than announced."""
    S, R = side("vec"), side("dispm8")              # both 24 bytes an instance; words of 4
    rng = np.random.default_rng(60 + n)
    sc = rng.integers(0, 40, (n, n)).tolist()
    sc[n - 1] = [0] * n                             # a rank that sends nothing
    sc[1][0] = 0
    sc[0][n - 1] = 9000                             # one pair far larger: 216 000 bytes, many workgroups
    rc = [[sc[i][j] for i in range(n)] for j in range(n)]
    rc[1][0] = max(0, sc[0][1] - 3)                 # less room than its sender announces
    rc[2][1] = sc[1][2] + 5                         # more room than is sent
    sd, rd = [], []
    for i in range(n):
        o, row = 1 + i, []
        for j in range(n):
            row.append(o)
            o += sc[i][j] + 1 + j
        sd.append(row)
    for j in range(n):
        o, row = 2, []
        for i in range(n):
            row.append(o)
            o += rc[j][i] + 2 + i
        rd.append(row)
    _local_v(n, S, R, sc, sd, rc, rd, seed=n, what=f"ragged n={n}")


# -- 4. differential: fused == pack -> alltoall_local -> unpack ------------------------
@pytest.mark.parametrize("sname,rname", [("b24s40", "b12s20"), ("negstride", "b16s48"), ("vec", "resized")])
def test_fused_equals_pack_exchange_unpack(ready, sname, rname):
    n, S, R = 3, side(sname), side(rname)
    pair = PAIR * 40
    scount, rcount = pair // S.size, pair // R.size
    sc, sd, rc, rd = _alltoall_tables(n, scount, rcount)
    rng = np.random.default_rng(11)
    comm = mxompi.Comm.local(n)
    try:
        sbufs = [Buf(*_span(S, sc[i], sd[i]), data=lambda k: rng.integers(0, 256, k, dtype=np.uint8)) for i in range(n)]
        fused = [Buf(*_span(R, rc[j], rd[j])) for j in range(n)]
        three = [Buf(*_span(R, rc[j], rd[j])) for j in range(n)]
        st = _stream()
        comm.alltoall_ddt_local([b.user for b in sbufs], scount, S.dt, [b.user for b in fused], rcount, R.dt, st)
        packed = [torch.empty(n * pair, dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        moved = [torch.empty(n * pair, dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        for i in range(n):
            S.dt.pack(n * scount, sbufs[i].user, packed[i].data_ptr(), stream=st)
        comm.alltoall_local([t.data_ptr() for t in packed], [t.data_ptr() for t in moved], pair, st)
        for j in range(n):
            R.dt.unpack(n * rcount, three[j].user, moved[j].data_ptr(), stream=st)
        torch.cuda.synchronize()
        for j in range(n):
            assert torch.equal(fused[j].dev, three[j].dev), f"rank {j}: fused and composed results differ"
        _check(fused, _expected(n, S, R, sc, sd, rc, rd, sbufs, fused), "fused")
    finally:
        comm.close()


# -- 5. declines -------------------------------------------------------------------------
@pytest.mark.parametrize("sname,rname", [("struct2", "vec"), ("vec", "struct2"), ("twolevel", "vec"),
                                         ("vec", "twolevel"), ("b2s4", "flat"), ("flat", "b2s4"),
                                         ("vec", "negstride"), ("bigblen", "flat"), ("flat", "bigblen")])
def test_declines_leave_buffers_untouched(ready, sname, rname):
    """A two-run struct, a two-level layout, 2-byte blocks, a non-monotonic
    receive layout and blocks above the limit: MX_ERR_UNSUPPORTED, nothing
    written, no call counted."""
    n, S, R = 2, side(sname), side(rname)
    stream = int(np.lcm(S.size, R.size))
    sc, sd, rc, rd = _alltoall_tables(n, stream // S.size, stream // R.size)
    comm = mxompi.Comm.local(n)
    try:
        sbufs = [Buf(*_span(S, sc[i], sd[i])) for i in range(n)]
        rbufs = [Buf(*_span(R, rc[j], rd[j])) for j in range(n)]
        before = comm.exchange_ddt_stats()
        with pytest.raises(mxompi.MxError) as e:
            comm.alltoall_ddt_local([b.user for b in sbufs], stream // S.size, S.dt, [b.user for b in rbufs],
                                    stream // R.size, R.dt, _stream())
        assert e.value.rc == UNSUPPORTED
        torch.cuda.synchronize()
        for b in rbufs:
            assert bool((b.dev == FILL).all())
        assert comm.exchange_ddt_stats() == before
    finally:
        comm.close()


def test_strided_answers(ready):
    """mx_ddt_strided is the qualification: one run of one level, blocks up to
    the limit, and a monotonic layout where it receives."""
    for name in RECV[1:]:
        assert side(name).dt.strided(False) and side(name).dt.strided(True), name
    assert side("negstride").dt.strided(False) and not side("negstride").dt.strided(True)
    assert side("b2s4").dt.strided(True)            # a layout the word rule declines, not the qualification
    for name in ("struct2", "twolevel", "bigblen"):
        assert not side(name).dt.strided(False) and not side(name).dt.strided(True), name


# -- 6. multi-process: staged, staged in rounds, zero-copy, in place, a refusing rank ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_STAGING = 40 << 10      # small: three and more rounds for pairs of a few tens of KiB


def _rank_rng(idx, rank):
    return np.random.default_rng(1000 * idx + rank)


def _mp_call(comm, rank, n, idx, S, R, sc, sd, rc, rd, st, inplace=False):
    """One alltoallv_ddt of this rank; every rank builds every rank's send
    buffer from seeds, so the expectation needs no communication.  Returns an
    error text or None."""
    if inplace:
        S, sc, sd = R, [[rc[i][j] for j in range(n)] for i in range(n)], rd
    sh = [Buf(*_span(S, sc[i], sd[i]), data=lambda k, i=i: _rank_rng(idx, i).integers(0, 256, k, dtype=np.uint8))
          if i == rank else None for i in range(n)]
    # host images of the peers' send buffers (the same seeds), without device memory
    hosts, bases = [], []
    for i in range(n):
        lo, hi = _span(S, sc[i], sd[i])
        base = PAD + (-lo + 255) // 256 * 256 if lo < 0 else PAD
        hosts.append(_rank_rng(idx, i).integers(0, 256, base + hi + PAD, dtype=np.uint8))
        bases.append(base)
    if inplace:
        rb = sh[rank]
        exp = rb.host.copy()
    else:
        rb = Buf(*_span(R, rc[rank], rd[rank]))
        exp = rb.host.copy()
    for i in range(n):
        ln = min(sc[i][rank] * S.size, rc[rank][i] * R.size)
        if ln:
            sm = S.map(sc[i][rank], sd[i][rank])[:ln] + bases[i]
            rm = R.map(rc[rank][i], rd[rank][i])[:ln] + rb.base
            exp[rm] = hosts[i][sm]
    comm.alltoallv_ddt(None if inplace else sh[rank].user, sc[rank], sd[rank], S.dt, rb.user, rc[rank], rd[rank], R.dt, st)
    got = rb.dev.cpu().numpy()
    bad = np.nonzero(got != exp)[0]
    return None if bad.size == 0 else f"{bad.size} wrong bytes, first at user offset {bad[0] - rb.base}"


def _mp_tables(n, idx, per_pair):
    """ragged counts around per_pair instances, one empty pair, displacements with gaps"""
    rng = np.random.default_rng(500 + idx)
    sc = (per_pair + rng.integers(0, 6, (n, n))).tolist()
    sc[0][n - 1] = 0
    rc = [[sc[i][j] for i in range(n)] for j in range(n)]
    sd = [[sum(sc[i][:j]) + 2 * j + 1 for j in range(n)] for i in range(n)]
    rd = [[sum(rc[j][:i]) + 3 * i + 2 for i in range(n)] for j in range(n)]
    return sc, sd, rc, rd


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
        errs, routes = [], {}
        V, D, B24 = side("vec"), side("dispm8"), side("b24s40")
        cap = max(p for p in range(256, _STAGING, 256) if comm.exchange_rounds(p) == 1)   # what a round carries per pair
        assert cap % 24, cap                       # a round's cut falls inside a 24-byte block
        rounds_pair = -(-(3 * cap + cap // 2) // B24.size)       # instances: the fourth round is half full
        jobs = [
            ("staged", 0, V, D, _mp_tables(n, 1, 20), False),
            ("staged_rounds", 0, B24, B24, _mp_tables(n, 2, rounds_pair), False),
            ("zero_copy", 1, B24, D, _mp_tables(n, 3, 300), False),
            ("zero_copy_flat_recv", 1, side("negstride"), side("flat"),
             _alltoall_tables(n, 50, 50 * 48), False),
            ("inplace", 1, None, V, _alltoall_tables(n, 700, 700), True),
        ]
        for idx, (kind, reg_min, S, R, (sc, sd, rc, rd), inplace) in enumerate(jobs):
            comm.set_reg_min(reg_min)
            by0, d0 = comm.exchange_stats(), comm.exchange_ddt_stats()
            err = _mp_call(comm, rank, n, idx, S, R, sc, sd, rc, rd, st, inplace)
            d1 = comm.exchange_ddt_stats()
            d = {k: d1[k] - d0[k] for k in d1}
            what = f"rank {rank} {kind}"
            if err:
                errs.append(f"{what}: {err}")
            if comm.exchange_stats() != by0:
                errs.append(f"{what}: the byte forms' counters moved")
            Ssz = (R if inplace else S).size
            planned = comm.exchange_rounds(max(max(row) for row in (rc if inplace else sc)) * Ssz)
            if kind == "staged_rounds" and planned < 3:
                errs.append(f"{what}: only {planned} rounds planned")
            if reg_min == 0 or inplace:              # staged, exactly as planned
                if d != {"calls": 1, "zero_copy_calls": 0, "staged_calls": 1, "staged_rounds": planned}:
                    errs.append(f"{what}: stats {d}, planned {planned} rounds")
            else:   # zero-copy, or staged where the registration was refused (re-made allocations)
                if d["calls"] != 1 or d["zero_copy_calls"] + d["staged_calls"] != 1 or \
                        d["staged_rounds"] != d["staged_calls"] * planned:
                    errs.append(f"{what}: stats {d}, planned {planned} rounds")
            routes[kind] = d
        # one rank passes a type the kernel does not take (another one a type it
        # cannot describe at all): every rank is told so, soon, and nothing moved
        comm.set_reg_min(0)
        bad = side("struct2").dt if rank == 0 else (mxompi.DDT_NONE if rank == 1 and n > 2 else V.dt)
        R = Buf(0, n * 20 * 48)
        Sb = Buf(0, n * 20 * 48)
        d0, t0 = comm.exchange_ddt_stats(), time.monotonic()
        try:
            comm.alltoall_ddt(Sb.user, 20, bad, R.user, 20, V.dt, st)
            errs.append(f"rank {rank}: a call with a refusing rank succeeded")
        except mxompi.MxError as e:
            if e.rc != UNSUPPORTED:
                errs.append(f"rank {rank}: refusing rank gives {e}")
        if time.monotonic() - t0 > 10:
            errs.append(f"rank {rank}: the refusal took {time.monotonic() - t0:.1f} s")
        torch.cuda.synchronize()
        if not bool((R.dev == FILL).all()) or comm.exchange_ddt_stats() != d0:
            errs.append(f"rank {rank}: a refused call moved bytes or was counted")
        err = _mp_call(comm, rank, n, 9, V, D, *_mp_tables(n, 9, 30), st)     # the communicator still works
        if err:
            errs.append(f"rank {rank} after the refusal: {err}")
        # at or under the exchange minimum: declined alike
        comm.set_exchange_min(1 << 30)
        try:
            comm.alltoall_ddt(Sb.user, 20, V.dt, R.user, 20, V.dt, st)
            errs.append(f"rank {rank}: a call under the exchange minimum ran")
        except mxompi.MxError as e:
            if e.rc != UNSUPPORTED:
                errs.append(f"rank {rank}: exchange minimum gives {e}")
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
    # every rank saw the same data paths (the decisions are collective), and
    # the zero-copy pull ran (fresh allocations of the caching allocator register)
    for r in range(1, n):
        assert out[r][1] == out[0][1], (out[r][1], out[0][1])
    assert out[0][1]["zero_copy"]["zero_copy_calls"] + out[0][1]["zero_copy_flat_recv"]["zero_copy_calls"] > 0, out[0][1]
