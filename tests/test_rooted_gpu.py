"""GPU: gather, gatherv, scatter and scatterv on the two exchange kernels, on
local communicators (n = 1..4).  Pure data movement: expected bytes come from
numpy index maps of the datatypes' description trees (tests/ddt_gen.py), never
from the library.  Every test checks EVERY byte of every buffer it handed in:
the layout's bytes against numpy; gap bytes, the padding around each span, the
send buffers and the buffers that are not significant still what they were."""
import numpy as np
import pytest

import mxompi
from rooted_util import ARG, FILL, GATHER, SCATTER, UNSUPPORTED, Buf, block_len, move_block, side, span

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ready():
    mxompi.init(0)
    return True


def _run(kind, n, root, single, multi, c1, mc, md, seed, what, inplace=False, s_shift=0, m_shift=0, expect_w="auto",
         comm=None):
    """One gatherv_local / scatterv_local call on fresh buffers, every byte of
    every buffer checked.  single: the side every rank has one block of (c1[p]
    instances); multi: the root's side (mc[p] instances md[p] extents in).  The
    ranks that are not the root hand in a buffer for the side that is not
    significant there: it must stay the fill."""
    rng = np.random.default_rng(seed)
    own = comm is None
    comm = comm or mxompi.Comm.local(n)
    try:
        gather = kind == GATHER
        sing = [Buf(*span(single, [c1[p]], [0]), shift=s_shift, rng=rng if gather else None) for p in range(n)]
        mult = [Buf(*span(multi, mc, md), shift=m_shift, rng=None if gather or p != root else rng) for p in range(n)]
        exp_s = [b.host.copy() for b in sing]
        exp_m = [b.host.copy() for b in mult]
        jobs = 0
        for p in range(n):
            if inplace and p == root:
                continue
            move_block(kind, single, multi, c1[p], mc[p], md[p], exp_s[p], sing[p].base, exp_m[root], mult[root].base)
            jobs += 1 if block_len(single, multi, c1[p], mc[p]) else 0
        sp = [mxompi.IN_PLACE if inplace and p == root else sing[p].user for p in range(n)]
        mp = [b.user for b in mult]
        w0, st0 = mxompi.exchange_vec_widths(), comm.rooted_stats()
        by0, d0 = comm.exchange_stats(), comm.exchange_ddt_stats()
        if gather:
            comm.gatherv_local(sp, c1, single.dt, mp, mc, md, multi.dt, root, _stream())
        else:
            comm.scatterv_local(mp, mc, md, multi.dt, sp, c1, single.dt, root, _stream())
        torch.cuda.synchronize()
        for p in range(n):
            for b, e, name in ((sing[p], exp_s[p], "single"), (mult[p], exp_m[p], "multi")):
                bad = b.wrong(e)
                assert bad is None, f"{what}: rank {p} {name} side: {bad}"
        st1 = comm.rooted_stats()
        assert st1["calls"] - st0["calls"] == 1, (what, st0, st1)
        assert comm.exchange_stats() == by0 and comm.exchange_ddt_stats() == d0, f"{what}: the exchange counters moved"
        took = {w: v - w0[w] for w, v in mxompi.exchange_vec_widths().items()}
        if expect_w == "auto":
            expect_w = None if single.lay is None and multi.lay is None else min(single.unit(), multi.unit())
        want = {w: (jobs if w == expect_w else 0) for w in (4, 8, 16)}
        assert took == want, f"{what}: jobs by width {took}, expected {want}"
        return expect_w
    finally:
        if own:
            comm.close()


def _even(n, count):
    return [count] * n, [p * count for p in range(n)]


# -- 1. the layout matrix -------------------------------------------------------------
SEND = ["flat", "b4s8", "b24s40", "b48s64", "negstride"]
RECV = ["flat", "vec", "dispm8", "resized", "b16s48"]
BLOCK = 288        # lcm of the layouts' instance sizes, and a multiple of 16 (a flat side counts bytes)


@pytest.mark.parametrize("kind", [GATHER, SCATTER])
def test_layout_matrix(ready, kind):
    """Every send layout against every receive layout with the root rotating
    over the ranks of n = 2..4: together W = 4, 8 and 16, and the flat -> flat
    pair on the byte kernel (no strided job is counted)."""
    seen, k = set(), 0
    comms = {n: mxompi.Comm.local(n) for n in (2, 3, 4)}
    try:
        for sname in SEND:
            for rname in RECV:
                S, R = side(sname), side(rname)
                n = 2 + k % 3
                root = (k // 3) % n
                block = BLOCK * (1 + (k + k // 5) % 3)
                single, multi = (S, R) if kind == GATHER else (R, S)
                mc, md = _even(n, block // multi.size)
                seen.add(_run(kind, n, root, single, multi, [block // single.size] * n, mc, md, seed=100 + k,
                              what=f"{kind} {sname} -> {rname} n={n} root={root}", comm=comms[n]))
                k += 1
    finally:
        for c in comms.values():
            c.close()
    assert seen == {None, 4, 8, 16}, seen           # None: flat -> flat, no strided job
    for W in (4, 8, 16):                            # the widths are the kernel's: its geometry knows them
        blk, wave = mxompi.exchange_vec_geometry(W)
        assert wave == 64 * W and blk % wave == 0
    assert side("vec").unit() == 4 and side("dispm8").unit() == 8 and side("b48s64").unit() == 16


def test_even_forms_match_v_forms(ready):
    """mx_gather_local / mx_scatter_local lay their blocks out as MPI does: rank p's at p x count."""
    n, root, S, R = 3, 2, side("b24s40"), side("dispm8")
    rng = np.random.default_rng(5)
    comm = mxompi.Comm.local(n)
    try:
        for kind in (GATHER, SCATTER):
            single, multi = (S, R) if kind == GATHER else (R, S)
            c1, cm = 576 // single.size, 576 // multi.size
            mc, md = _even(n, cm)
            sing = [Buf(*span(single, [c1], [0]), rng=rng if kind == GATHER else None) for _ in range(n)]
            mult = Buf(*span(multi, mc, md), rng=None if kind == GATHER else rng)
            exp_s, exp_m = [b.host.copy() for b in sing], mult.host.copy()
            for p in range(n):
                move_block(kind, single, multi, c1, mc[p], md[p], exp_s[p], sing[p].base, exp_m, mult.base)
            sp, mp = [b.user for b in sing], [mult.user if p == root else None for p in range(n)]
            if kind == GATHER:
                comm.gather_local(sp, c1, single.dt, mp, cm, multi.dt, root, _stream())
            else:
                comm.scatter_local(mp, cm, multi.dt, sp, c1, single.dt, root, _stream())
            torch.cuda.synchronize()
            assert mult.wrong(exp_m) is None, (kind, mult.wrong(exp_m))
            for p in range(n):
                assert sing[p].wrong(exp_s[p]) is None, (kind, p, sing[p].wrong(exp_s[p]))
    finally:
        comm.close()


# -- 2. byte forms: no word rule ----------------------------------------------------------
@pytest.mark.parametrize("kind", [GATHER, SCATTER])
@pytest.mark.parametrize("block", [1, 15, 17, 4099])
def test_bytes_any_length_any_alignment(ready, kind, block):
    """Flat to flat: the send buffer 1 and 3 bytes past a 256-byte boundary,
    the receive buffer 5 past one, odd displacements, odd lengths."""
    n, F = 3, side("flat")
    stride = block + block % 2 + 2                  # even: 1 + p * stride stays odd
    md = [1 + p * stride for p in range(n)]
    for send_shift in (1, 3):
        s_shift, m_shift = (send_shift, 5) if kind == GATHER else (5, send_shift)
        _run(kind, n, block % n, F, F, [block] * n, [block] * n, md, seed=block + send_shift,
             what=f"{kind} {block} bytes at +{send_shift}", s_shift=s_shift, m_shift=m_shift)


# -- 3. ragged gatherv / scatterv -----------------------------------------------------------
@pytest.mark.parametrize("kind", [GATHER, SCATTER])
@pytest.mark.parametrize("root", [1, 2])
def test_ragged_v_forms(ready, kind, root):
    """Ranks with count 0 (rank 1: the root among them once), displacements
    with gaps and in non-rank order, one block of 9000 instances of a 24-byte
    type (many workgroups), a receiver with 3 instances less room than
    announced and one with 5 more."""
    n = 4
    S, R = side("vec"), side("dispm8")              # both 24 bytes an instance; words of 4
    single, multi = (S, R) if kind == GATHER else (R, S)
    c1 = [37, 0, 9000, 21]
    mc = list(c1)
    if kind == GATHER:                              # the root's multi side receives
        mc[0], mc[3] = c1[0] - 3, c1[3] + 5
    else:                                           # the single sides receive
        c1[0], c1[3] = mc[0] - 3, mc[3] + 5
    md = [9100, 9090, 40, 2]                        # non-rank order, gaps of a few extents between the blocks
    assert md[3] + mc[3] < md[2] and md[2] + mc[2] < md[1] <= md[0] - mc[1]
    _run(kind, n, root, single, multi, c1, mc, md, seed=40 + root, what=f"ragged {kind} root={root}")


# -- 4. one word below, at and above a workgroup's and a wave step's share -------------------
@pytest.mark.parametrize("unit", ["workgroup", "wave"])
@pytest.mark.parametrize("kind", [GATHER, SCATTER])
def test_stream_boundaries(ready, kind, unit):
    """b24s40 moves by 8-byte words and its 24-byte blocks divide neither
    share: a gather into it (the senders announce the stream under test in
    bytes, the root has room for more) and a scatter out of it (the root
    announces whole instances, the receivers have room for the stream)."""
    W = 8
    block, wave = mxompi.exchange_vec_geometry(W)
    base = block if unit == "workgroup" else wave
    assert base % 24 and wave == 64 * W and block % wave == 0
    V, F, n = side("b24s40"), side("flat"), 2
    for stream in (base - W, base, base + W):
        whole = -(-stream // V.size) + 1            # instances: more than the stream
        mc, md = _even(n, whole)
        _run(kind, n, 1, F, V, [stream] * n, mc, md, seed=stream, what=f"{kind} {unit} {stream}", expect_w=W)


# -- 5. in place at the root ------------------------------------------------------------------
@pytest.mark.parametrize("kind", [GATHER, SCATTER])
@pytest.mark.parametrize("sname,mname", [("flat", "flat"), ("b24s40", "dispm8"), ("flat", "vec"), ("b16s48", "flat")])
def test_in_place_at_the_root(ready, kind, sname, mname):
    """The root's own block stays where it is: nothing of it is read or written."""
    n, root = 3, 1
    single, multi = side(sname), side(mname)
    if kind == SCATTER and sname == "b16s48":
        single, multi = multi, single               # the same pair, strided on the root's side
    mc, md = _even(n, 576 // multi.size)
    _run(kind, n, root, single, multi, [576 // single.size] * n, mc, md, seed=9, inplace=True,
         what=f"in place {kind} {sname} / {mname}")


# -- 6. declines ---------------------------------------------------------------------------------
DECLINED = [("struct2", "vec"), ("vec", "struct2"), ("twolevel", "vec"), ("vec", "twolevel"), ("bigblen", "flat"),
            ("flat", "bigblen"), ("vec", "negstride"), ("b2s4", "vec"), ("vec", "b2s4"), ("b2s4", "flat"),
            ("flat", "b2s4")]


@pytest.mark.parametrize("kind", [GATHER, SCATTER])
@pytest.mark.parametrize("sname,rname", DECLINED)
def test_declines_leave_buffers_untouched(ready, kind, sname, rname):
    """A two-run struct, a two-level layout, blocks above the limit, a
    non-monotonic receive layout and 2-byte blocks against a strided or a flat
    partner: MX_ERR_UNSUPPORTED, nothing written, nothing counted."""
    n, root = 2, 1
    S, R = side(sname), side(rname)
    single, multi = (S, R) if kind == GATHER else (R, S)
    stream = int(np.lcm(S.size, R.size))
    c1, (mc, md) = stream // single.size, _even(n, stream // multi.size)
    comm = mxompi.Comm.local(n)
    try:
        sing = [Buf(*span(single, [c1], [0])) for _ in range(n)]
        mult = [Buf(*span(multi, mc, md)) for _ in range(n)]
        before = comm.rooted_stats()
        sp, mp = [b.user for b in sing], [b.user for b in mult]
        with pytest.raises(mxompi.MxError) as e:
            if kind == GATHER:
                comm.gather_local(sp, c1, single.dt, mp, mc[0], multi.dt, root, _stream())
            else:
                comm.scatter_local(mp, mc[0], multi.dt, sp, c1, single.dt, root, _stream())
        assert e.value.rc == UNSUPPORTED
        torch.cuda.synchronize()
        for b in sing + mult:
            assert bool((b.dev == FILL).all())
        assert comm.rooted_stats() == before
    finally:
        comm.close()


@pytest.mark.parametrize("kind", [GATHER, SCATTER])
def test_root_out_of_range(ready, kind):
    n, F = 2, side("flat")
    comm = mxompi.Comm.local(n)
    try:
        bufs = [Buf(0, 64) for _ in range(2 * n)]
        sp, mp = [b.user for b in bufs[:n]], [b.user for b in bufs[n:]]
        before = comm.rooted_stats()
        for root in (n, -1):
            with pytest.raises(mxompi.MxError) as e:
                if kind == GATHER:
                    comm.gather_local(sp, 16, F.dt, mp, 16, F.dt, root, _stream())
                else:
                    comm.scatter_local(mp, 16, F.dt, sp, 16, F.dt, root, _stream())
            assert e.value.rc == ARG
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b.dev == FILL).all())
        assert comm.rooted_stats() == before
    finally:
        comm.close()


# -- 7. n = 1 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [GATHER, SCATTER])
def test_single_rank(ready, kind):
    """Size 1: the local form and the rank's own entry point are one job each
    on the caller's stream; in place nothing moves."""
    S, R = side("b24s40"), side("vec")
    single, multi = (S, R) if kind == GATHER else (R, S)
    _run(kind, 1, 0, single, multi, [12], [36], [2], seed=1, what=f"{kind} n=1")
    _run(kind, 1, 0, side("flat"), side("flat"), [77], [77], [3], seed=2, what=f"{kind} n=1 bytes", s_shift=1)
    _run(kind, 1, 0, single, multi, [12], [36], [2], seed=3, what=f"{kind} n=1 in place", inplace=True)
    comm = mxompi.Comm.local(1)
    try:
        rng = np.random.default_rng(4)
        sing = Buf(*span(single, [12], [0]), rng=rng if kind == GATHER else None)
        mult = Buf(*span(multi, [36], [2]), rng=None if kind == GATHER else rng)
        exp_s, exp_m = sing.host.copy(), mult.host.copy()
        move_block(kind, single, multi, 12, 36, 2, exp_s, sing.base, exp_m, mult.base)
        before = comm.rooted_stats()
        if kind == GATHER:
            comm.gatherv(sing.user, 12, single.dt, mult.user, [36], [2], multi.dt, 0, _stream())
        else:
            comm.scatterv(mult.user, [36], [2], multi.dt, sing.user, 12, single.dt, 0, _stream())
        torch.cuda.synchronize()
        assert sing.wrong(exp_s) is None and mult.wrong(exp_m) is None, (sing.wrong(exp_s), mult.wrong(exp_m))
        assert comm.rooted_stats()["calls"] == before["calls"] + 1
        with pytest.raises(mxompi.MxError) as e:
            comm.gather(sing.user, 12, single.dt, mult.user, 36, multi.dt, 1, _stream())
        assert e.value.rc == ARG
    finally:
        comm.close()
