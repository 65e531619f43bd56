"""Differential fuzz of derived-datatype pack / unpack across the device
convertor's kernel families (csrc/mx_convertor.hip, convert<PACK>()).

The reference is tests/ddt_gen.py's index map -- a numpy walk of the
description tree giving the user offset of every packed byte, so
`packed[b] = user[map[b]]` -- not the oracle; the CPU tests here keep the
two honest with each other (oracle pack == gather, oracle unpack ==
scatter) and count that the fixed seed list fills every property and
call-shape bin, so a shifted random stream fails a test instead of thinning
the coverage.

The layouts are seeded description trees with nested LOOPs, negative
strides and displacements, zero and negative extents (`pack_any`),
non-overlapping by construction (`unpack_safe`), and one-run vectors
(`vector_like`); the calls are whole streams, 1-byte and sub-granule windows,
odd windows cutting blocks, windows inside instance 0 and across instance
ends, `packed - offset` off the 16-byte grid, every user-origin residue
mod 16, and a full fragmentation into chunks of 1..5000 bytes.

On a mismatch the message names seed, class, call shape, kernel family, the
first wrong stream byte (its instance, its offset in the instance, its user
offset) and both values; `ddt_gen.layout(seed, klass)` reproduces the case.
"""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ddt_gen as G
import mxompi
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = list(range(126))                # 7-8 x the 16 tree recipes (3 as written, then with drawn knobs), 14 x the 9 vector ones
CHUNKS = [SEEDS[i:i + 21] for i in range(0, len(SEEDS), 21)]
GUARD = 256


@functools.lru_cache(maxsize=None)
def _layout(klass, seed):
    return G.layout(seed, klass)


def _user_bytes(lay, tag):
    lo, hi = lay.span()
    return np.random.default_rng([lay.seed, tag]).integers(0, 256, hi - lo, dtype=np.uint8)


def _ids(v):
    return v if isinstance(v, str) else f"seeds{v[0]}-{v[-1]}"


# ---- CPU: the two references agree; the seed list fills the bins ------------------------
def _oracle_convert(lay, user, lo, packed, unpack):
    O = oracle_lib.oracle()
    vp, sz, i64, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int
    O.mxo_ddt_convert.argtypes = [vp, sz, vp, i64, i64, sz, vp, vp, ci]
    desc = np.frombuffer(lay.desc, np.uint8).copy()
    n = O.mxo_ddt_convert(desc.ctypes.data, lay.nrec, G.BASIC.ctypes.data, lay.lb, lay.ub, lay.count,
                          user.ctypes.data - lo, packed.ctypes.data, 1 if unpack else 0)
    assert n == lay.total


@pytest.mark.parametrize("seeds", CHUNKS, ids=_ids)
@pytest.mark.parametrize("klass", G.CLASSES)
def test_oracle_agrees_with_index_map(klass, seeds):
    """For every seed the GPU tests use: the oracle's packed stream is the
    index-map gather, and (non-overlapping layouts) its unpack into a
    prefilled buffer is the index-map scatter."""
    for seed in seeds:
        lay = _layout(klass, seed)
        lo, hi = lay.span()
        m = lay.map_all() - lo
        assert m.min() == 0 and m.max() == hi - lo - 1, (klass, seed)
        user = _user_bytes(lay, 7)
        got = np.zeros(lay.total, np.uint8)
        _oracle_convert(lay, user, lo, got, False)
        np.testing.assert_array_equal(got, user[m], err_msg=f"{klass} seed {seed} pack ({lay.note})")
        if klass != "pack_any":
            pre = _user_bytes(lay, 8)
            stream = np.random.default_rng([seed, 9]).integers(0, 256, lay.total, dtype=np.uint8)
            want = pre.copy()
            want[m] = stream
            _oracle_convert(lay, pre, lo, stream, True)
            np.testing.assert_array_equal(pre, want, err_msg=f"{klass} seed {seed} unpack ({lay.note})")
        lay._all.clear()


PROPERTY_BINS = ["S%16==0", "S%4==0,not16", "S odd", "S<=65535", "S>65535", "span+ext<=65536", "span+ext>65536",
                 "ext<0", "ext==0", "sparse ext>4S", "monotonic", "shuffled", "instance in order, instances interleave or overlap",
                 "negative inner stride",
                 "depth1", "depth2", "depth>=3", "loop of contiguous ELEM", "loop of strided ELEM",
                 "runs<=64", "runs65-512", "runs>512", "es1", "es2", "es4", "es8", "es16"]
CALL_BINS = list(G.SHAPES) + [f"ures{r}" for r in range(16)] + [f"packed%16=={r}" for r in range(16)] + \
    ["packed-offset misaligned", "packed-offset aligned", "odd offset and len"]


def _coverage():
    prop = {b: 0 for b in PROPERTY_BINS}
    unpack_prop = {b: 0 for b in PROPERTY_BINS}
    call = {b: 0 for b in CALL_BINS}
    for klass in G.CLASSES:
        for seed in SEEDS:
            lay = _layout(klass, seed)           # unpack_safe asserts non-overlap itself: nothing is discarded
            for b in lay.bins():
                prop[b] += 1
                if klass != "pack_any":
                    unpack_prop[b] += 1
            lay._all.clear()
            for c in G.calls_for(lay):
                for b in G.call_bins(c):
                    call[b] += 1
    return prop, unpack_prop, call


def test_seed_list_fills_every_bin():
    """Conditions, not measurements: over the fixed seed list every property
    bin and every call-shape bin holds at least 3 cases (ext == 0 for PACK
    only: an unpack of overlapping instances has no defined result), all 16
    user-origin residues occur, and every unpack_safe seed yields a layout."""
    prop, unpack_prop, call = _coverage()
    print("property bins:", json.dumps(prop))
    print("property bins (unpack layouts):", json.dumps(unpack_prop))
    print("call bins:", json.dumps(call))
    thin = {b: n for b, n in prop.items() if n < 3}
    thin.update({"unpack " + b: n for b, n in unpack_prop.items() if n < 3 and b != "ext==0"})
    thin.update({b: n for b, n in call.items() if n < 3})
    assert not thin, f"bins with fewer than 3 cases: {thin}"
    assert unpack_prop["ext==0"] == 0
    for klass in G.CLASSES:
        sizes = [_layout(klass, s).total for s in SEEDS]
        assert min(sizes) >= 20_000 and max(sizes) <= (2 << 20), (klass, min(sizes), max(sizes))
        assert all(_layout(klass, s).total <= 600 * 1024 for s in SEEDS if _layout(klass, s).size <= 65535)
    assert all(_layout(k, s).overlap_free() for k in ("unpack_safe", "vector_like") for s in SEEDS)
    for k in G.CLASSES:
        for s in SEEDS:
            _layout(k, s)._all.clear()


def test_emitter_records_nest():
    """LOOP items counts the body and its END_LOOP; a nested tree's records
    walk back to the tree's own map through the oracle (a hand-made case)."""
    inner = G.Loop(3, -16, [G.Elem(4, 2, 1, 8, 40), G.Elem(1, 1, 3, 3, 33)])
    lay = G.Layout([G.Loop(2, 100, [inner, G.Elem(2, 1, 2, 4, 60)])], 0, 200, 2, seed=0)
    assert lay.nrec == 8 and len(lay.desc) == 8 * 32 and lay.size == 2 * (3 * 11 + 4)
    assert list(lay.map[:11]) == [40, 41, 42, 43, 48, 49, 50, 51, 33, 34, 35]
    assert lay.map[11] == 24 and lay.map[33] == 60 and lay.map[37] == 140
    lo, hi = lay.span()
    user = np.arange(hi - lo, dtype=np.uint8)
    got = np.zeros(lay.total, np.uint8)
    _oracle_convert(lay, user, lo, got, False)
    np.testing.assert_array_equal(got, user[lay.map_all() - lo])


# ---- GPU ----------------------------------------------------------------------------------
torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


def _first_bad(lay, call, path, direction, k, exp, got):
    """The failure report for stream byte k (absolute position in the stream)."""
    inst, b = divmod(int(k), lay.size)
    uoff = int(lay.map[b]) + inst * lay.extent
    return (f"{direction} mismatch: seed {lay.seed} class {lay.klass} ({lay.note}; size {lay.size} extent {lay.extent} "
            f"count {lay.count}) call {call['shape']} offset {call['offset']} len {call['length']} ures {call['ures']} "
            f"pdelta {call['pdelta']} family {path}: stream byte {k} = instance {inst} + {b}, user offset {uoff}: "
            f"expected {exp} got {got}")


class _Dev:
    """One layout on the device: its datatype, user bytes per origin residue."""

    def __init__(self, lay, block=False):
        mxompi.init(0)
        self.lay = lay
        self.dt = mxompi.Datatype(lay.desc, lay.nrec, lay.size, lay.lb, lay.ub)
        self.st = torch.cuda.current_stream().cuda_stream
        self.lo, self.hi = lay.span()
        self.span = self.hi - self.lo
        self.m = lay.map_all() - self.lo
        self.paths = {}
        if block:
            self.dt.set_path("block")

    def close(self):
        self.dt.close()
        self.lay._all.clear()

    def _buf(self, host):
        t = torch.from_numpy(host).cuda()
        assert t.data_ptr() % 16 == 0
        return t

    def _chunks(self, c):
        return c["chunks"] if c["shape"] == "frag" else [(c["offset"], c["length"])]

    def pack(self, shapes=None):
        lay, dt = self.lay, self.dt
        user = _user_bytes(lay, 7)
        exp = user[self.m]
        ubufs = {}
        for c in G.calls_for(lay):
            if shapes and c["shape"] not in shapes:
                continue
            if c["ures"] not in ubufs:
                h = np.zeros(GUARD + 16 + self.span + GUARD, np.uint8)
                h[GUARD + c["ures"]:GUARD + c["ures"] + self.span] = user
                ubufs[c["ures"]] = self._buf(h)
            ubase = ubufs[c["ures"]].data_ptr() + GUARD + c["ures"] - self.lo
            off, ln = c["offset"], c["length"]
            at = GUARD + (off + c["pdelta"]) % 16          # where stream byte `off` lands: (packed - offset) % 16 == pdelta
            P = torch.zeros(at + ln + GUARD, dtype=torch.uint8, device="cuda")
            assert P.data_ptr() % 16 == 0
            for o, n in self._chunks(c):
                dt.pack(lay.count, ubase, P.data_ptr() + at + o - off, offset=o, length=n, stream=self.st)
            torch.cuda.synchronize()
            path = dt.last_path
            self.paths[("pack", c["shape"])] = path
            got = P.cpu().numpy()
            win = got[at:at + ln]
            if not np.array_equal(win, exp[off:off + ln]):
                k = int(np.nonzero(win != exp[off:off + ln])[0][0])
                raise AssertionError(_first_bad(lay, c, path, "pack", off + k, exp[off + k], win[k]))
            stray = np.nonzero(got[:at])[0].tolist() + (np.nonzero(got[at + ln:])[0] + at + ln).tolist()
            assert not stray, (f"pack wrote outside its window: seed {lay.seed} class {lay.klass} ({lay.note}) call "
                               f"{c['shape']} offset {off} len {ln} family {path}: buffer byte {stray[0] - at} "
                               f"relative to the window start = {got[stray[0]]}")

    def unpack(self, shapes=None):
        lay, dt = self.lay, self.dt
        pre = _user_bytes(lay, 8)
        stream = np.random.default_rng([lay.seed, 9]).integers(0, 256, lay.total, dtype=np.uint8)
        guard = np.random.default_rng([lay.seed, 10]).integers(0, 256, 2 * GUARD + 16, dtype=np.uint8)
        pbufs = {}
        for c in G.calls_for(lay):
            if shapes and c["shape"] not in shapes:
                continue
            if c["pdelta"] not in pbufs:                   # the stream at (address % 16) == pdelta
                h = np.full(GUARD + 16 + lay.total + GUARD, 0xA5, np.uint8)
                h[GUARD + c["pdelta"]:GUARD + c["pdelta"] + lay.total] = stream
                pbufs[c["pdelta"]] = self._buf(h)
            pbase = pbufs[c["pdelta"]].data_ptr() + GUARD + c["pdelta"]
            u0 = GUARD + c["ures"]
            h = np.empty(GUARD + 16 + self.span + GUARD, np.uint8)
            h[:u0] = guard[:u0]
            h[u0:u0 + self.span] = pre
            h[u0 + self.span:] = guard[u0:u0 + len(h) - u0 - self.span]
            D = self._buf(h)
            ubase = D.data_ptr() + u0 - self.lo
            off, ln = c["offset"], c["length"]
            for o, n in self._chunks(c):
                dt.unpack(lay.count, ubase, pbase + o, offset=o, length=n, stream=self.st)
            torch.cuda.synchronize()
            path = dt.last_path
            self.paths[("unpack", c["shape"])] = path
            want = h.copy()
            want[u0 + self.m[off:off + ln]] = stream[off:off + ln]
            got = D.cpu().numpy()
            if not np.array_equal(got, want):
                bad = int(np.nonzero(got != want)[0][0])
                hit = np.nonzero(self.m == bad - u0)[0]
                if bad < u0 or bad >= u0 + self.span:
                    where = f"guard byte {bad - u0} relative to the span start"
                elif not len(hit):
                    where = f"gap byte at user offset {bad - u0 + self.lo} (no stream byte maps there)"
                else:
                    raise AssertionError(_first_bad(lay, c, path, "unpack", int(hit[0]), want[bad], got[bad]))
                raise AssertionError(f"unpack wrote where it must not: seed {lay.seed} class {lay.klass} ({lay.note}) "
                                     f"call {c['shape']} offset {off} len {ln} ures {c['ures']} pdelta {c['pdelta']} "
                                     f"family {path}: {where}; expected {want[bad]} got {got[bad]}")


@gpu
@pytest.mark.parametrize("seeds", CHUNKS, ids=_ids)
@pytest.mark.parametrize("klass", G.CLASSES)
def test_pack_matches_index_map(klass, seeds):
    """Every call shape of every layout: the window holds
    user[map_all][offset:offset+len] and every other byte of the zeroed
    buffer, the 256-byte guards included, is still zero; the fragmented
    stream is compared assembled."""
    for seed in seeds:
        d = _Dev(_layout(klass, seed))
        d.pack()
        d.close()


@gpu
@pytest.mark.parametrize("seeds", CHUNKS, ids=_ids)
@pytest.mark.parametrize("klass", ["unpack_safe", "vector_like"])
def test_unpack_matches_index_map(klass, seeds):
    """Unpack into a random prefill between random guards: the whole buffer
    equals the prefill with prefill[map_all[offset:offset+len]] = the packed
    bytes (gap bytes and guards untouched); whole, windowed, fragmented."""
    for seed in seeds:
        d = _Dev(_layout(klass, seed))
        d.unpack()
        d.close()


BLOCK_SHAPES = ("whole", "odd", "boundary", "misaligned", "frag")


@gpu
@pytest.mark.parametrize("seeds", CHUNKS, ids=_ids)
@pytest.mark.parametrize("klass", G.CLASSES)
def test_forced_block_path_matches(klass, seeds):
    """The same layouts through dt.set_path("block"), both directions.  The
    block table needs a positive extent (blk_tab): a zero or negative one is
    refused with MX_ERR_UNSUPPORTED and the datatype stays on its own path."""
    for seed in seeds:
        lay = _layout(klass, seed)
        if lay.extent <= 0:
            dt = mxompi.Datatype(lay.desc, lay.nrec, lay.size, lay.lb, lay.ub)
            with pytest.raises(mxompi.MxError):
                dt.set_path("block")
            dt.close()
            continue
        d = _Dev(lay, block=True)
        d.pack(BLOCK_SHAPES)
        if klass != "pack_any":
            d.unpack(BLOCK_SHAPES)
        want = {"copy"} if lay.size == lay.extent and np.all(np.diff(lay.map) == 1) else {"block"}
        assert set(d.paths.values()) == want, (seed, klass, d.paths)
        d.close()


def _gcd(*v):
    g = 0
    for x in v:
        g = math.gcd(g, abs(int(x)))
    return g


def _negative_extent_unpack_family(lay, c):
    """What convert<false>() gives an extent < 0: never the copy (extent ==
    size > 0), no block table and no byte map (both need extent > 0), so: the
    VEC kernel for one strided run of aligned words (unit u % 4 == 0, u != 16),
    the granule kernel when every piece is 16-byte aligned (u == 16), else the
    tile kernel.  u = gcd(layout gcd, user % 16, offset % 16, len % 16 and,
    off the 16-byte grid, packed % 16).  Returns the set the call may take:
    one family wherever u is known from the tree."""
    res = [16, c["ures"] or 16, c["offset"] % 16 or 16, c["length"] % 16 or 16, (c["offset"] + c["pdelta"]) % 16 or 16]
    if lay.klass == "vector_like" and isinstance(lay.nodes[0], G.Elem):
        e = lay.nodes[0]
        u = _gcd(e.disp or 16, e.blk, e.extent if e.count > 1 else 16, lay.extent, *res)
        return {"vector"} if u % 4 == 0 and u != 16 else {"granule"} if u == 16 else {"tile"}
    if lay.klass == "vector_like":
        return {"vector", "granule", "tile"}
    # two or more runs (the trees end in a separate fix-up ELEM): u divides gcd(extent, S, residues)
    return {"tile"} if _gcd(lay.extent, lay.size, *res) % 16 else {"tile", "granule"}


PACK_FAMILIES = {"copy", "vector", "granule", "bytemap", "piece", "block"}
UNPACK_FAMILIES = {"copy", "vector", "granule", "piece", "block", "tile"}
PATH_SHAPES = ("whole", "odd", "misaligned")


@gpu
def test_default_dispatch_reaches_the_families():
    """Its own run over the fixed seed list (whole, odd and misaligned calls),
    so the result does not depend on which other tests ran: with default
    switches PACK reaches copy, vector, granule, byte map, piece and block and
    UNPACK copy, vector, granule, piece, block and tile, and every extent < 0
    UNPACK takes the family convert<false>() gives it.

    The tile PACK kernels are not reachable with default switches: they come
    after the block table (taken by every instance > 65535 bytes with
    extent > 0) and the byte map / piece table (every instance <= 65535 bytes
    with extent > 0 has a byte map, and 256 pieces of <= 16 bytes always fit
    the piece kernel's 16 KiB stage), and extent <= 0 is never monotonic; see
    test_tile_pack_and_switched_off_families for their run with MX_CONV_BMAP=0
    and MX_CONV_BLK=0."""
    seen = {"pack": {}, "unpack": {}}
    neg = 0
    for klass in G.CLASSES:
        for seed in SEEDS:
            lay = _layout(klass, seed)
            d = _Dev(lay)
            d.pack(PATH_SHAPES)
            if klass != "pack_any":
                d.unpack(PATH_SHAPES)
                if lay.extent < 0:
                    for c in G.calls_for(lay):
                        if c["shape"] in PATH_SHAPES:
                            want = _negative_extent_unpack_family(lay, c)
                            got = d.paths[("unpack", c["shape"])]
                            assert got in want, (klass, seed, c["shape"], got, want)
                            neg += len(want) == 1
            for (direction, shape), path in d.paths.items():
                seen[direction].setdefault(path, []).append(f"{klass}:{seed}:{shape}")
            d.close()
    print("families:", json.dumps({k: {p: len(v) for p, v in s.items()} for k, s in seen.items()}))
    assert PACK_FAMILIES <= set(seen["pack"]), {p: len(v) for p, v in seen["pack"].items()}
    assert UNPACK_FAMILIES <= set(seen["unpack"]), {p: len(v) for p, v in seen["unpack"].items()}
    assert "tile" not in seen["pack"], seen["pack"]["tile"][:5]
    assert neg >= 9, f"only {neg} extent < 0 unpack calls with a single expected family"


# ---- families behind the A/B switches: one child process per switch -----------------------
CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1] + "/zhpe-ompi_amd"); sys.path.insert(0, sys.argv[1] + "/tests")
import test_convertor_fuzz as T
sys.exit(T.child_main())
"""
CHILD_SEEDS = list(range(16))           # one seed per tree recipe


def child_main():
    seen = {"pack": set(), "unpack": set()}
    try:
        for klass in ("unpack_safe", "pack_any"):
            for seed in CHILD_SEEDS:
                d = _Dev(_layout(klass, seed))
                d.pack()
                if klass == "unpack_safe":
                    d.unpack()
                for (direction, _), path in d.paths.items():
                    seen[direction].add(path)
                d.close()
    except AssertionError as e:
        print("FAIL", e)
        return 1
    print("FAMILIES", json.dumps({k: sorted(v) for k, v in seen.items()}))
    return 0


SWITCHES = {
    # no byte map / piece kernels: monotonic small instances PACK through the pipelined tile kernel
    "MX_CONV_BMAP=0": dict(pack_has={"tile"}, never={"bytemap", "piece"}),
    # ... and through the one-tile-per-workgroup kernel
    "MX_CONV_BMAP=0 MX_CONV_PIPE=0": dict(pack_has={"tile"}, never={"bytemap", "piece"}),
    # no block kernels: instances > 65535 bytes take the tile (monotonic PACK, UNPACK) and granule kernels
    "MX_CONV_BLK=0": dict(pack_has={"tile", "granule"}, never={"block"}),
}


@gpu
def test_tile_pack_and_switched_off_families():
    """The tile PACK kernels (pipelined and one tile per workgroup), which no
    layout reaches with default switches, and the large instances without the
    block kernels: the tree seeds of one recipe each, every call shape, in one
    child process per switch (the switches are read once per process), run
    side by side."""
    procs = []
    for env in SWITCHES:
        e = dict(os.environ)
        e.update(kv.split("=") for kv in env.split())
        procs.append((env, subprocess.Popen([sys.executable, "-c", CHILD, ROOT], stdout=subprocess.PIPE,
                                            stderr=subprocess.PIPE, text=True, env=e)))
    failed = []
    for env, p in procs:
        try:
            out, err = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            p.kill()
            out, err = p.communicate()
        fam = [l for l in out.splitlines() if l.startswith("FAMILIES ")]
        if p.returncode != 0 or not fam:
            failed.append((env, p.returncode, out[-2000:], err[-2000:]))
            continue
        seen = json.loads(fam[-1][len("FAMILIES "):])
        w = SWITCHES[env]
        if not w["pack_has"] <= set(seen["pack"]) or w["never"] & (set(seen["pack"]) | set(seen["unpack"])):
            failed.append((env, "families", seen))
    assert not failed, failed
