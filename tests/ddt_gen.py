"""Seeded generator of derived-datatype descriptions for the convertor fuzz
(tests/test_convertor_fuzz.py).

Three things live here, none of which looks into the library:

* a record emitter: a description tree of `Elem` and `Loop` nodes becomes the
  committed-description bytes mx_ddt_create reads (ELEM / LOOP / END_LOOP
  records of 32 bytes, the layouts of RecElem / RecLoop in
  csrc/mx_ddt_layout.hip and of rec_elem / rec_loop in oracle/mx_oracle_ddt.c),
  nested loops included, closed by the final END_LOOP;
* an independent index map: a numpy walk of the same tree gives, for every
  packed byte of one instance, its user offset, so that
  `packed[b] = user[map[b]]`; size, true bounds and the map of `count`
  instances (`map + i * extent`) follow from it;
* `layout(seed, klass)` and `calls(seed, total, ...)`: the layouts and the
  (offset, length, pointer residue) call shapes of the fuzz, stratified over
  the seed so that a fixed seed list provably fills every property bin
  (`Layout.bins`, `call_bins`); the coverage test counts them.

Everything is a pure function of its arguments (numpy's PCG64 streams).
"""
import math
import struct

import numpy as np

F_DATA = 0x0100
T_LOOP, T_END_LOOP = 0, 1
# OPAL basic type ids of the 1/2/4/8/16-byte integers (opal_datatype_internal.h:50-80)
TYPE_OF_SIZE = {1: 4, 2: 5, 4: 6, 8: 7, 16: 8}
BASIC = np.array([0, 0, 0, 0, 1, 2, 4, 8, 16, 1, 2, 4, 8, 16, 2, 4, 8, 16, 16, 4, 8, 16, 32, 1, 4, 0], np.uint64)

CLASSES = ("pack_any", "unpack_safe", "vector_like")


class Elem:
    """`count` blocks of `blocklen` elements of `es` bytes at disp + j * extent."""

    def __init__(self, es, count, blocklen, extent, disp):
        self.es, self.count, self.blocklen, self.extent, self.disp = es, int(count), int(blocklen), int(extent), int(disp)

    @property
    def blk(self):
        return self.blocklen * self.es


class Loop:
    """`loops` repetitions of `body`, repetition l displaced by l * extent."""

    def __init__(self, loops, extent, body):
        self.loops, self.extent, self.body = int(loops), int(extent), list(body)


# ---- record emitter ----------------------------------------------------------
def _size(nodes):
    return sum(n.count * n.blk if isinstance(n, Elem) else n.loops * _size(n.body) for n in nodes)


def _emit(nodes, out):
    for n in nodes:
        if isinstance(n, Elem):
            out.append(struct.pack("<HHIQqq", F_DATA, TYPE_OF_SIZE[n.es], n.count, n.blocklen, n.extent, n.disp))
        else:
            body = []
            _emit(n.body, body)
            # items counts the body's records and the END_LOOP that closes them
            out.append(struct.pack("<HHIIIQq", 0, T_LOOP, len(body) + 1, n.loops, 0, 0, n.extent))
            out.extend(body)
            out.append(struct.pack("<HHIQqq", 0, T_END_LOOP, len(body) + 1, 0, _size(n.body), 0))


def emit(nodes):
    """(description bytes, record count) of a tree, with the final END_LOOP."""
    out = []
    _emit(nodes, out)
    out.append(struct.pack("<HHIQqq", 0, T_END_LOOP, len(out), 0, _size(nodes), 0))
    return b"".join(out), len(out)


# ---- independent index map -----------------------------------------------------
def index_map(nodes):
    """int64 user offset of every packed byte of one instance, in stream order."""
    parts = []
    for n in nodes:
        if isinstance(n, Elem):
            starts = n.disp + n.extent * np.arange(n.count, dtype=np.int64)
            parts.append((starts[:, None] + np.arange(n.blk, dtype=np.int64)[None, :]).ravel())
        else:
            body = index_map(n.body)
            parts.append((n.extent * np.arange(n.loops, dtype=np.int64)[:, None] + body[None, :]).ravel())
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def _shift(n, d):
    if isinstance(n, Elem):
        n.disp += int(d)
    else:
        for c in n.body:
            _shift(c, d)


def _depth(nodes):
    return max([0] + [1 + _depth(n.body) for n in nodes if isinstance(n, Loop)])


def _walk(nodes):
    for n in nodes:
        yield n
        if isinstance(n, Loop):
            yield from _walk(n.body)


def _contig(e):
    return e.count == 1 or e.extent == e.blk


def _run_bound(nodes):
    """Upper bound on flatten()'s run count: an ELEM is one run, a loop of a
    single ELEM is one run (cnt1 or cnt2), any other loop repeats its body's
    runs `loops` times (adjacent contiguous blocks may still merge)."""
    r = 0
    for n in nodes:
        if isinstance(n, Elem):
            r += 1
        elif len(n.body) == 1 and isinstance(n.body[0], Elem):
            r += 1
        else:
            r += n.loops * _run_bound(n.body)
    return r


class Layout:
    def __init__(self, nodes, lb, extent, count, seed=None, klass=None, note=""):
        self.nodes, self.seed, self.klass, self.note = nodes, seed, klass, note
        self.desc, self.nrec = emit(nodes)
        self.map = index_map(nodes)
        self.size = int(self.map.size)
        assert self.size == _size(nodes) and self.size > 0
        self.lb, self.ub, self.extent, self.count = int(lb), int(lb) + int(extent), int(extent), int(count)
        self.true_lb, self.true_ub = int(self.map.min()), int(self.map.max()) + 1
        self._all = {}

    def map_all(self, count=None):
        """user offset of every byte of the stream of `count` instances"""
        count = self.count if count is None else count
        if count not in self._all:
            inst = self.extent * np.arange(count, dtype=np.int64)
            self._all[count] = (inst[:, None] + self.map[None, :]).ravel()
        return self._all[count]

    def span(self, count=None):
        """[lo, hi) of the user offsets `count` instances touch"""
        count = self.count if count is None else count
        tail = (count - 1) * self.extent
        return self.true_lb + min(0, tail), self.true_ub + max(0, tail)

    @property
    def total(self):
        return self.size * self.count

    def overlap_free(self):
        m = self.map_all()
        return int(np.unique(m).size) == int(m.size)

    def aligned16(self):
        """one-run vectors, and layouts whose every block start, block length and extent is a multiple of 16"""
        if self.klass == "vector_like":
            return True
        cut = np.nonzero(np.diff(self.map) != 1)[0] + 1
        return not (np.any(self.map[cut] % 16) or np.any(cut % 16) or self.map[0] % 16 or self.size % 16 or
                    self.extent % 16)

    def block_interior(self):
        """stream positions p (of instance 0) with p - 1 and p in one contiguous user block"""
        return np.nonzero(np.diff(self.map) == 1)[0] + 1

    def bins(self):
        """The property bins this layout falls into (tree and map only)."""
        S, ext = self.size, self.extent
        m = self.map_all()
        mono = bool(np.all(np.diff(m) > 0)) if m.size > 1 else True
        elems = [n for n in _walk(self.nodes) if isinstance(n, Elem)]
        loops = [n for n in _walk(self.nodes) if isinstance(n, Loop)]
        single = [l.body[0] for l in loops if len(l.body) == 1 and isinstance(l.body[0], Elem)]
        rb, d = _run_bound(self.nodes), _depth(self.nodes)
        b = {
            "S%16==0": S % 16 == 0, "S%4==0,not16": S % 4 == 0 and S % 16 != 0, "S odd": S % 2 == 1,
            "S<=65535": S <= 65535, "S>65535": S > 65535,
            "span+ext<=65536": self.true_ub - self.true_lb + ext <= 65536,
            "span+ext>65536": self.true_ub - self.true_lb + ext > 65536,
            "ext<0": ext < 0, "ext==0": ext == 0, "sparse ext>4S": ext > 4 * S,
            "monotonic": mono, "shuffled": not mono,
            "instance in order, instances interleave or overlap": not mono and ext > 0 and bool(np.all(np.diff(self.map) > 0)),
            "negative inner stride": any(e.count > 1 and e.extent < 0 for e in elems) or
                                     any(l.loops > 1 and l.extent < 0 for l in loops),
            "depth1": d == 1, "depth2": d == 2, "depth>=3": d >= 3,
            "loop of contiguous ELEM": any(_contig(e) for e in single),
            "loop of strided ELEM": any(not _contig(e) for e in single),
            "runs<=64": rb <= 64, "runs65-512": 64 < rb <= 512, "runs>512": rb > 512,
        }
        for es in (1, 2, 4, 8, 16):
            b[f"es{es}"] = any(e.es == es for e in elems)
        return {k for k, v in b.items() if v}


# ---- generators ------------------------------------------------------------------
def _up(x, a):
    return -(-int(x) // a) * a


def _leaf(rng, k, strided=None):
    """One ELEM occupying the box [0, width): (node, width)."""
    es = int(rng.choice(k["es"]))
    a = max(k["align"], 1)
    b = int(rng.integers(16, 200)) if k["fat"] else int(rng.integers(1, 7))
    c = int(rng.choice([1, 2, 3, 5])) if strided is None else (int(rng.integers(2, 6)) if strided else 1)
    blk = b * es
    if k["overlap"]:
        stride = int(rng.integers(-2, 3)) * _up(blk, a) // 2 // a * a      # 0, +-half, +-whole block pitch
        e = Elem(es, c, b, stride, 0)
        return e, blk + (c - 1) * abs(stride)
    stride = _up(blk, a) + a * int(rng.integers(1 if strided else 0, 4))
    width = (c - 1) * stride + blk
    if c > 1 and rng.random() < k["neg"]:
        return Elem(es, c, b, -stride, (c - 1) * stride), width
    return Elem(es, c, b, stride, 0), width


def _loop(rng, k, depth, force=None):
    a = max(k["align"], 1)
    if force or depth <= 1 and rng.random() < 0.3:
        leaf, width = _leaf(rng, k, strided=(force == "strided") if force else None)
        body = [leaf]
    else:
        body, width = _box(rng, k, depth - 1)
    n = int(rng.integers(2, 5))
    if k["overlap"]:
        E = int(rng.integers(-2, 3)) * _up(width, a) // 2 // a * a
        return Loop(n, E, body), width + (n - 1) * abs(E)
    E = _up(width, a) + a * int(rng.integers(0, 3))
    if len(body) == 1 and isinstance(body[0], Elem) and _contig(body[0]) and E == body[0].count * body[0].blk:
        E += a                                  # keep the loop a strided one
    total = (n - 1) * E + width
    if rng.random() < k["neg"]:
        for c in body:
            _shift(c, (n - 1) * E)
        return Loop(n, -E, body), total
    return Loop(n, E, body), total


def _box(rng, k, depth, force=None, kids=None):
    """Children in address slots of one box, in a (maybe permuted) stream
    order: (nodes, width).  Slots are disjoint unless k['overlap']."""
    a = max(k["align"], 1)
    nk = int(rng.integers(1, 4)) if kids is None else kids
    made = []
    for i in range(nk):
        if depth > 0 and (i == 0 or rng.random() < 0.4):
            made.append(_loop(rng, k, depth if i == 0 else int(rng.integers(1, depth + 1)), force if i == 0 else None))
        else:
            made.append(_leaf(rng, k))
    pos = 0
    for node, w in made:
        if k["overlap"]:
            at = a * int(rng.integers(0, max(1, sum(x[1] for x in made) // a)))
            _shift(node, at)
            pos = max(pos, at + w)
        else:
            _shift(node, pos)
            pos = _up(pos + w, a) + a * int(rng.integers(1, 3))
    width = pos
    order = rng.permutation(nk) if k["shuffle"] else np.arange(nk)
    return [made[i][0] for i in order], width


# knobs of the tree recipes: element sizes, alignment of every offset, LOOP
# depth before scaling, size class, wanted residue of S, stream-order shuffle,
# probability of a negative inner stride, extent mode, forced single-ELEM loop
_K = dict(es=(1,), align=1, depth=0, sclass="small", sres=None, shuffle=False, neg=0.0, ext="tight", force=None,
          fat=False, wrap=None, kids=None, inorder=False)
RECIPES = [
    dict(_K, es=(1,), depth=0, sres="odd", shuffle=True, kids=3),
    dict(_K, es=(4,), align=4, depth=1, sres=4, force="contig", ext="gap"),
    dict(_K, es=(8,), align=8, depth=1, sres=16, force="strided"),
    dict(_K, es=(16,), align=16, depth=2, sres=16, ext="gap"),
    dict(_K, es=(2, 1), depth=3, shuffle=True, neg=0.5, ext="neg"),
    dict(_K, es=(1, 2), depth=2, sclass="medium", sres="odd", ext="sparse"),
    dict(_K, es=(4,), align=4, depth=1, sclass="big", sres=4),
    dict(_K, es=(8, 4), align=4, depth=0, sclass="big", fat=True, sres=16, kids=2),
    dict(_K, es=(4, 2), align=2, depth=0, sclass="medium", wrap=40, ext="negsparse", kids=3),
    dict(_K, es=(2,), align=2, depth=2, sclass="medium", ext="inter", neg=0.3, kids=2),
    dict(_K, es=(1, 4), depth=0, sclass="medium", wrap=300, sres="odd", kids=2),
    dict(_K, es=(16, 4), align=4, depth=1, neg=0.6, shuffle=True, ext="neg", sres=4, force="strided"),
    dict(_K, es=(8,), align=8, depth=0, sclass="medium", fat=True, kids=3, sres=16, ext="gap"),
    dict(_K, es=(2, 4), align=2, depth=3, sclass="medium", shuffle=True, neg=0.3, sres=4, ext="zero"),
    # every instance in address order, the instances interleaved (or, to send, overlapping)
    dict(_K, es=(4, 1), depth=1, sclass="medium", ext="inter", kids=2, inorder=True),
    dict(_K, es=(2,), align=2, depth=0, sclass="medium", ext="inter", kids=3, inorder=True),
]


def _fixup(rng, k, S):
    """A one-block ELEM whose size gives S + its size the wanted residue."""
    want = k["sres"]
    es = 1 if 1 in k["es"] else min(k["es"])
    for n in range(1, 65):
        s = S + n * es
        if want is None or (want == "odd" and s % 2) or (want == 4 and s % 4 == 0 and s % 16) or \
                (want == 16 and s % 16 == 0):
            return Elem(es, 1, n, n * es, 0), n * es
    raise AssertionError(f"no fix-up for residue {want} with {es}-byte elements")


def _tree_layout(seed, klass):
    rng = np.random.default_rng([seed, 1 + CLASSES.index(klass)])
    ri = seed % len(RECIPES)
    k = dict(RECIPES[ri])
    k["overlap"] = klass == "pack_any" and not k["inorder"]
    a = max(k["align"], 1)
    if seed >= 3 * len(RECIPES) and not k["inorder"]:              # later rounds keep the recipe's sizes and draw the rest
        k["shuffle"], k["neg"] = bool(rng.integers(0, 2)), float(rng.choice([0.0, 0.3, 0.6]))
        if k["ext"] != "inter" or rng.random() < 0.5:
            k["ext"] = str(rng.choice(["tight", "gap", "sparse", "neg", "negsparse"]))
        if k["sclass"] == "small":
            k["depth"] = int(rng.integers(0, 4))
    inter = k["ext"] == "inter" and klass != "pack_any"
    # to send: small in-order instances that overlap the next one (extent below the span), the byte map's size
    lapped = k["inorder"] and klass == "pack_any"
    nodes, width = _box(rng, k, k["depth"], k["force"], k["kids"])
    if inter and len(nodes) < 2:
        nodes, width = _box(rng, k, k["depth"], k["force"], 2)
    S0 = _size(nodes)
    if k["sclass"] != "small" or inter:
        target = int(rng.integers(70_000, 300_000)) if k["sclass"] == "big" else int(rng.integers(500, 4_500)) if lapped else \
            int(rng.integers(11_000 if inter else 6_000, 50_000))   # two interleaved instances still make 20 KiB
        n = k["wrap"] or max(2, -(-target // S0))
        if k["sclass"] != "big":
            n = max(2, min(n, 60_000 // S0))
        if k["overlap"]:
            E = int(rng.integers(-1, 3)) * _up(width, a) // 2 // a * a
        elif inter:
            E = 2 * _up(width, a)               # the odd half-slots are instance 1's
        else:
            E = _up(width, a) + a * int(rng.integers(0, 3))
        if n > 1:
            if not k["overlap"] and not inter and rng.random() < k["neg"]:
                for c in nodes:
                    _shift(c, (n - 1) * E)
                nodes = [Loop(n, -E, nodes)]
            else:
                nodes = [Loop(n, E, nodes)]
    if not inter:                               # a second top-level child: the residue of S, and >= 2 runs
        fx, fw = _fixup(rng, k, _size(nodes))
        m = index_map(nodes)
        hi = int(m.max()) + 1
        _shift(fx, int(rng.integers(0, hi)) // a * a if k["overlap"] else _up(hi, a) + a * int(rng.integers(1, 4)))
        nodes = nodes + [fx] if (not k["shuffle"] or rng.random() < 0.5) else [fx] + nodes
    if rng.random() < 0.4:                      # negative displacements: move the origin into the layout
        d0 = int(rng.integers(0, int(index_map(nodes).max()) + 1)) // a * a
        for c in nodes:
            _shift(c, -d0)
    m = index_map(nodes)
    S, W = int(m.size), int(m.max()) - int(m.min()) + 1
    if S > 65535:
        count = int(rng.integers(2, 5))
        while count > 2 and count * S > (2 << 20):
            count -= 1
    else:
        count = max(2, -(-int(rng.integers(20_000, 120_000)) // S))
    mode = k["ext"]
    if k["overlap"]:
        # anything legal to send: the extent may cut into the instance, vanish or point backwards
        mode = ("zero", "half", "neg", "negsmall", "tight", "sparse", "one")[int(rng.integers(0, 7))] \
            if mode not in ("zero",) else mode
    if lapped:
        mode = ("half", "one")[int(rng.integers(0, 2))]
    if mode == "inter":
        ext, count = _up(width, a), 2
    elif mode == "zero":
        ext = 0 if k["overlap"] else _up(W, a)
    elif mode == "half":
        ext = max(a, _up(W, a) // 2 // a * a)
    elif mode == "one":
        ext = a
    elif mode == "negsmall":
        ext = -max(a, _up(W, a) // 3 // a * a)
    elif mode == "tight":
        ext = _up(W, a)
    elif mode == "gap":
        ext = _up(W, a) + a * int(rng.integers(1, 9))
    elif mode == "sparse":
        ext = _up(max(W, 4 * S + 1), a) + a * int(rng.integers(0, 5))
    elif mode == "neg":
        ext = -(_up(W, a) + a * int(rng.integers(0, 9)))
    elif mode == "negsparse":
        ext = -(_up(max(W, 4 * S + 1), a) + a * int(rng.integers(0, 5)))
    else:
        raise AssertionError(mode)
    lb = int(rng.integers(-4, 5)) * a
    lay = Layout(nodes, lb, ext, count, seed, klass, f"recipe {ri} ext {mode}")
    if klass == "unpack_safe":
        # non-overlap is built in (disjoint slots, |extent| >= span or exact
        # interleave): asserted, never filtered
        assert lay.overlap_free(), f"unpack_safe seed {seed}: overlapping layout ({lay.note})"
    return lay


def _vector_layout(seed):
    """One ELEM or one LOOP of one ELEM."""
    rng = np.random.default_rng([seed, 1 + CLASSES.index("vector_like")])
    v, rnd = seed % 9, seed // 9
    es, b, stride, form, neg, ext_mode = 4, 1, 8, "elem", False, "resized"
    if v == 0:
        pass                                                    # 4-byte blocks every 8: the span kernel's domain
    elif v == 1:
        es, stride, ext_mode = 8, 16, "plain"                   # 8 every 16
    elif v == 2:
        stride, form = 16, "loop1"                              # 4 every 16, as a loop of one contiguous ELEM
    elif v == 3:
        b, stride, ext_mode = 2, 16, "plain"                    # 2 x 4 bytes every 16
    elif v == 4:
        b = int(rng.choice([3, 5, 6, 16, 33]))                  # other multiples of 4, stride backwards
        stride, neg = b * 4 + 4 * int(rng.integers(1, 9)), True
    elif v == 5:
        b, form = int(rng.choice([1, 2, 3, 7])), "loop2"        # a loop of one strided ELEM (two levels)
        stride, neg = b * 4 + 4 * int(rng.integers(1, 5)), rnd % 2 == 1
    elif v == 6:
        es, b = int(rng.choice([4, 8])), int(rng.choice([1, 2, 4]))
        stride, ext_mode = b * es + es * int(rng.integers(1, 4)), "neg"
    elif v == 7:
        es, b, neg = int(rng.choice([1, 2])), int(rng.choice([3, 5, 7])), rnd % 2 == 0
        stride, ext_mode = b * es + int(rng.integers(1, 9)), "plain"
    else:
        es, b = int(rng.choice([1, 4, 8])), int(rng.choice([1, 3, 16]))   # touching blocks: a contiguous type
        stride, form = b * es, ("elem", "loop1")[rnd % 2]
    blk = b * es
    big = rnd % 3 == 2 and v in (1, 4)                               # a few instances above 65535 bytes
    cnt = max(3, int(rng.integers(70_000, 200_000) if big else rng.integers(6_000, 50_000)) // blk)
    disp0 = int(rng.choice([0, 0, 16, -32, 4 if v >= 4 else 0]))
    single = rnd % 4 == 3 and v in (0, 1, 2, 3, 6)               # one block per instance: a resized basic type
    if single:
        cnt, form, ext_mode = 1, "elem", "neg" if ext_mode == "neg" else "resized"
    if form == "loop2":
        inner = int(rng.integers(2, 6))
        outer = max(2, cnt // inner)
        pitch = (inner - 1) * stride + blk + 4 * int(rng.integers(0, 4))
        e = Elem(es, inner, b, stride, disp0)
        nodes = [Loop(outer, -pitch, [e])] if neg else [Loop(outer, pitch, [e])]
        if neg:
            _shift(e, (outer - 1) * pitch)
        reach, period = (outer - 1) * pitch + (inner - 1) * stride + blk, outer * pitch
    else:
        sd, d = (-stride, disp0 + (cnt - 1) * stride) if neg else (stride, disp0)
        nodes = [Elem(es, cnt, b, sd, d)] if form == "elem" else [Loop(cnt, sd, [Elem(es, 1, b, blk, d)])]
        reach, period = (cnt - 1) * stride + blk, cnt * stride
    ext = {"resized": period, "plain": reach, "neg": -period}[ext_mode]
    S = _size(nodes)
    count = -(-int(rng.integers(20_000, 60_000)) // S) if single else \
        max(2, min(4, -(-int(rng.integers(20_000, 120_000)) // S)))
    lay = Layout(nodes, 0, ext, count, seed, "vector_like", f"vector {v} {form} {ext_mode}{' single' if single else ''}")
    assert lay.overlap_free(), f"vector_like seed {seed}: overlapping layout"
    return lay


def layout(seed, klass):
    """The layout of (seed, klass): klass one of CLASSES."""
    assert klass in CLASSES, klass
    return _vector_layout(seed) if klass == "vector_like" else _tree_layout(seed, klass)


# ---- call shapes -----------------------------------------------------------------------
SHAPES = ("whole", "len1", "short", "odd", "inblock", "inst0", "boundary", "misaligned", "frag")


def calls(seed, total, size=None, interior=None, aligned_bias=False):
    """Call shapes over a stream of `total` bytes (instances of `size`
    bytes; `interior`: stream positions of instance 0 inside a user block).
    Each is a dict: shape, offset, length, ures (user origin address mod 16),
    pdelta ((packed - offset) mod 16); "frag" also has `chunks`, the
    (offset, length) list that tiles the whole stream."""
    rng = np.random.default_rng([seed, 99])
    size = total if size is None else size
    ua, ub = seed % 16, (5 * seed + 3) % 16
    if aligned_bias:                       # the whole stream 16-byte aligned, every second seed its windows too
        ua, ub = 0, 0 if seed % 2 == 0 else ub
    out = []

    def add(shape, off, ln, ures, pdelta=0, **kw):
        off, ln = int(off), int(ln)
        assert 0 <= off and ln >= 1 and off + ln <= total, (shape, off, ln, total)
        out.append(dict(shape=shape, offset=off, length=ln, ures=ures, pdelta=pdelta, **kw))

    add("whole", 0, total, ua, 0 if seed % 3 or aligned_bias else int(rng.integers(1, 16)))
    add("len1", rng.integers(0, total), 1, ub)
    n = int(rng.integers(2, 16))
    add("short", rng.integers(0, total - n + 1), n, ub, int(rng.integers(0, 16)) if seed % 2 else 0)
    off = int(rng.integers(0, total // 2)) | 1
    ln = min(total - off, int(rng.integers(total // 8, total // 2 + 1)) | 1)
    add("odd", off, ln - (ln % 2 == 0), ub)
    if interior is not None and len(interior) >= 2:               # both ends cut a block
        inst = rng.integers(0, total // size, 2)
        p = np.sort(inst * size + rng.choice(interior, 2))
        if p[1] > p[0]:
            add("inblock", p[0], p[1] - p[0], ub)
    if size >= 2:
        o = int(rng.integers(0, size - 1))
        add("inst0", o, int(rng.integers(1, size - o + 1)), ub)
    if total > size:                                              # across the end of an instance
        kb = int(rng.integers(1, total // size)) * size
        lo, hi = int(rng.integers(1, min(kb, 9000) + 1)), int(rng.integers(1, min(total - kb, 9000) + 1))
        add("boundary", kb - lo, lo + hi, ub)
    off = int(rng.integers(0, total // 4 + 1))
    add("misaligned", off, max(1, (total - off) * 3 // 4), ub, int(rng.integers(1, 16)))
    chunks, p = [], 0
    while p < total:
        ln = min(total - p, int(rng.integers(1, 5001)))
        chunks.append((p, ln))
        p += ln
    add("frag", 0, total, ua, 0 if seed % 2 else int(rng.integers(1, 16)), chunks=chunks)
    return out


def calls_for(lay):
    return calls(lay.seed, lay.total, lay.size, lay.block_interior(), aligned_bias=lay.aligned16())


def call_bins(c):
    """The call-shape bins one call falls into."""
    b = {c["shape"], f"ures{c['ures']}"}
    b.add("packed-offset misaligned" if c["pdelta"] else "packed-offset aligned")
    if c["shape"] != "frag":
        b.add(f"packed%16=={(c['offset'] + c['pdelta']) % 16}")
        if c["offset"] % 2 and c["length"] % 2:
            b.add("odd offset and len")
    return b
