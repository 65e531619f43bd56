"""Shared by the rooted exchange tests (gather, gatherv, scatter, scatterv): the
layouts -- the parameters tests/test_exchange_ddt_gpu.py uses --, device
buffers with padding around their span, and the numpy expectation.  Expected
bytes come from numpy index maps of the description trees (tests/ddt_gen.py),
never from the library."""
import numpy as np

import ddt_gen as G
import mxompi

FILL = 0xA5
PAD = 512          # bytes kept around every buffer's span (they must keep the fill)
ARG = -1
UNSUPPORTED = -2
GATHER, SCATTER = "gather", "scatter"


# name: (nodes, lb, extent); blen / stride / extent in bytes as the comments say
def _nodes(name):
    E = G.Elem
    return {
        "b4s8": ([E(4, 6, 1, 8, 0)], 0, 48),             # blen 4 / stride 8
        "vec": ([E(4, 3, 2, 20, 0)], 0, 48),             # blen 8 / stride 20 / extent 48 (the mini-host's VEC)
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

    def map(self, count, displ=0):
        """user offset of every stream byte of `count` instances `displ` extents in"""
        if self.lay is None:
            return np.arange(count, dtype=np.int64) + displ
        return self.lay.map_all(count) + displ * self.extent

    def unit(self):
        """the access unit of the layout alone (for 256-byte aligned buffers)"""
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


def span(sd, counts, displs):
    """[lo, hi) of the user offsets the blocks touch (0, 0 for none)"""
    lo, hi = 0, 0
    for c, d in zip(counts, displs):
        if c:
            m = sd.map(c, d)
            lo, hi = min(lo, int(m.min())), max(hi, int(m.max()) + 1)
    return lo, hi


def host_image(lo, hi, shift=0, rng=None):
    """(bytes, base): the host image of a buffer around [lo, hi); `base` is
    where the user pointer sits, `shift` bytes off a 256-byte boundary."""
    base = (PAD + (-lo + 255) // 256 * 256 if lo < 0 else PAD) + shift
    n = base + hi + PAD
    img = np.full(n, FILL, np.uint8) if rng is None else rng.integers(0, 256, n, dtype=np.uint8)
    return img, base


class Buf:
    """A device buffer around a span: `user` is the address the call gets."""

    def __init__(self, lo, hi, shift=0, rng=None):
        import torch
        self.host, self.base = host_image(lo, hi, shift, rng)
        self.n = self.host.size
        self.dev = torch.from_numpy(self.host.copy()).to("cuda:0")
        assert self.dev.data_ptr() % 256 == 0
        self.user = self.dev.data_ptr() + self.base

    def wrong(self, exp):
        """None, or where the device bytes differ from `exp`"""
        got = self.dev.cpu().numpy()
        bad = np.nonzero(got != exp)[0]
        if bad.size == 0:
            return None
        return (f"{bad.size} wrong bytes, first at user offset {bad[0] - self.base} "
                f"(got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


def block_len(single, multi, c1, mc):
    """stream bytes of a block: the sender's announcement cut at the receiver's room"""
    return min(c1 * single.size, mc * multi.size)


def move_block(kind, single, multi, c1, mc, md, s_img, s_base, m_img, m_base):
    """numpy: one block between a rank's single side and its place in the root's
    multi side (gather: single -> multi, scatter: multi -> single), in place"""
    ln = block_len(single, multi, c1, mc)
    if not ln:
        return
    sm = single.map(c1)[:ln] + s_base
    mm = multi.map(mc, md)[:ln] + m_base
    if kind == GATHER:
        m_img[mm] = s_img[sm]
    else:
        s_img[sm] = m_img[mm]
