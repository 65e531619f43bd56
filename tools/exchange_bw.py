#!/usr/bin/env python3
"""Call rates of the exchange kernel on a local communicator (8 ranks on one
GPU), against the existing copy kernel in the same run.

Per pair size S (4 KiB ... 32 MiB) four calls are timed:
  (a) alltoall_local, every buffer 16-byte aligned
  (b) alltoallv_local with S-byte pairs whose sources sit 4 bytes off their
      destinations' alignment (the dword-shift path)
  (c) alltoallv_local with pair sizes spread 1 : 64 around S
  (d) allgather_local of S bytes per rank: the same n*n*S bytes through
      k_copy, the yardstick
Times are host-clock medians of blocking calls (each ends in a stream
synchronise), so small sizes measure launch and synchronise cost.  GB/s is
read + write traffic (2 x payload) over call time; the share is of the
6.29 TB/s float4 copy rate measured for this part.

    python tools/exchange_bw.py [--out profiles/r07/exchange_local.txt]

--ddt times the strided exchange instead (profiles/r08/exchange_ddt_local.txt):
per shape and pair size, on the same bytes,
  (f) alltoall_ddt_local: the fused kernel, sender's layout to receiver's
  (p) Datatype.pack on every rank -> alltoall_local -> Datatype.unpack on
      every rank: the three-launch composition through packed buffers
  (k) allgather_local of the packed bytes: k_copy, the yardstick
Shapes: 16-byte words (blen 64 / stride 128 on both sides), 8-byte words
(blen 8 / stride 16 on both sides), and a 4-byte element transpose (blen 4 /
stride 8 sent, flat received).  GB/s counts the payload read and written once.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhpe-ompi_amd"))

COPY_RATE = 6.29e12
N = 8


def _time(fn, payload):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    est = max(time.perf_counter() - t0, 1e-6)
    reps = int(min(200, max(7, 0.3 / est)))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    t = statistics.median(ts)
    return t, 2 * payload / t / 1e9


def _vector(es, count, blocklen, stride_bytes):
    """mxompi.Datatype of `count` blocks of `blocklen` elements of `es` bytes
    every stride_bytes; the extent continues the period."""
    import struct
    import mxompi
    size = count * blocklen * es
    desc = struct.pack("<HHIQqq", 0x0100, {4: 6, 8: 7, 16: 8}[es], count, blocklen, stride_bytes, 0) + \
        struct.pack("<HHIQqq", 0, 1, 1, 0, size, 0)
    return mxompi.Datatype(desc, 2, size, 0, count * stride_bytes)


def ddt_leg(out):
    import torch
    import mxompi
    mxompi.init(0)
    comm = mxompi.Comm.local(N)
    st = torch.cuda.current_stream().cuda_stream
    shapes = [("W16 blen 64/stride 128", _vector(16, 8, 4, 128), _vector(16, 8, 4, 128)),
              ("W8  blen 8/stride 16", _vector(8, 64, 1, 16), _vector(8, 64, 1, 16)),
              ("W4  blen 4/stride 8 -> flat", _vector(4, 128, 1, 8), None)]
    lines = [f"# exchange_bw --ddt: local communicator, n = {N}, {torch.cuda.get_device_name(0)}",
             "# GB/s = 2 x payload / median call time (host clock, every case ends in a synchronise); "
             "share = of 6.29 TB/s (float4 copy)",
             f"{'pair':>10} {'shape':<28} {'case':<30} {'payload MiB':>12} {'us':>10} {'GB/s':>9} {'vs (p)':>7} {'share':>6}"]
    for S in (256 << 10, 32 << 20):
        for name, sdt, rdt in shapes:
            scount = S // sdt.size
            rcount = S // rdt.size if rdt else S
            sspan, rspan = N * scount * sdt.extent, N * rcount * (rdt.extent if rdt else 1)
            sb = [torch.empty(sspan + 64, dtype=torch.uint8, device="cuda").random_(0, 256) for _ in range(N)]
            rb = [torch.empty(rspan + 64, dtype=torch.uint8, device="cuda").zero_() for _ in range(N)]
            rb2 = [torch.empty(rspan + 64, dtype=torch.uint8, device="cuda").zero_() for _ in range(N)]
            ps = [torch.empty(N * S, dtype=torch.uint8, device="cuda") for _ in range(N)]
            pr = [torch.empty(N * S, dtype=torch.uint8, device="cuda") for _ in range(N)]
            sp, rp, rp2 = (mxompi._ptrs([t.data_ptr() for t in b]) for b in (sb, rb, rb2))
            pp, qp = mxompi._ptrs([t.data_ptr() for t in ps]), mxompi._ptrs([t.data_ptr() for t in pr])

            def fused():
                comm.alltoall_ddt_local(sp, scount, sdt, rp, rcount, rdt, st)

            def composed():
                for i in range(N):
                    sdt.pack(N * scount, sb[i].data_ptr(), ps[i].data_ptr(), stream=st)
                comm.alltoall_local(pp, qp, S, st)
                if rdt:   # (a flat receive side: the exchanged bytes are the result)
                    for i in range(N):
                        rdt.unpack(N * rcount, rb2[i].data_ptr(), pr[i].data_ptr(), stream=st)
                torch.cuda.synchronize()

            def kcopy():
                comm.allgather_local(pp, qp, S, st)

            ref = None
            for case, fn in (("(p) pack+alltoall+unpack", composed), ("(f) alltoall_ddt_local fused", fused),
                             ("(k) allgather_local (k_copy)", kcopy)):
                t, gbs = _time(fn, N * N * S)
                ref = ref or gbs
                lines.append(f"{S:>10} {name:<28} {case:<30} {N * N * S / 2**20:>12.2f} {t * 1e6:>10.1f} {gbs:>9.1f} "
                             f"{gbs / ref:>7.2f} {100 * gbs * 1e9 / COPY_RATE:>5.1f}%")
            fused()
            composed()
            for i in range(N):   # both routes moved the same bytes
                assert torch.equal(rb[i], rb2[i]) if rdt else torch.equal(rb[i][:N * S], pr[i]), "fused != composed"
            del sb, rb, rb2, ps, pr
            torch.cuda.empty_cache()
    comm.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


def rooted_leg(out):
    import torch
    import mxompi
    mxompi.init(0)
    comm = mxompi.Comm.local(N)
    st = torch.cuda.current_stream().cuda_stream
    # (name, the ranks' side, the root's side): flat, and the three shapes of --ddt
    shapes = [("flat", None, None),
              ("W16 blen 64/stride 128", _vector(16, 8, 4, 128), _vector(16, 8, 4, 128)),
              ("W8  blen 8/stride 16", _vector(8, 64, 1, 16), _vector(8, 64, 1, 16)),
              ("W4  blen 4/stride 8 -> flat", _vector(4, 128, 1, 8), None)]
    lines = [f"# exchange_bw --rooted: local communicator, n = {N}, root 0, {torch.cuda.get_device_name(0)}",
             "# a gather / scatter moves n blocks; (k) allgather_local of block/n bytes per rank moves the same n x block",
             "# bytes through k_copy; (a) the alltoall of the same shape moves n x n blocks",
             "# GB/s = 2 x payload / median call time (host clock, blocking calls); vs (k), vs (a): ratios of GB/s",
             f"{'block':>10} {'shape':<28} {'case':<26} {'payload MiB':>12} {'us':>10} {'GB/s':>9} {'vs (k)':>7} {'vs (a)':>7}"]
    for S in (4 << 10, 32 << 10, 256 << 10, 2 << 20, 16 << 20, 32 << 20):
        for name, one, many in shapes:
            # W4: the strided side sends (the ranks of a gather, the root of a scatter), the flat side receives
            c1 = S // one.size if one else S
            cm = S // many.size if many else S
            span1 = c1 * (one.extent if one else 1)
            spanm = N * cm * (many.extent if many else 1)
            tr = name.startswith("W4")
            sing = [torch.empty(span1 + 64, dtype=torch.uint8, device="cuda").random_(0, 256) for _ in range(N)]
            mult = [torch.empty((N * span1 if tr else spanm) + 64, dtype=torch.uint8, device="cuda").random_(0, 256)]
            flatm = [torch.empty(N * S + 64, dtype=torch.uint8, device="cuda").zero_()]
            flat1 = [torch.empty(S + 64, dtype=torch.uint8, device="cuda").zero_() for _ in range(N)]
            a2a_s = [torch.empty(spanm if many else N * span1 + 64, dtype=torch.uint8, device="cuda") for _ in range(N)]
            a2a_r = [torch.empty(spanm + 64 if many else N * S + 64, dtype=torch.uint8, device="cuda") for _ in range(N)]
            kc_s = [torch.empty(S // N, dtype=torch.uint8, device="cuda") for _ in range(N)]
            kc_r = [torch.empty(S, dtype=torch.uint8, device="cuda") for _ in range(N)]
            P = lambda ts: mxompi._ptrs([t.data_ptr() for t in ts])   # noqa: E731
            rest = [0] * (N - 1)
            sp, fp1, kp, kq, ap, aq = P(sing), P(flat1), P(kc_s), P(kc_r), P(a2a_s), P(a2a_r)
            mp, fpm = mxompi._ptrs([mult[0].data_ptr()] + rest), mxompi._ptrs([flatm[0].data_ptr()] + rest)
            if tr:
                # gather: strided ranks -> flat root; scatter: strided root (n blocks of the ranks' type) -> flat ranks
                g = lambda: comm.gather_local(sp, c1, one, fpm, S, None, 0, st)          # noqa: E731
                s = lambda: comm.scatter_local(mp, c1, one, fp1, S, None, 0, st)         # noqa: E731
                a = lambda: comm.alltoall_ddt_local(ap, c1, one, aq, S, None, st)        # noqa: E731
            elif one is None:
                g = lambda: comm.gather_local(sp, S, None, fpm, S, None, 0, st)          # noqa: E731
                s = lambda: comm.scatter_local(fpm, S, None, sp, S, None, 0, st)         # noqa: E731
                a = lambda: comm.alltoall_local(ap, aq, S, st)                           # noqa: E731
            else:
                g = lambda: comm.gather_local(sp, c1, one, mp, cm, many, 0, st)          # noqa: E731
                s = lambda: comm.scatter_local(mp, cm, many, sp, c1, one, 0, st)         # noqa: E731
                a = lambda: comm.alltoall_ddt_local(ap, cm, many, aq, cm, many, st)      # noqa: E731
            k = lambda: comm.allgather_local(kp, kq, S // N, st)                         # noqa: E731
            res = {}
            for case, fn, payload in (("(k) allgather_local (k_copy)", k, N * S), ("(a) alltoall, same shape", a, N * N * S),
                                      ("(g) gather_local", g, N * S), ("(s) scatter_local", s, N * S)):
                t, gbs = _time(fn, payload)
                res[case[:3]] = gbs
                lines.append(f"{S:>10} {name:<28} {case:<26} {payload / 2**20:>12.2f} {t * 1e6:>10.1f} {gbs:>9.1f} "
                             f"{gbs / res['(k)']:>7.2f} {gbs / res.get('(a)', gbs):>7.2f}")
            del sing, mult, flatm, flat1, a2a_s, a2a_r, kc_s, kc_r
            torch.cuda.empty_cache()
    comm.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ddt", action="store_true", help="time the strided exchange against its composition")
    ap.add_argument("--rooted", action="store_true", help="time gather and scatter beside k_copy and the alltoall")
    args = ap.parse_args()
    if args.rooted:
        import torch
        if not torch.cuda.is_available():
            sys.exit("exchange_bw: no GPU")
        return rooted_leg(args.out)
    if args.ddt:
        import torch
        if not torch.cuda.is_available():
            sys.exit("exchange_bw: no GPU")
        return ddt_leg(args.out)
    import torch
    import mxompi
    if not torch.cuda.is_available():
        sys.exit("exchange_bw: no GPU")
    mxompi.init(0)
    comm = mxompi.Comm.local(N)
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# exchange_bw: local communicator, n = {N}, {torch.cuda.get_device_name(0)}",
             "# GB/s = 2 x payload / median call time (host clock, blocking calls); "
             "share = of 6.29 TB/s (float4 copy)",
             f"{'pair':>10} {'case':<28} {'payload MiB':>12} {'us':>10} {'GB/s':>9} {'vs (d)':>7} {'share':>6}"]
    sizes = [4 << 10, 32 << 10, 256 << 10, 2 << 20, 16 << 20, 32 << 20]
    for S in sizes:
        spread = [[max(16, (S >> 3) << ((i + j) % 7)) for j in range(N)] for i in range(N)]   # S/8 ... 8S
        span = max(N * S, max(sum(r) for r in spread),
                   max(sum(spread[i][j] for i in range(N)) for j in range(N))) + 64
        sb = [torch.empty(span, dtype=torch.uint8, device="cuda").random_(0, 256) for _ in range(N)]
        rb = [torch.empty(span, dtype=torch.uint8, device="cuda") for _ in range(N)]
        # tables and pointer arrays are converted once: the timed calls are the library's
        sp, rp = mxompi._ptrs([t.data_ptr() for t in sb]), mxompi._ptrs([t.data_ptr() for t in rb])
        eq = [S] * (N * N)
        off = [j * S for _ in range(N) for j in range(N)]
        off4 = [j * S + 4 for _ in range(N) for j in range(N)]
        vs = [v for r in spread for v in r]
        vso = [sum(spread[i][:j]) for i in range(N) for j in range(N)]
        vr = [spread[i][j] for j in range(N) for i in range(N)]
        vro = [sum(spread[k][j] for k in range(i)) for j in range(N) for i in range(N)]
        ceq, coff, coff4 = mxompi._sizes(eq), mxompi._sizes(off), mxompi._sizes(off4)
        cvs, cvso, cvr, cvro = mxompi._sizes(vs), mxompi._sizes(vso), mxompi._sizes(vr), mxompi._sizes(vro)
        cases = [
            ("(d) allgather_local (k_copy)", lambda: comm.allgather_local(sp, rp, S, st), N * N * S),
            ("(a) alltoall aligned", lambda: comm.alltoall_local(sp, rp, S, st), N * N * S),
            ("(b) alltoall src +4 bytes", lambda: comm.alltoallv_local(sp, ceq, coff4, rp, ceq, coff, st), N * N * S),
            ("(c) alltoallv 1:64 spread", lambda: comm.alltoallv_local(sp, cvs, cvso, rp, cvr, cvro, st), sum(vs)),
        ]
        ref = None
        for name, fn, payload in cases:
            t, gbs = _time(fn, payload)
            if ref is None:
                ref = gbs
            lines.append(f"{S:>10} {name:<28} {payload / 2**20:>12.2f} {t * 1e6:>10.1f} {gbs:>9.1f} "
                         f"{gbs / ref:>7.2f} {100 * gbs * 1e9 / COPY_RATE:>5.1f}%")
        # the timed calls moved the right bytes (the last one: the spread alltoallv)
        got = rb[1][vro[N + 0]:vro[N + 0] + spread[0][1]]
        want = sb[0][vso[1]:vso[1] + spread[0][1]]
        assert torch.equal(got, want), "alltoallv moved wrong bytes"
        del sb, rb
        torch.cuda.empty_cache()
    comm.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
