"""Speed of the binary16 op kernels against the kernels of equal element
bytes that were there before them.

In one process, at 1 GiB per buffer (the non-temporal instances), five
alternating repeats of each pair:

    SUM   UINT16_T         vs  SHORT_FLOAT
    MAX   UINT16_T         vs  SHORT_FLOAT
    PROD  C_FLOAT_COMPLEX  vs  C_SHORT_FLOAT_COMPLEX   (equal bytes)

One repeat is bench.py's headline method: warm-up launches, then one HIP
event pair around `steps` back-to-back mx_reduce2 launches on one stream;
the figure is the algorithmic 3 * bytes over the average launch time.  These
kernels are bound by memory, so the binary16 kernel passes when its median
rate is not below the yardstick's median by more than the spread (max - min)
of the yardstick's own five repeats.

usage: python tools/short_float_speed.py [--out FILE] [--steps K] [--warmup W]
Needs a GPU; exits 1 when a pair does not pass."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhpe-ompi_amd"))

NBYTES = 1 << 30
REPEATS = 5


def _rate(torch, mx, op, t, a, b, count, steps, warmup):
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    for _ in range(warmup):
        mx.reduce2(op, t, a.data_ptr(), b.data_ptr(), count, sp)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        mx.reduce2(op, t, a.data_ptr(), b.data_ptr(), count, sp)
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return 3.0 * NBYTES / (ms * 1e-3) / 1e12          # TB/s of algorithmic traffic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import mxompi as mx
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing measured")
    mx.init(0)
    g = torch.Generator(device="cuda").manual_seed(0x5EEDC0DE)
    # binary16 values in (-1, 1): the same bytes serve the 16-bit integer yardstick
    h = [torch.empty(NBYTES // 2, dtype=torch.float16, device="cuda") for _ in range(2)]
    f = [torch.empty(NBYTES // 4, dtype=torch.float32, device="cuda") for _ in range(2)]
    c = [torch.empty(NBYTES // 2, dtype=torch.float16, device="cuda") for _ in range(2)]
    for x in h:
        x.uniform_(-1, 1, generator=g)
    for x in f + c:                                    # complex components in [0.7, 1.4)
        x.uniform_(0.7, 1.4, generator=g)
    pairs = [("SUM", "UINT16_T", h, NBYTES // 2, "SUM", "SHORT_FLOAT", h, NBYTES // 2),
             ("MAX", "UINT16_T", h, NBYTES // 2, "MAX", "SHORT_FLOAT", h, NBYTES // 2),
             ("PROD", "C_FLOAT_COMPLEX", f, NBYTES // 8, "PROD", "C_SHORT_FLOAT_COMPLEX", c, NBYTES // 4)]
    rows, ok = [], True
    for op0, t0, b0, n0, op1, t1, b1, n1 in pairs:
        base, new = [], []
        for _ in range(REPEATS):                       # alternating
            base.append(_rate(torch, mx, op0, t0, b0[0], b0[1], n0, args.steps, args.warmup))
            new.append(_rate(torch, mx, op1, t1, b1[0], b1[1], n1, args.steps, args.warmup))
        spread = max(base) - min(base)
        mb, mn = statistics.median(base), statistics.median(new)
        passed = mn >= mb - spread
        ok = ok and passed
        rows.append({"yardstick": f"{op0} {t0}", "binary16": f"{op1} {t1}",
                     "yardstick_tbps": [round(x, 3) for x in base], "binary16_tbps": [round(x, 3) for x in new],
                     "yardstick_median": round(mb, 3), "yardstick_spread": round(spread, 3),
                     "binary16_median": round(mn, 3), "pass": passed})
    res = {"bytes_per_buffer": NBYTES, "steps": args.steps, "warmup": args.warmup, "repeats": REPEATS,
           "unit": "TB/s, 3 * bytes per launch over the average launch time", "rows": rows, "pass": ok}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
