"""GPU: every (op, type) pair through every device consumer that instantiates it.

The library builds one kernel per (MPI_Op, datatype) pair for each of five
consumers; tests/test_reduce_gpu.py runs all 176 pairs through the op kernels
only.  Here every pair goes through the other four, on the adversarial
operands of op_values.edge_values, against the oracle (mxo_* of
oracle/mx_oracle_coll.c, mxo_reduce2 / mxo_reduce3).  No tolerances: bit for
bit, except that a floating-point SUM/PROD result that is NaN in the oracle
only has to be a NaN (golden_io.assert_op_equal); test_pair_matrix_host.py
shows that at most 10 % of those results are NaN and that the operands are
order- and role-sensitive.

  a. k_fold (test_fold_pair): allreduce ring / recursive doubling /
     Rabenseifner and a ragged reduce_scatter ring on 5 virtual ranks --
     16-byte aligned, every buffer one element off, rank 2's send buffer
     alone one element off (mixed misalignment: the element path), in place;
     receive buffers pre-filled with 0xA5 between 64-byte guards: guards and
     the padding bytes of padded types untouched.
  b. k_vm (test_vm_pair): rooted reduce (binomial, in-order binary), scan,
     exscan (rank 0's buffer keeps its fill), reduce_scatter_block on 5
     ranks, aligned and one element off; the 32-byte element types also on
     16 ranks (the VM fold's 160 KiB LDS opt-in).
  c. k_oneshot (test_oneshot_pairs): 2 and 3 processes sharing the GPU,
     every pair at one element, ~2 KiB (tagged words for 4- and 8-byte
     elements, raw otherwise) and ~12 KiB (several workgroups); at 2 ranks
     the resident collective service must have taken exactly the tagged-word
     calls it admits: 4- and 8-byte elements without padding bytes, up to
     4 KiB (MPI_SHORT_INT is 8 bytes with a 2-byte gap: the service's
     admission rule, CsvVisitor in csrc/mx_coll_svc.hip, sends it to the
     launch, where it still travels as tagged words).
  d. the resident reduce service (test_reduce_service_pairs): every golden
     record and every pair at 4099 elements of edge values (2- and 3-buffer
     form) through reduce2_sync / reduce3_sync on a side stream, read back without synchronisation; served
     exactly when 16 % element size == 0 and the type has no padding, exact
     on the launch path otherwise.
"""
import os

import numpy as np
import pytest

import golden_io
import mxompi
import op_values as ov
import oracle_lib
from test_coll_gpu import _free_port

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAIRS = ov.pairs()
_IDS = [f"{op}-{t}" for op, t in PAIRS]
FILL = ov.PREFILL
GUARD = 64
N = 5


@pytest.fixture(scope="module", autouse=True)
def _init():
    assert torch.cuda.is_available()
    mxompi.init(0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pad_mask(t, count):
    """Boolean mask of the non-data bytes of `count` elements (None: the type has none)."""
    slot = mxompi.TYPE[t]
    if slot not in golden_io._DATA_BYTES:
        return None
    es, keep = golden_io._DATA_BYTES[slot]
    m = np.ones(es, bool)
    m[keep] = False
    return np.tile(m, count)


class _Buf:
    """A device buffer of nbytes at `off` bytes past a 16-byte boundary,
    between guards, everything pre-filled with 0xA5 (or holding `data`)."""

    def __init__(self, nbytes, off=0, data=None):
        self.lo, self.nbytes = GUARD + off, nbytes
        host = np.full(self.lo + nbytes + GUARD, FILL, np.uint8)
        if data is not None:
            host[self.lo:self.lo + nbytes] = data
        self.t = torch.from_numpy(host).to("cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo

    def check(self, exp, op, t, what, pad_ref=None):
        """Guards untouched, data equal to the oracle's, padding bytes as
        they were (the fill, or pad_ref's bytes for an in-place call)."""
        host = self.t.cpu().numpy()
        got = host[self.lo:self.lo + self.nbytes]
        assert (host[:self.lo] == FILL).all() and (host[self.lo + self.nbytes:] == FILL).all(), f"{what}: guard written"
        golden_io.assert_coll_equal(got, exp, mxompi.OP[op], mxompi.TYPE[t], what)
        mask = _pad_mask(t, self.nbytes // mxompi.type_size(t))
        if mask is not None:
            ref = np.full(self.nbytes, FILL, np.uint8) if pad_ref is None else pad_ref
            np.testing.assert_array_equal(got[mask], ref[mask], err_msg=f"{what}: padding bytes written")

    def untouched(self, what):
        assert (self.t.cpu().numpy() == FILL).all(), f"{what}: written"


# ---------------------------------------------------------------------------
# a. k_fold
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("op,t", PAIRS, ids=_IDS)
def test_fold_pair(op, t):
    es = mxompi.type_size(t)
    comm = mxompi.Comm.local(N)
    st = _stream()
    for kind, alg, n, count, _ in ov.FOLD_CASES:
        exp = ov.expected(kind, alg, n, count, op, t)
        if kind == "reduce_scatter":
            rc = [count + 3 * r for r in range(n)]
            xs = ov.inputs(op, t, n, sum(rc))
            S = [_Buf(len(x), 0, x) for x in xs]
            R = [_Buf(c * es) for c in rc]
            comm.reduce_scatter_local([s.ptr for s in S], [r.ptr for r in R], rc, t, op, alg, st)
            for r in range(n):
                R[r].check(exp[r], op, t, f"reduce_scatter {alg} rc={rc} {op} {t} rank {r}")
            continue
        xs = ov.inputs(op, t, n, count)
        nb = count * es
        for mode in ("aligned", "offset", "mixed", "in_place"):
            what = f"allreduce {alg} count={count} {mode} {op} {t}"
            soff = [es if mode == "offset" or (mode == "mixed" and r == 2) else 0 for r in range(n)]
            roff = es if mode == "offset" else 0
            S = [_Buf(nb, soff[r], xs[r]) for r in range(n)]
            if mode == "in_place":
                comm.allreduce_local([mxompi.IN_PLACE] * n, [s.ptr for s in S], count, t, op, alg, st)
                for r in range(n):
                    S[r].check(exp[r], op, t, f"{what} rank {r}", pad_ref=xs[r])
            else:
                R = [_Buf(nb, roff) for _ in range(n)]
                comm.allreduce_local([s.ptr for s in S], [r.ptr for r in R], count, t, op, alg, st)
                for r in range(n):
                    R[r].check(exp[r], op, t, f"{what} rank {r}")
    comm.close()


# ---------------------------------------------------------------------------
# b. k_vm
# ---------------------------------------------------------------------------
def _vm_case(comm, kind, alg, n, count, root, op, t, off, st):
    es = mxompi.type_size(t)
    exp = ov.expected(kind, alg, n, count, op, t, root)
    what = f"{kind} {alg} n={n} count={count} off={off} {op} {t}"
    scount = count * n if kind == "reduce_scatter_block" else count
    xs = ov.inputs(op, t, n, scount)
    S = [_Buf(scount * es, off * es, x) for x in xs]
    R = [_Buf(count * es, off * es) for _ in range(n)]
    sp, rp = [s.ptr for s in S], [r.ptr for r in R]
    try:
        if kind == "reduce":
            comm.reduce_local(sp, [rp[r] if r == root else 0 for r in range(n)], count, t, op, root, alg, st)
        else:
            getattr(comm, kind + "_local")(sp, rp, count, t, op, alg, st)
    except mxompi.MxError as e:
        pytest.fail(f"{what}: {e}")
    for r in range(n):
        if (kind == "reduce" and r != root) or (kind == "exscan" and r == 0):
            R[r].untouched(f"{what} rank {r}")
        else:
            R[r].check(exp[r], op, t, f"{what} rank {r}")


@pytest.mark.parametrize("op,t", PAIRS, ids=_IDS)
def test_vm_pair(op, t):
    st = _stream()
    comm = mxompi.Comm.local(N)
    for kind, alg, n, count, root in ov.VM_CASES:
        for off in (0, 1):
            _vm_case(comm, kind, alg, n, count, root, op, t, off, st)
    comm.close()
    if (op, t) in ov.VM16_PAIRS:
        # 257 x 32 B x 16 ranks: past the 64 KiB LDS default, vm_launch opts in to 160 KiB
        comm = mxompi.Comm.local(16)
        for kind, alg, n, count, root in ov.VM16_CASES:
            _vm_case(comm, kind, alg, n, count, root, op, t, 0, st)
        comm.close()


# ---------------------------------------------------------------------------
# c. k_oneshot: raw and tagged words, launched and served
# ---------------------------------------------------------------------------
def _oneshot_worker(rank, n, port, q):
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

        comm = mxompi.Comm(rank, n, ag, device=0, staging_bytes=1 << 20)
        comm.set_timeout(30.0)
        # the worker pattern's ("path", ..., "one_shot") job: every call below takes the one-shot path
        comm.set_autotune(False)
        comm.set_oneshot_max(1 << 20)
        comm.set_reg_min(0)
        comm.set_protocol("auto")
        st = torch.cuda.current_stream().cuda_stream
        results = []
        for op, t in ov.pairs():
            es = mxompi.type_size(t)
            for count in ov.oneshot_counts(t):
                x = torch.from_numpy(ov.edge_values(op, t, count, ov.ONESHOT_BASE + rank)).to("cuda")
                out = torch.full((count * es,), FILL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                served = comm.stats()["service_calls"]
                comm.allreduce(x.data_ptr(), out.data_ptr(), count, t, op, "auto", st)
                got = out.cpu().numpy().tobytes()              # read right after the call
                results.append((got, comm.stats()["service_calls"] - served))
        comm.close()
        dist.destroy_process_group()
        q.put((rank, "ok", results))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc()))


def _spawn(n):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_oneshot_worker, args=(r, n, port, q)) for r in range(n)]
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


@pytest.mark.parametrize("n", [2, 3])
def test_oneshot_pairs(n):
    """n = 2: the collective service serves the tagged-word class; n = 3:
    more than two ranks per device, the same calls launch."""
    out = _spawn(n)
    bad, j = [], 0
    for op, t in PAIRS:
        es = mxompi.type_size(t)
        for count in ov.oneshot_counts(t):
            exp = ov.expected("allreduce", "auto", n, count, op, t, 0, ov.ONESHOT_BASE)
            admitted = n == 2 and es in (4, 8) and count * es <= 4096 and _pad_mask(t, 1) is None
            for r in range(n):
                got, served = out[r][j]
                try:
                    golden_io.assert_coll_equal(np.frombuffer(got, np.uint8), exp[r], mxompi.OP[op], mxompi.TYPE[t],
                                                f"one-shot n={n} {op} {t} count={count} rank {r}")
                except AssertionError as e:
                    bad.append(str(e).strip().splitlines()[-1] + f" [{op} {t} count={count} rank {r}]")
                if served != int(admitted):
                    bad.append(f"{op} {t} count={count} rank {r}: served {served}, expected {int(admitted)}")
            j += 1
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:40])


# ---------------------------------------------------------------------------
# d. the resident reduce service behind mx_reduce2_sync / mx_reduce3_sync
# ---------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to("cuda")


def test_reduce_service_pairs():
    O = oracle_lib.oracle()
    side = torch.cuda.Stream()
    mxompi.op_service_set(True)
    bad = []

    def run(kind, op, t, a, b, count, exp, what):
        """One call; the result read back on the default stream with no further synchronisation."""
        es = mxompi.type_size(t)
        A, B = _dev(a), _dev(b)
        C = torch.zeros_like(B) if kind == 3 else None
        assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        served0 = mxompi.op_service_stats()[1]
        if kind == 2:
            mxompi.reduce2_sync(op, t, A.data_ptr(), B.data_ptr(), count, side.cuda_stream)
            got = B.cpu().numpy()
        else:
            mxompi.reduce3_sync(op, t, A.data_ptr(), B.data_ptr(), C.data_ptr(), count, side.cuda_stream)
            got = C.cpu().numpy()
        served = mxompi.op_service_stats()[1] - served0
        mask = _pad_mask(t, count)
        want = int(16 % es == 0 and mask is None)
        if served != want:
            bad.append(f"{what}: served {served}, expected {want}")
        try:
            golden_io.assert_op_equal(got, exp, mxompi.OP[op], mxompi.TYPE[t], what)
            if mask is not None:    # padding: inout's own bytes (2-buffer), the zeroed destination's (3-buffer)
                ref = np.asarray(b) if kind == 2 else np.zeros(len(got), np.uint8)
                np.testing.assert_array_equal(got[mask], ref[mask], err_msg=f"{what}: padding bytes")
        except AssertionError as e:
            bad.append(f"{what}: " + str(e).strip().splitlines()[-1])

    for rec in golden_io.op_records():
        op, t = mxompi.OPS[rec["op"]], mxompi.TYPES[rec["type"]]
        run(rec["kind"], op, t, rec["a"], rec["b"], rec["n"], rec["out"], f"golden k{rec['kind']} {op} {t}")
    assert mxompi.op_service_stats()[0] == 1, "service unusable on this box"
    count = ov.SERVICE_COUNT
    for op, t in PAIRS:
        a, b = ov.inputs(op, t, 2, count, 100)
        exp = b.copy()
        assert O.mxo_reduce2(mxompi.OP[op], mxompi.TYPE[t], a.ctypes.data, exp.ctypes.data, count, 1) == 0
        run(2, op, t, a, b, count, exp, f"edge values {op} {t} count={count}")
        exp = np.zeros(len(b), np.uint8)     # the 3-buffer form has its own evaluator (OP3)
        assert O.mxo_reduce3(mxompi.OP[op], mxompi.TYPE[t], a.ctypes.data, b.ctypes.data, exp.ctypes.data,
                             count, 1) == 0
        run(3, op, t, a, b, count, exp, f"edge values, 3-buffer {op} {t} count={count}")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:40])
