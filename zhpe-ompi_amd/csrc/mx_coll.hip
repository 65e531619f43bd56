// mx_coll.hip -- all-peer xGMI collectives with the reference's fold order.
//
// What the reference does (ompi/mca/coll/base/coll_base_allreduce.c et al.):
// n-1 neighbour exchanges through the PML, one host `ompi_op_reduce` per
// step.  What this file does on MI355X:
//
//   * a FOLD PROGRAM describes, for a range of elements, the exact reduction
//     tree the selected reference algorithm applies to the n contributions:
//       CHAIN      acc = x[o0]; acc = OP(x[oj], acc) (ring: local operand is
//                  the target, :471/:782) or OP(acc, x[oj]) (basic linear
//                  reduce, coll_base_reduce.c:62-81), for j = 1..n-1;
//       BUTTERFLY  a binary tree over p' = 2^D virtual ranks combined level
//                  by level; at each level the operand holding the `pref`
//                  side is the target.  Recursive doubling (:130-274) is
//                  pref = all ones (every rank computes OP(high, low)),
//                  Rabenseifner (:970-1243) and recursive halving
//                  (coll_base_reduce_scatter.c:132-) are pref = the final
//                  owner's virtual rank; leaves fold the non-power-of-two
//                  pairs (2v, 2v+1) first in the reference's order.
//   * ONE fused kernel per output part loads the n contributions (16-B
//     vectors), evaluates the program in registers (uniform control flow),
//     and stores the result to every destination (local rbuf and each
//     peer's gather area = the allgather push over all xGMI links at once).
//   * multi-process: contributions are pushed all-peer into IPC-mapped
//     staging (uncached device memory), ordered by generation-tagged
//     system-scope flags and bounded spins; local (1-process) communicators
//     read/write every rank's buffers directly.
//
// Work partition (who computes which elements) is COLL_BASE_COMPUTE_
// BLOCKCOUNT over each chunk (coll_base_functions.h:428-435); the FOLD
// partition (which tree an element gets) always follows the reference
// algorithm over the full count, so chunking never changes results.  The
// fold programs and expression DAGs are planned on the host in mx_plan.hip.
#include <hip/hip_runtime.h>
#include <thread>
#include <rccl/rccl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include <climits>
#include <chrono>
#include <map>
#include <mutex>
#include <new>
#include <atomic>
#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include "mx_comm.hpp"
#include "../../include/mx_convertor.h"
#include "mx_env.hpp"
#include "mx_exchange.hpp"
#include "mx_rooted_plan.hpp"

namespace mx {

// ---------------------------------------------------------------------------
// multi-job byte copy (scatter push, gather, allgather, bcast)
// ---------------------------------------------------------------------------
struct CopyJob { const char *src; char *dst; size_t bytes; };
struct CopyArgs { CopyJob j[MAXR]; int n; unsigned bpj; const int *poison; };

// Jobs are interleaved block by block (job = blockIdx.x % n): a push to
// n-1 peers keeps every xGMI link busy from the first wave on, instead of
// draining the peers one after another in dispatch order.
template <bool NT>
__global__ void __launch_bounds__(kFB) k_copy(CopyArgs a) {
  if (poisoned(a.poison)) return;
  const CopyJob jb = a.j[blockIdx.x % (unsigned)a.n];
  const size_t tid = (size_t)(blockIdx.x / (unsigned)a.n) * kFB + threadIdx.x;
  const uintptr_t ms = (uintptr_t)jb.src & 15, md = (uintptr_t)jb.dst & 15;
  if (ms == md) {
    size_t head = ms ? 16 - ms : 0;
    if (head > jb.bytes) head = jb.bytes;
    const size_t nvec = (jb.bytes - head) / 16;
    if (tid < nvec)
    {
      uint4 v;
      ld16<NT>(v, reinterpret_cast<const uint4 *>(jb.src + head) + tid);
      st16<NT>(reinterpret_cast<uint4 *>(jb.dst + head) + tid, v);
    }
    const size_t tail0 = head + nvec * 16;
    if (tid < head) jb.dst[tid] = jb.src[tid];
    if (tid < jb.bytes - tail0) jb.dst[tail0 + tid] = jb.src[tail0 + tid];
  } else {
    for (size_t i = tid; i < jb.bytes; i += (size_t)a.bpj * kFB) jb.dst[i] = jb.src[i];
  }
}

static int copy_launch(CopyArgs &a, hipStream_t s) {
  size_t maxw = 1, total = 0;
  int k = 0;
  for (int i = 0; i < a.n; i++) {
    if (a.j[i].bytes == 0) continue;
    a.j[k++] = a.j[i];
    size_t w = a.j[i].bytes / 16 + 32;
    if (w > maxw) maxw = w;
    total += a.j[i].bytes;
  }
  a.n = k;
  if (k == 0) return MX_SUCCESS;
  const size_t g = (maxw + kFB - 1) / kFB;
  if (g * (size_t)k * kFB > 0xffffffffu) return MX_ERR_UNSUPPORTED;   // HIP: grid threads < 2^32
  a.bpj = (unsigned)g;
  if (mx_nt_for(2 * total))
    hipLaunchKernelGGL(k_copy<true>, dim3((unsigned)(g * k)), dim3(kFB), 0, s, a);
  else
    hipLaunchKernelGGL(k_copy<false>, dim3((unsigned)(g * k)), dim3(kFB), 0, s, a);
  return mx_check_launch();
}

// Device-to-device copy on `s` (K7, opal_datatype_copy_content_same_ddt for a
// contiguous type, opal_datatype_copy.c:99-141): the 16-byte copy kernel when
// both ends share their misalignment mod 16, else the runtime's copy.
int copy_async(void *dst, const void *src, size_t bytes, hipStream_t s) {
  if (!bytes || dst == src) return MX_SUCCESS;
  if ((((uintptr_t)dst ^ (uintptr_t)src) & 15) == 0) {
    CopyArgs a;
    memset(&a, 0, sizeof a);
    a.j[0] = CopyJob{(const char *)src, (char *)dst, bytes};
    a.n = 1;
    return copy_launch(a, s);
  }
  return mx_hip_rc(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
}

// a communicator's copy: skipped on the device once the communicator is poisoned
static int copy_launch(const mx_comm *c, CopyArgs &a, hipStream_t s) {
  a.poison = c ? c->poison : nullptr;
  return copy_launch(a, s);
}

// ---------------------------------------------------------------------------
// cross-GPU flags: generation-tagged, system scope, bounded spin
// ---------------------------------------------------------------------------

// bytes per rank (default; MX_ONESHOT_MAX overrides).  Round 1 put the
// crossover with the nine-launch staged path at 256 KiB - 1 MiB; since the
// staged / zero-copy rounds take six launches and the completion word, they
// win from 256 KiB (2 ranks on one GPU: 256 KiB 27 vs 31 us, 1 MiB 26 vs
// 51 us; profiles/r02/allreduce_oneshot_crossover.txt), so one-shot keeps
// the messages up to 128 KiB (24.7 vs 26.3 us there).
constexpr size_t kOneShotMax = 128 << 10;
constexpr size_t kOneShotCap = 1 << 20;   // one-shot slot capacity per rank (autotuning range)

static size_t oneshot_max() {
  const char *e = getenv("MX_ONESHOT_MAX");
  if (!e || !*e) return kOneShotMax;
  const long long v = atoll(e);
  return v > 0 ? (size_t)v : 0;
}

struct SignalArgs {
  uint64_t *peer_flag[MAXR];
  int n;
  uint64_t value;
  const int *poison;
  uint64_t *mark;     // a blocking call's completion word (Mark.word), raised after the flags, or null
  uint64_t mark_v;
};

__global__ void k_signal(SignalArgs a) {
  const int j = threadIdx.x;
  if (poisoned(a.poison)) return;   // a wait before this one timed out: tell no peer anything
  __threadfence_system();  // everything this stream wrote is visible first (the fence is the release)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // keep the write-back ahead of the flag (guide G16 pitfall 12)
  if (j < a.n && a.peer_flag[j])
    __hip_atomic_store(a.peer_flag[j], a.value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (a.mark && j == 0) __hip_atomic_store(a.mark, a.mark_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Waits until flags[j] >= value for every j in `mask`; a timeout raises the
// host error and poisons the communicator (timeout_ticks = ~0: wait forever).
//
// Cross-device memory model: a wait is the acquire before this
// rank reads what its peers published -- their staging (uncached: never in an
// L2) or, on the zero-copy paths, their cacheable user buffers over xGMI.
// Remote lines may sit in this GPU's L2s from an earlier call, and each of
// the 8 XCDs has its own L2, so every workgroup of the wait polls the flags
// itself and then takes a SYSTEM-scope acquire (buffer_inv sc0 sc1, which
// drops the non-coherent -- remote -- lines of its XCD's L2); kWaitBlocks
// workgroups, dealt round-robin over the XCDs, cover all of them.  The
// writer side is the signal's system-scope release (buffer_wbl2 sc0 sc1)
// after the end-of-kernel release of the user's producing kernels.
constexpr int kWaitBlocks = 16;

__global__ void k_wait(const uint64_t *flags, uint32_t mask, uint64_t value, uint64_t timeout_ticks, int *err,
                       int *poison) {
  const int j = threadIdx.x;
  if (j < MAXR && ((mask >> j) & 1) && !poisoned(poison)) {
    const uint64_t t0 = wall_clock64();
    while (__hip_atomic_load(&flags[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < value) {
      __builtin_amdgcn_s_sleep(2);
      if (wall_clock64() - t0 > timeout_ticks) {
        raise_timeout(err, poison);
        break;
      }
    }
  }
  __syncthreads();
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

// k_signal then k_wait in one launch (one kernel and one inter-kernel gap
// less per phase): thread j raises my flag at peer j, then spins on flag j
// of mine.  Poisoned: neither.
__global__ void k_signal_wait(SignalArgs a, const uint64_t *flags, uint32_t mask, uint64_t value,
                              uint64_t timeout_ticks, int *err, int *poison) {
  const int j = threadIdx.x;
  if (!poisoned(a.poison)) {
    if (blockIdx.x == 0) {   // the signal half: once
      __threadfence_system();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (j < a.n && a.peer_flag[j])
        __hip_atomic_store(a.peer_flag[j], a.value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (j < MAXR && ((mask >> j) & 1)) {
      const uint64_t t0 = wall_clock64();
      while (__hip_atomic_load(&flags[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < value) {
        __builtin_amdgcn_s_sleep(2);
        if (wall_clock64() - t0 > timeout_ticks) {
          raise_timeout(err, poison);
          break;
        }
      }
    }
  }
  __syncthreads();
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

}  // namespace mx

using namespace mx;

static uint64_t ticks_for(double seconds) {
  int rate_khz = 0;
  if (hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, 0) != hipSuccess || rate_khz <= 0)
    rate_khz = 100000;
  return (uint64_t)(seconds * rate_khz * 1000.0);
}

extern "C" int mx_comm_set_profiling(mx_comm_t *c, int on) {
  if (!c) return MX_ERR_ARG;
  if (on && !c->prof) {
    for (int i = 0; i < 64; i++)
      if (hipEventCreate(&c->ev[i]) != hipSuccess) return MX_ERR_HIP;
  }
  c->prof = on ? 1 : 0;
  c->nev = 0;
  return MX_SUCCESS;
}

extern "C" int mx_comm_get_stats(mx_comm_t *c, mx_coll_stats_t *st, int reset) {
  if (!c || !st) return MX_ERR_ARG;
  *st = c->st;
  if (reset) memset(&c->st, 0, sizeof c->st);
  return MX_SUCCESS;
}

// bracket a kernel with an event pair (no-op unless profiling)
static inline void prof_begin(mx_comm *c, hipStream_t s) {
  if (c && c->prof && c->nev + 2 <= 64) (void)hipEventRecord(c->ev[c->nev], s);
}
static inline void prof_end(mx_comm *c, hipStream_t s, int kind, double bytes) {
  if (c && c->prof && c->nev + 2 <= 64) {
    (void)hipEventRecord(c->ev[c->nev + 1], s);
    c->ev_kind[c->nev / 2] = kind;
    c->ev_bytes[c->nev / 2] = bytes;
    c->nev += 2;
  }
}
static void prof_collect(mx_comm *c) {
  if (!c || !c->prof) return;
  c->st.calls++;
  for (int i = 0; i < c->nev; i += 2) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]);
    const int k = c->ev_kind[i / 2];
    if (k == 0) { c->st.fold_ms += ms; c->st.fold_launches++; c->st.fold_bytes += c->ev_bytes[i / 2]; }
    else if (k == 1) c->st.push_ms += ms;
    else c->st.gather_ms += ms;
  }
  if (c->nev >= 2) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[c->nev - 1]);
    c->st.total_ms += ms;
  }
  c->nev = 0;
}

extern "C" int mx_comm_set_timeout(mx_comm_t *c, double seconds) {
  if (!c || seconds < 0) return MX_ERR_ARG;
  c->timeout_s = seconds;
  c->timeout_ticks = seconds == 0 ? ~(uint64_t)0 : ticks_for(seconds);
  return MX_SUCCESS;
}

extern "C" int mx_comm_size(const mx_comm_t *c) { return c ? c->size : MX_ERR_ARG; }
extern "C" int mx_comm_rank(const mx_comm_t *c) { return c ? c->rank : MX_ERR_ARG; }

static void live_add(mx_comm *c);

extern "C" int mx_comm_create_local(int size, int device, mx_comm_t **out) {
  if (!out || size < 1 || size > MAXR) return MX_ERR_ARG;
  int rc = mx_init(device);
  if (rc) return rc;
  mx_comm *c = (mx_comm *)calloc(1, sizeof(mx_comm));
  if (!c) return MX_ERR_NOMEM;
  c->rank = 0;
  c->size = size;
  c->device = g_device;
  c->local = 1;
  mx_comm_set_timeout(c, 60.0);
  live_add(c);
  *out = c;
  return MX_SUCCESS;
}

struct ipc_info {
  hipIpcMemHandle_t staging, flags, hregion;
  int rank, device, ok;
  uint64_t staging_bytes, hregion_bytes;
  char pci[32];   // PCI bus id of the rank's GPU (hipDeviceGetPCIBusId)
  char shm[48];   // rank 0: name of the registration page ("" = none)
};

// ---------------------------------------------------------------------------
// user-buffer registration exchange (zero-copy allreduce).  One
// record per rank in a POSIX shared-memory page (the ranks of an IPC
// communicator share a node).  Per call k every rank publishes the IPC
// handles of its buffers (seq = k, written last), reads every peer's, maps
// them (cached), then publishes whether that worked (vseq = k); all ranks
// see the same records and verdicts, so all take the same path.  A record
// is rewritten only at call k+1, which no rank reaches before every peer
// has read record k (call k needs every rank's device participation).
// ---------------------------------------------------------------------------
struct RegBuf {
  hipIpcMemHandle_t h;          // the allocation holding the buffer
  uint64_t base, size, id;      // its base address, size and runtime buffer id (exporter side)
  uint64_t off;                 // the buffer's offset in it
};
struct RegRec {
  std::atomic<uint64_t> seq, vseq;
  RegBuf sb, rb;
  int32_t ok, mis, verdict, pad_;
  std::atomic<uint64_t> tseq;   // autotuning: the call's elapsed time, published with tseq
  double t;
  char pad[256 - 2 * 8 - 2 * sizeof(RegBuf) - 4 * 4 - 2 * 8];
};
static_assert(sizeof(RegRec) == 256, "RegRec layout");
static_assert(std::atomic<uint64_t>::is_always_lock_free, "shared-memory atomics");

// The page: two banks of records (reg_exchange), then the row area of
// alltoallv (xrow_exchange): every rank publishes the row it sends by, (offsets, sizes) -- one
// host round like tune_exchange.
// Two banks, call k in bank k % 2, for the reason reg_exchange gives.
// the strided forms (mx_alltoallv_ddt) add the send layout, the lower bound
// of the send span the rank registers, its access units and its verdict
struct XRowExt {
  XLay slay;
  int64_t lo;
  uint32_t sunit, runit;
  int32_t verdict, pad;
  RRowHead r;   // the rooted forms (mx_gather ...): bytes[] / offs[] then carry the root's per-rank blocks
};
struct XRow {
  std::atomic<uint64_t> seq;
  uint64_t flags;   // bits 0-3: the send buffer's address mod 16; bit 4: the rank calls in place; bit 5: a strided form;
                    // bit 6: a rooted form
  uint64_t bytes[MAXR], offs[MAXR];
  XRowExt e;
};
static size_t reg_page_bytes(int n) { return 2 * (size_t)n * sizeof(RegRec) + 2 * (size_t)n * sizeof(XRow); }

// bytes per rank (MX_REG_MIN overrides; 0 = off): zero-copy is ahead of the
// staged path at every size measured above the one-shot range
constexpr size_t kRegMinDefault = (size_t)256 << 10;
constexpr size_t kRegCachePerPeer = 8;
constexpr size_t kTuneMin = (size_t)64 << 10;       // autotuned allreduces / bcasts: bytes per rank
constexpr size_t kTuneMinMove = (size_t)256 << 10;  // autotuned reduce_scatters / allgathers

static size_t reg_min() {
  const char *e = getenv("MX_REG_MIN");
  if (!e || !*e) return kRegMinDefault;
  const long long v = atoll(e);
  return v > 0 ? (size_t)v : 0;
}

// ---------------------------------------------------------------------------
// live communicators and deferred releases.  On this runtime
// hipFree, hipHostFree and hipIpcCloseMemHandle wait for every stream of the
// device (tools/lifecycle_sync_probe.hip, profiles/r05/lifecycle_sync_probe.txt),
// so a communicator freed -- or a stale zero-copy mapping closed -- while
// another communicator's request spins on a peer could deadlock a legal
// program.  They run when no live communicator has device work pending.
// ---------------------------------------------------------------------------
static std::mutex g_live_mu;
static std::vector<mx_comm *> g_live;
struct Deferred { void *p; int kind; };
static std::vector<Deferred> g_graveyard;

// exchange counters (mx_comm_exchange_stats): per communicator and, for a
// caller that cannot reach the communicator (an MPI program above the coll
// component), summed over the process
static std::atomic<uint64_t> g_xst[4], g_xdst[4];   // byte forms, strided forms
static void xcount(mx_comm *c, int k, bool ddt = false) {
  (ddt ? c->xdst : c->xst)[k]++;
  (ddt ? g_xdst : g_xst)[k].fetch_add(1, std::memory_order_relaxed);
}

// the rooted forms' counters (mx_comm_rooted_stats), kept apart from both
static std::atomic<uint64_t> g_rst[4];
static void rcount(mx_comm *c, int k) {
  c->rst[k]++;
  g_rst[k].fetch_add(1, std::memory_order_relaxed);
}

static void live_add(mx_comm *c) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  g_live.push_back(c);
}
static void live_del(mx_comm *c) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  for (size_t i = 0; i < g_live.size(); i++)
    if (g_live[i] == c) { g_live[i] = g_live.back(); g_live.pop_back(); break; }
}
static bool pending(hipError_t e) {
  if (e == hipErrorNotReady) { (void)hipGetLastError(); return true; }
  if (e != hipSuccess) (void)hipGetLastError();   // a failed request reports itself at its wait
  return false;
}
static bool device_quiet_locked() {
  for (mx_comm *c : g_live) {
    if (c->tail_valid && c->tail && pending(hipEventQuery(c->tail))) return false;
    if (p2p_pending(c)) return false;
  }
  return true;
}
bool mx::device_quiet() {
  std::lock_guard<std::mutex> lk(g_live_mu);
  return device_quiet_locked();
}
static void release_now(void *p, int kind) {
  hipError_t e = kind == REL_IPC ? hipIpcCloseMemHandle(p) : kind == REL_HOST ? hipHostFree(p) : hipFree(p);
  if (e != hipSuccess) (void)hipGetLastError();
}
bool mx::release_now_if_quiet(void *p, int kind) {
  if (!p) return true;
  std::unique_lock<std::mutex> lk(g_live_mu);
  if (!device_quiet_locked()) {
    g_graveyard.push_back(Deferred{p, kind});
    return false;
  }
  lk.unlock();
  release_now(p, kind);
  return true;
}
void mx::release_later(void *p, int kind) { (void)release_now_if_quiet(p, kind); }
bool mx::release_now_or_keep(void *p, int kind) {   // nothing queued when not quiet: the caller keeps p
  if (!p) return true;
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    if (!device_quiet_locked()) return false;
  }
  release_now(p, kind);
  return true;
}
bool mx::export_remade(uint64_t base, uint64_t size, uint64_t id) {
  struct Ex { uint64_t base, size, id; };
  static std::mutex mu;
  static std::vector<Ex> hist;   // every allocation exported (the last 4096)
  std::lock_guard<std::mutex> lk(mu);
  for (const Ex &e : hist)
    if (e.base < base + size && base < e.base + e.size) {
      if (e.base == base && e.size == size && e.id == id) return false;   // the same allocation
      return true;   // another allocation was exported over this range
    }
  if (hist.size() >= 4096) hist.erase(hist.begin());
  hist.push_back(Ex{base, size, id});
  return false;
}
uint64_t mx::ipc_object_id(const void *p) {
  unsigned long long id = 0;
  if (!p || hipPointerGetAttribute(&id, HIP_POINTER_ATTRIBUTE_BUFFER_ID, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return id;
}
void mx::ipc_gone_add(std::vector<IpcGone> &g, int64_t owner, uint64_t base, uint64_t size, const void *mapping) {
  const uint64_t oid = ipc_object_id(mapping);
  if (!oid) return;
  if (g.size() >= 64) g.erase(g.begin());
  g.push_back(IpcGone{owner, base, size, oid});
}
int mx::ipc_open_checked(const void *handle, std::vector<IpcGone> &g, int64_t owner, uint64_t base, uint64_t size,
                         char **out, uint64_t *oid) {
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof h);
  char *p = nullptr;
  if (hipIpcOpenMemHandle((void **)&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess || !p) {
    (void)hipGetLastError();
    return MX_ERR_HIP;
  }
  const uint64_t id = ipc_object_id(p);
  bool old = false;
  for (const IpcGone &d : g)
    if (id && d.owner == owner && d.base < base + size && base < d.base + d.size && d.oid == id) old = true;
  if (!old && id) {   // a new object at that range: the closed ones are gone
    for (size_t i = 0; i < g.size();) {
      if (g[i].owner == owner && g[i].base < base + size && base < g[i].base + g[i].size) g.erase(g.begin() + (long)i);
      else i++;
    }
  }
  if (old) {
    release_later(p, REL_IPC);   // drop the reference this open took
    return 0;
  }
  *out = p;
  *oid = id;
  return 1;
}
void mx::release_flush() {
  std::vector<Deferred> go;
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    if (g_graveyard.empty() || !device_quiet_locked()) return;
    go.swap(g_graveyard);
  }
  for (const Deferred &d : go) release_now(d.p, d.kind);
}
extern "C" int mx_release_pending(void) {   // tests: deferred releases not yet run
  std::lock_guard<std::mutex> lk(g_live_mu);
  return (int)g_graveyard.size();
}

// The last exchange of a communicator, identical on every rank: the records
// every rank read (they are the same shared records) and the final verdict.
struct RegFast {
  bool valid = false;
  std::vector<RegBuf> sb, rb;
  std::vector<int32_t> mis, ok;
  const char *ps[MAXR];
  char *pr[MAXR];
};

static void reg_fast_free(mx_comm *c) {
  delete (RegFast *)c->reg_fast;
  c->reg_fast = nullptr;
}

static void reg_release(mx_comm *c) {
  reg_fast_free(c);
  if (c->reg_imp) {
    for (const mx_reg_import &m : *c->reg_imp) release_later(m.ptr, REL_IPC);
    delete c->reg_imp;
    c->reg_imp = nullptr;
    delete c->reg_gone;
    c->reg_gone = nullptr;
  }
  if (c->reg_shm) munmap(c->reg_shm, c->reg_shm_bytes);
  c->reg_shm = nullptr;
}

// rank 0 creates the page before the first exchange; the others open it
// after it; rank 0 unlinks it once every rank has agreed (nothing is left in
// /dev/shm whatever happens later)
static void reg_create(mx_comm *c, char *name, size_t cap) {
  static std::atomic<unsigned> ctr{0};
  name[0] = 0;
  if (c->size < 2 || !reg_min()) return;
  snprintf(name, cap, "/mx_reg_%d_%u", (int)getpid(), ctr.fetch_add(1));
  const size_t bytes = reg_page_bytes(c->size);
  const int fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
  if (fd < 0) { name[0] = 0; return; }
  void *p = MAP_FAILED;
  if (ftruncate(fd, (off_t)bytes) == 0) p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (p == MAP_FAILED) { shm_unlink(name); name[0] = 0; return; }
  memset(p, 0, bytes);
  c->reg_shm = p;
  c->reg_shm_bytes = bytes;
}

static void reg_open(mx_comm *c, const char *name) {
  if (c->reg_shm || !name[0]) return;
  const size_t bytes = reg_page_bytes(c->size);
  const int fd = shm_open(name, O_RDWR, 0600);
  if (fd < 0) return;
  void *p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (p == MAP_FAILED) return;
  c->reg_shm = p;
  c->reg_shm_bytes = bytes;
}

static int proto_default(const mx_comm *c) {
  const char *e = getenv("MX_ALLREDUCE_PROTO");
  if (e && !strcmp(e, "push")) return MX_PROTO_PUSH;
  if (e && !strcmp(e, "pull")) return MX_PROTO_PULL;
  // PULL: one xGMI phase and no DONE(g-1) wait; measured ahead of PUSH on one
  // GPU too, so it no longer depends on c->xdev
  (void)c;
  return MX_PROTO_PULL;
}

extern "C" int mx_comm_set_protocol(mx_comm_t *c, int proto) {
  if (!c || proto < MX_PROTO_AUTO || proto > MX_PROTO_PULL) return MX_ERR_ARG;
  c->proto = proto == MX_PROTO_AUTO ? proto_default(c) : proto;
  return c->proto;
}

extern "C" int mx_comm_get_protocol(const mx_comm_t *c) { return c ? c->proto : MX_ERR_ARG; }

// MX_ZC_DIRECT=0: zero-copy allreduce results go through the peers' uncached
// gather areas and a gather copy (round 4's path; A/B switch)
static int zc_direct_default() {
  const char *e = getenv("MX_ZC_DIRECT");
  return !(e && *e == '0');
}

extern "C" int mx_comm_set_zc_direct(mx_comm_t *c, int on) {
  if (!c) return MX_ERR_ARG;
  c->zc_direct = on ? 1 : 0;
  return MX_SUCCESS;
}

extern "C" int mx_comm_set_autotune(mx_comm_t *c, int on) {
  if (!c) return MX_ERR_ARG;
  if (on && !c->reg_shm) return MX_ERR_UNSUPPORTED;   // the timings travel through the registration page
  c->tune_on = on ? 1 : 0;
  return MX_SUCCESS;
}

extern "C" int mx_comm_get_tuning(const mx_comm_t *c, size_t bytes) {
  return mx_comm_get_tuning_ex(c, 0, bytes);   // TUNE_ALLREDUCE
}

extern "C" int mx_comm_get_tuning_ex(const mx_comm_t *c, int coll, size_t bytes) {
  if (!c || !bytes || coll < 0 || coll > 3) return MX_ERR_ARG;
  const int b = 63 - __builtin_clzll((unsigned long long)bytes);
  return c->tune_best[coll][b] ? c->tune_best[coll][b] - 1 : -1;
}

extern "C" int mx_comm_set_reg_min(mx_comm_t *c, size_t min_bytes) {
  if (!c) return MX_ERR_ARG;
  if (!c->reg_shm) return min_bytes ? MX_ERR_UNSUPPORTED : MX_SUCCESS;
  c->reg_min = min_bytes;
  return MX_SUCCESS;
}

extern "C" long long mx_comm_set_oneshot_max(mx_comm_t *c, size_t max_bytes) {
  if (!c) return MX_ERR_ARG;
  c->os_max = std::min(max_bytes, c->os_cap);
  return (long long)c->os_max;
}

extern "C" int mx_comm_create(int rank, int size, int device, size_t staging_bytes, int flags,
                              mx_allgather_fn ag, void *ctx, mx_comm_t **out) {
  return mx_comm_create_ex(rank, size, device, staging_bytes, 0, flags, ag, ctx, out);
}

// IPC-exported regions (staging, flags, heap region) outlive their
// communicator in a process-wide pool.  Ranks destroy a communicator at
// different times, so a peer may still map this rank's region when the
// rank frees it, and the runtime then refused to export a new allocation
// made in that place: hipIpcGetMemHandle failed (hsa_status 0x1000) on the
// next communicator's staging in 8-process runs that create and free
// communicators back to back.  A destroyed communicator's regions therefore
// go back to the pool and a later communicator reuses them (same
// allocation, same handle) instead of freeing and reallocating.
//
// A region goes back to the pool only once every peer has said BYE
// (round 4).  A rank may finish its last call of a communicator while a
// peer's trailing signals of that call are still on their way into its
// flags: DONE(g) ends every round and is waited for only by the next call,
// and a rooted reduce's non-roots never wait for PUSHED(g).  Round 3
// recycled the flags at once; the next communicator zeroed them at creation,
// the late DONE / PUSHED of the old one landed after that, and a wait of
// the new one for PUSHED(2) passed on the stale PUSHED(6): one rank gathered
// one peer's part before that peer had written it (the 5000-element block of
// test_tuned_forced_rules_and_basic_orders[8-device]).  Now
// mx_comm_destroy waits for its own device to go idle and then writes BYE
// into every peer's flags; a destroyed communicator's regions wait in
// quarantine until the BYE row of its flags shows every peer.
static std::mutex g_ipc_pool_mu;
static std::vector<std::pair<char *, size_t>> g_ipc_pool;
struct IpcQuarantine { char *staging, *hregion; uint64_t *flags; uint32_t peers, scans; };
static std::vector<IpcQuarantine> g_ipc_quarantine;
// A peer that never destroys the communicator (it aborted, or exits without
// MPI_Comm_free) never says BYE: its regions would be rescanned at every
// creation for the rest of the process.  After kQuarantineScans scans (or
// beyond kQuarantineMax groups, oldest first) a group is given up: it stays
// allocated -- never reused, never freed under a peer's mapping -- and is
// no longer scanned.
constexpr uint32_t kQuarantineScans = 64;
constexpr size_t kQuarantineMax = 32;
static uint64_t g_ipc_abandoned;

static size_t ipc_region_size(const char *p);

// MX_IPC_QUARANTINE=0: round 3's immediate recycling (the regression
// demonstration of tools/stale_flag_repro.py only)
static bool ipc_quarantine_on() { static const bool v = env_default_on("MX_IPC_QUARANTINE"); return v; }

static void ipc_pool_put(char *p) {   // caller holds g_ipc_pool_mu
  if (p) g_ipc_pool.emplace_back(p, ipc_region_size(p));
}

// move every quarantined group whose peers have all said BYE to the pool
static void ipc_quarantine_scan() {
  std::lock_guard<std::mutex> lk(g_ipc_pool_mu);
  while (g_ipc_quarantine.size() > kQuarantineMax) {
    g_ipc_quarantine.erase(g_ipc_quarantine.begin());
    g_ipc_abandoned++;
  }
  for (size_t i = 0; i < g_ipc_quarantine.size();) {
    IpcQuarantine &q = g_ipc_quarantine[i];
    if (++q.scans > kQuarantineScans) {
      g_ipc_quarantine.erase(g_ipc_quarantine.begin() + (long)i);
      g_ipc_abandoned++;
      continue;
    }
    uint64_t bye[MAXR];
    hipStream_t ls = life_stream();
    bool clear = hipMemcpyAsync(bye, q.flags + BYE_BASE, sizeof bye, hipMemcpyDeviceToHost, ls) == hipSuccess &&
                 hipStreamSynchronize(ls) == hipSuccess;
    if (!clear) (void)hipGetLastError();
    for (int p = 0; clear && p < MAXR; p++)
      if (((q.peers >> p) & 1) && bye[p] != BYE_WORD) clear = false;
    if (!clear) { i++; continue; }
    ipc_pool_put(q.staging);
    ipc_pool_put(q.hregion);
    ipc_pool_put((char *)q.flags);
    g_ipc_quarantine.erase(g_ipc_quarantine.begin() + (long)i);
  }
}

static int ipc_region_alloc(size_t bytes, char **p) {
  {
    std::lock_guard<std::mutex> lk(g_ipc_pool_mu);
    size_t best = (size_t)-1;
    for (size_t i = 0; i < g_ipc_pool.size(); i++)   // smallest pooled region that fits, at most 2x
      if (g_ipc_pool[i].second >= bytes && g_ipc_pool[i].second <= 2 * bytes &&
          (best == (size_t)-1 || g_ipc_pool[i].second < g_ipc_pool[best].second))
        best = i;
    if (best != (size_t)-1) {
      *p = g_ipc_pool[best].first;
      g_ipc_pool.erase(g_ipc_pool.begin() + (long)best);
      hipIpcMemHandle_t h;   // (exported before: the same handle again)
      if (hipIpcGetMemHandle(&h, *p) == hipSuccess) return MX_SUCCESS;
      (void)hipGetLastError();
      fprintf(stderr, "mx: a pooled %zu-byte region could not be exported again; allocating another\n", bytes);
      *p = nullptr;   // (left allocated, out of the pool)
    }
  }
  // A fresh allocation may land where an exported allocation of this
  // process was freed (a torch buffer registered for zero-copy, then
  // released), and the runtime then refuses to export it: hipIpcGetMemHandle
  // failed with "invalid argument" on a recycled communicator's heap region
  // (profiles/r06/gpu_suite_r6az_export_refused.txt).  Such an allocation is
  // kept aside -- so the next one lands elsewhere -- and another is made.
  static std::vector<void *> g_unexportable;   // (under g_ipc_pool_mu below)
  for (int attempt = 0; attempt < 4; attempt++) {
    if (hipExtMallocWithFlags((void **)p, bytes, hipDeviceMallocUncached) != hipSuccess) {
      (void)hipGetLastError();
      *p = nullptr;
      return MX_ERR_NOMEM;
    }
    hipIpcMemHandle_t h;
    if (hipIpcGetMemHandle(&h, *p) == hipSuccess) return MX_SUCCESS;
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(g_ipc_pool_mu);
    g_unexportable.push_back(*p);
    fprintf(stderr, "mx: a fresh %zu-byte region could not be exported; allocating another\n", bytes);
  }
  *p = nullptr;
  return MX_ERR_NOMEM;
}

static size_t ipc_region_size(const char *p) {
  void *base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (void *)p) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return size;
}

// a destroyed communicator's regions: to the pool once `peers` said BYE
static void ipc_regions_release(char *staging, char *hregion, uint64_t *flags, uint32_t peers) {
  std::lock_guard<std::mutex> lk(g_ipc_pool_mu);
  if (!flags || !peers || !ipc_quarantine_on()) {
    ipc_pool_put(staging);
    ipc_pool_put(hregion);
    ipc_pool_put((char *)flags);
    return;
  }
  g_ipc_quarantine.push_back(IpcQuarantine{staging, hregion, flags, peers, 0});
}

extern "C" int mx_ipc_quarantine_stats(int *held, unsigned long long *abandoned) {   // tests
  std::lock_guard<std::mutex> lk(g_ipc_pool_mu);
  if (held) *held = (int)g_ipc_quarantine.size();
  if (abandoned) *abandoned = g_ipc_abandoned;
  return MX_SUCCESS;
}

// BYE: written after this rank's device went idle (no poison check: a
// poisoned communicator's kernels have ended too)
__global__ void k_bye(SignalArgs a) {
  const int j = threadIdx.x;
  __threadfence_system();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (j < a.n && a.peer_flag[j])
    __hip_atomic_store(a.peer_flag[j], BYE_WORD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// fault injection (tests only, MX_DEBUG_LAG_RANK / _US): that rank's fold
// kernels start `ticks` of the wall clock late, so its results and its
// trailing signals reach the peers late
__global__ void k_lag(uint64_t ticks) {
  const uint64_t t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}
static void lag_launch(const mx_comm *c, hipStream_t s) {
  if (c && c->lag_ticks) hipLaunchKernelGGL(k_lag, dim3(1), dim3(1), 0, s, c->lag_ticks);
}

constexpr uint32_t all_ranks_mask(int n) { return (n >= 32) ? 0xffffffffu : ((1u << n) - 1); }

// my flag word `word0 + rank` at every peer (none at myself)
static SignalArgs signal_args(const mx_comm *c, size_t word0, uint64_t value) {
  SignalArgs a;
  memset(&a, 0, sizeof a);
  a.n = c->size;
  a.value = value;
  for (int p = 0; p < c->size; p++) a.peer_flag[p] = (p == c->rank) ? nullptr : c->peer_flags[p] + word0 + c->rank;
  return a;
}

// Every bootstrap exchange runs on every rank whatever happened locally:
// each carries this rank's verdict so far, and the communicator exists only
// if every rank says yes -- so either all ranks get one or none does (a rank
// failing alone would otherwise leave its peers blocked in the exchange, or
// give ranks different protocols to run).
static int agree(mx_allgather_fn ag, void *ctx, int size, int ok) {
  int *oks = (int *)calloc(size, sizeof(int));
  if (!oks) return -1;   // cannot even take part: the exchange itself fails
  int all = ag(&ok, oks, sizeof(int), ctx) == 0 ? 1 : -1;
  for (int p = 0; p < size && all == 1; p++)
    if (!oks[p]) all = 0;
  free(oks);
  return all;
}

extern "C" int mx_comm_create_ex(int rank, int size, int device, size_t staging_bytes, size_t heap_bytes, int flags,
                                 mx_allgather_fn ag, void *ctx, mx_comm_t **out) {
  if (!out || !ag || size < 1 || rank < 0 || rank >= size) return MX_ERR_ARG;
  if ((flags & MX_COMM_IPC) && size > MAXR) return MX_ERR_ARG;
  int ok = mx_init(device) == MX_SUCCESS;
  if (ok) release_flush();
  mx_comm *c = (mx_comm *)calloc(1, sizeof(mx_comm));
  ok = ok && c;
  int rc = MX_ERR_HIP;
  if (c) {
    c->rank = rank;
    c->size = size;
    c->device = g_device;
    c->flags = flags;
    c->ag = ag;
    c->ag_ctx = ctx;
    c->zc_direct = zc_direct_default();
    mx_comm_set_timeout(c, 60.0);
  }
  // no device-wide synchronisation anywhere in creation: another
  // communicator's collective or receive may be spinning on a peer that is
  // about to enter this very creation; small buffers come
  // from the process pools, memsets and copies run on the lifecycle stream
  hipStream_t ls = ok ? life_stream() : nullptr;
  ok = ok && (c->err_host = (int *)pool_host_get(sizeof(int))) != nullptr;
  if (ok) *c->err_host = 0;
  ok = ok && hipHostGetDevicePointer((void **)&c->err_dev, c->err_host, 0) == hipSuccess;
  ok = ok && (c->poison = (int *)pool_dev_get(sizeof(int))) != nullptr &&
       hipMemsetAsync(c->poison, 0, sizeof(int), ls) == hipSuccess;

  if (flags & MX_COMM_IPC) {
    ipc_info mine, all[MAXR];
    memset(&mine, 0, sizeof mine);
    memset(all, 0, sizeof all);
    if (ok) {
      c->staging_bytes = staging_bytes ? staging_bytes : ((size_t)64 << 20);
      // one-shot region at the top of staging: 2 parities x n slots
      // the region holds up to os_cap per rank (autotuning may move the
      // one-shot crossover up to it); os_max is the default crossover
      // (MX_ONESHOT_MAX forces the crossover: the capacity is that value)
      const char *ose = getenv("MX_ONESHOT_MAX");
      c->os_cap = std::min<size_t>((ose && *ose) ? oneshot_max() : std::max<size_t>(kOneShotCap, oneshot_max()),
                                   c->staging_bytes / (8 * (size_t)size)) & ~(size_t)255;
      if (c->os_cap < 1024) c->os_cap = 0;
      c->os_max = std::min<size_t>(oneshot_max(), c->os_cap);
      // (MX_ONESHOT_LL=0: the raw protocol at every size; same on every rank)
      const char *lle = getenv("MX_ONESHOT_LL");
      // (the LL area, 2 * os_ll, kept within half the raw slot: small
      // stagings keep their room for the staged paths)
      c->os_ll = (lle && *lle == '0') ? 0 : std::min<size_t>(OS_LL_CAP, c->os_cap / 4) & ~(size_t)15;
      c->os_slot = c->os_cap ? c->os_cap + 256 + 2 * c->os_ll : 0;
      c->main_bytes = (c->staging_bytes - 2 * (size_t)size * c->os_slot) & ~(size_t)255;
      c->hregion_bytes = heap_bytes ? ((heap_bytes + 4095) & ~(size_t)4095) : 0;
      // point-to-point mailboxes (one per source rank) follow the staging
      c->p2p_off = (c->staging_bytes + 4095) & ~(size_t)4095;
      const uint64_t sig[2] = {0x5EED0000ull + (uint64_t)rank, 0x5EED1000ull + (uint64_t)rank};
      const size_t boxes = (flags & MX_COMM_P2P) ? (size_t)size * P2P_BOX : 0;
      c->staging_alloc = c->p2p_off + boxes;
      ipc_quarantine_scan();
      int stage = 0;   // the step that failed, for the diagnostic below
      ok = (++stage, ipc_region_alloc(c->staging_alloc, &c->staging) == MX_SUCCESS) &&
           (++stage, ipc_region_alloc(ALL_FLAG_WORDS * sizeof(uint64_t), (char **)&c->flagmem) == MX_SUCCESS) &&
           (++stage, !c->hregion_bytes || ipc_region_alloc(c->hregion_bytes, &c->hregion) == MX_SUCCESS) &&
           (++stage, hipMemsetAsync(c->flagmem, 0, ALL_FLAG_WORDS * sizeof(uint64_t), ls) == hipSuccess) &&
           // the one-shot slots too: a recycled staging region still holds the
           // previous communicator's tagged words, whose generations the new
           // communicator's count restarts through (tag 0 is never current);
           // no peer writes here before exchange 1, old peers have said BYE
           (++stage, !c->os_slot || hipMemsetAsync(c->staging + c->main_bytes, 0, 2 * (size_t)size * c->os_slot,
                                                   ls) == hipSuccess) &&
           (++stage, hipIpcGetMemHandle(&mine.staging, c->staging) == hipSuccess) &&
           (++stage, hipIpcGetMemHandle(&mine.flags, c->flagmem) == hipSuccess) &&
           (++stage, !c->hregion || hipIpcGetMemHandle(&mine.hregion, c->hregion) == hipSuccess) &&
           // signature words, read back through every mapping below
           (++stage, hipMemcpyAsync(c->flagmem + FLAG_WORDS, sig, sizeof sig, hipMemcpyHostToDevice, ls) ==
                         hipSuccess) &&
           (++stage, !c->hregion || hipMemcpyAsync(c->hregion, sig + 1, 8, hipMemcpyHostToDevice, ls) == hipSuccess) &&
           (++stage, hipStreamSynchronize(ls) == hipSuccess);
      if (!ok) {
        const hipError_t e = hipGetLastError();   // a failed export must not surface at a later launch
        fprintf(stderr, "mx_comm_create: rank %d: local setup step %d failed (%s)\n", rank, stage,
                hipGetErrorString(e));
      }
      mine.staging_bytes = c->staging_bytes;
      mine.hregion_bytes = c->hregion_bytes;
    } else {
      fprintf(stderr, "mx_comm_create: rank %d: init / pooled buffers failed\n", rank);
      ok = 0;
    }
    mine.rank = rank;
    mine.device = c ? c->device : -1;
    if (c && hipDeviceGetPCIBusId(mine.pci, (int)sizeof mine.pci - 1, c->device) != hipSuccess) {
      (void)hipGetLastError();
      snprintf(mine.pci, sizeof mine.pci, "dev%d", c->device);
    }
    if (ok && rank == 0) reg_create(c, mine.shm, sizeof mine.shm);
    mine.ok = ok;
    // exchange 1: handles + verdicts (taken part in even after a local failure)
    if (ag(&mine, all, sizeof(ipc_info), ctx) != 0) ok = 0;
    if (ok && rank != 0) reg_open(c, all[0].shm);
    for (int p = 0; ok && p < size; p++)
      if (!all[p].ok || all[p].staging_bytes != c->staging_bytes || all[p].hregion_bytes != c->hregion_bytes) {
        if (rank == 0)
          fprintf(stderr, "mx_comm_create: rank %d reports %s\n", p, all[p].ok ? "other staging sizes" : "a local failure");
        ok = 0;
      }
    if (ok) {
      int per_dev = 1;   // most ranks on one device (the same on every rank)
      for (int p = 0; p < size; p++) {
        if (strncmp(all[p].pci, mine.pci, sizeof mine.pci)) c->xdev = 1;
        int k = 0;
        for (int q = 0; q < size; q++) k += !strncmp(all[p].pci, all[q].pci, sizeof mine.pci);
        per_dev = std::max(per_dev, k);
      }
      // MX_COLL_SERVICE_PER_DEV: most ranks per device with the service on
      // (default 2; more is for tests of the n > 2 served protocol on one GPU)
      const char *spd = getenv("MX_COLL_SERVICE_PER_DEV");
      c->csv_ok = per_dev <= ((spd && *spd) ? atoi(spd) : 2);
      c->proto = proto_default(c);   // the same on every rank: xdev is symmetric, the env is job-wide
    }
    for (int p = 0; ok && p < size; p++) {
      if (p == rank) {
        c->peer_staging[p] = c->staging;
        c->peer_flags[p] = c->flagmem;
        c->peer_hregion[p] = c->hregion;
        continue;
      }
      if (hipIpcOpenMemHandle((void **)&c->peer_staging[p], all[p].staging, hipIpcMemLazyEnablePeerAccess) !=
              hipSuccess ||
          hipIpcOpenMemHandle((void **)&c->peer_flags[p], all[p].flags, hipIpcMemLazyEnablePeerAccess) !=
              hipSuccess ||
          (c->hregion &&
           hipIpcOpenMemHandle((void **)&c->peer_hregion[p], all[p].hregion, hipIpcMemLazyEnablePeerAccess) !=
               hipSuccess)) {
        fprintf(stderr, "mx_comm_create: rank %d cannot map rank %d's staging\n", rank, p);
        (void)hipGetLastError();
        ok = 0;
      }
    }
    // every mapping shows its owner's signature (a wrong IPC mapping fails
    // creation here instead of corrupting data later)
    for (int p = 0; ok && p < size; p++) {
      uint64_t v[2] = {0, 0};
      if (hipMemcpyAsync(v, c->peer_flags[p] + FLAG_WORDS, 8, hipMemcpyDeviceToHost, ls) != hipSuccess ||
          (c->hregion && hipMemcpyAsync(v + 1, c->peer_hregion[p], 8, hipMemcpyDeviceToHost, ls) != hipSuccess) ||
          hipStreamSynchronize(ls) != hipSuccess || v[0] != 0x5EED0000ull + (uint64_t)p ||
          (c->hregion && v[1] != 0x5EED1000ull + (uint64_t)p)) {
        fprintf(stderr, "mx_comm_create: rank %d: mapping of rank %d shows 0x%llx/0x%llx\n", rank, p,
                (unsigned long long)v[0], (unsigned long long)v[1]);
        ok = 0;
      }
    }
    // exchange 2: every rank mapped every peer (doubles as the barrier)
    const int all_ok = agree(ag, ctx, size, ok);
    if (all_ok != 1) {
      if (rank == 0 && mine.shm[0]) shm_unlink(mine.shm);
      mx_comm_destroy(c);
      return all_ok < 0 ? MX_ERR_HIP : MX_ERR_STATE;
    }
    // registration: available only if every rank mapped the page
    const int reg_all = agree(ag, ctx, size, c->reg_shm != nullptr);
    if (rank == 0 && mine.shm[0]) shm_unlink(mine.shm);
    if (reg_all == 1) {
      c->reg_min = reg_min();
      c->reg_imp = new (std::nothrow) std::vector<mx_reg_import>();
      c->reg_gone = new (std::nothrow) std::vector<IpcGone>();
      // autotuning unless switched off, or a data path is forced through the environment
      const char *at = getenv("MX_AUTOTUNE");
      c->tune_on = !(at && *at == '0') && !getenv("MX_ALLREDUCE_PROTO") && !getenv("MX_REG_MIN");
    }
    if (reg_all != 1 || !c->reg_imp || !c->reg_gone) reg_release(c);
    c->live = 1;
    const char *lr = getenv("MX_DEBUG_LAG_RANK"), *lu = getenv("MX_DEBUG_LAG_US");
    if (lr && lu && atoi(lr) == rank) c->lag_ticks = ticks_for(atof(lu) * 1e-6);
  } else {
    const int all_ok = agree(ag, ctx, size, ok);
    if (all_ok != 1) {
      mx_comm_destroy(c);
      return all_ok < 0 ? MX_ERR_HIP : MX_ERR_STATE;
    }
  }
  if (flags & MX_COMM_RCCL) {
    // every rank reached here (the verdicts above agreed), so the RCCL
    // bootstrap is entered by all of them
    ncclUniqueId id, *ids = (ncclUniqueId *)calloc(size, sizeof(ncclUniqueId));
    memset(&id, 0, sizeof id);
    ok = ids != nullptr && (rank != 0 || ncclGetUniqueId(&id) == ncclSuccess);
    ncclUniqueId dummy[1];
    if (ag(&id, ids ? ids : dummy, ids ? sizeof(id) : 0, ctx) != 0) ok = 0;
    if (ok) {
      id = ids[0];
      if (ncclCommInitRank(&c->nccl, size, id, rank) != ncclSuccess) {
        c->nccl = nullptr;
        ok = 0;
      }
    }
    free(ids);
    rc = agree(ag, ctx, size, ok);
    if (rc != 1) {
      mx_comm_destroy(c);
      return rc < 0 ? MX_ERR_HIP : MX_ERR_RCCL;
    }
  }
  live_add(c);
  *out = c;
  return MX_SUCCESS;
}

extern "C" int mx_comm_destroy(mx_comm_t *c) {
  if (!c) return MX_SUCCESS;
  csv_comm_gone(c);   // a resident service bound to this communicator leaves first
  // wait for this communicator's own work only -- its last deferred
  // collective (requests run in issue order behind the tail event) and its
  // point-to-point channels -- never for the whole device: another
  // communicator's request may be spinning on a peer that waits for this
  // rank's next step (example 2).  Blocking calls ended
  // before they returned.
  if (c->tail_valid && c->tail && hipEventSynchronize(c->tail) != hipSuccess) (void)hipGetLastError();
  p2p_quiesce(c);
  uint32_t peers = 0;
  if (c->live) {
    // this rank's last access to its peers' regions is over: say BYE to each
    // (their regions leave quarantine once every peer said it)
    const SignalArgs a = signal_args(c, BYE_BASE, 0);
    peers = all_ranks_mask(c->size) & ~(1u << c->rank);
    hipStream_t ls = life_stream();
    hipLaunchKernelGGL(k_bye, dim3(1), dim3(64), 0, ls, a);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ls) != hipSuccess) (void)hipGetLastError();
  }
  live_del(c);
  for (int p = 0; p < c->size && p < MAXR; p++) {
    if (p == c->rank) continue;
    release_later(c->peer_staging[p], REL_IPC);
    release_later(c->peer_flags[p], REL_IPC);
    release_later(c->peer_hregion[p], REL_IPC);
  }
  // creation failed (not live): a peer may have mapped the regions and will
  // never say BYE, so they stay allocated -- never reused, never freed under
  // a peer's mapping
  if (c->live || c->size == 1) ipc_regions_release(c->staging, c->hregion, c->flagmem, peers);
  pool_host_put(c->err_host, sizeof(int));
  pool_dev_put(c->poison, sizeof(int));
  if (c->nccl) ncclCommDestroy(c->nccl);
  if (c->prof)
    for (int i = 0; i < 64; i++) (void)hipEventDestroy(c->ev[i]);
  if (c->tail) (void)hipEventDestroy(c->tail);
  reg_release(c);
  p2p_release(c);
  xtable_free(c->xtab);   // waits for its slots' last launches, then returns them to the pools
  free(c);
  release_flush();
  return MX_SUCCESS;
}

// ---------------------------------------------------------------------------
// completion of a blocking call, ordering, and the fold launch
// ---------------------------------------------------------------------------
namespace {

// blocking completion: the mapped completion word (mx_stream_sync_fast)
// unless MX_FAST_SYNC=0 selects hipStreamSynchronize
static bool fast_sync() { static const bool v = env_default_on("MX_FAST_SYNC"); return v; }

// MX_DONE_SELF_MARK=0: a blocking staged / zero-copy collective ends with the
// marker kernel instead of its last DONE signal raising the completion word
// (n=2 on one GPU, 256 KiB - 4 MiB: 1.5-4 us of 23-30 us saved,
// profiles/r04/done_self_mark_ab.txt)
static bool done_self_mark() { static const bool v = env_default_on("MX_DONE_SELF_MARK"); return v; }

// A wait that timed out: one line per kind on stderr with this rank's
// generation and what every peer has raised in its flags, and the peers'
// registration-page sequence numbers -- enough to tell which peer stopped
// where (the communicator is poisoned after it; no kernel runs on it).
static void timeout_dump(mx_comm *c, const char *where) {
  if (!c || c->local || !c->flagmem) return;
  static std::atomic<int> dumps{0};
  if (dumps.fetch_add(1) >= 4) return;
  uint64_t f[NFLAGS * MAXR];
  hipStream_t ls = life_stream();
  if (hipMemcpyAsync(f, c->flagmem, sizeof f, hipMemcpyDeviceToHost, ls) != hipSuccess ||
      hipStreamSynchronize(ls) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  static const char *names[3] = {"READY", "PUSHED", "DONE"};
  fprintf(stderr, "mx: rank %d/%d timed out (%s), gen %llu\n", c->rank, c->size, where, (unsigned long long)c->gen);
  for (int k = 0; k < 3 && k < NFLAGS; k++) {
    char line[512];
    int o = snprintf(line, sizeof line, "mx:   %-6s from peers:", names[k]);
    for (int p = 0; p < c->size && o < (int)sizeof line - 24; p++)
      o += snprintf(line + o, sizeof line - o, " %llu", (unsigned long long)f[k * MAXR + p]);
    fprintf(stderr, "%s\n", line);
  }
  if (c->reg_shm) {
    const RegRec *R = (const RegRec *)c->reg_shm;   // both banks: calls of either parity
    const int n = c->size;
    char line[512];
    int o = snprintf(line, sizeof line, "mx:   reg seq/vseq:");
    for (int p = 0; p < n && o < (int)sizeof line - 60; p++)
      o += snprintf(line + o, sizeof line - o, " %llu/%llu|%llu/%llu", (unsigned long long)R[p].seq.load(),
                    (unsigned long long)R[p].vseq.load(), (unsigned long long)R[n + p].seq.load(),
                    (unsigned long long)R[n + p].vseq.load());
    fprintf(stderr, "%s (mine %llu)\n", line, (unsigned long long)c->reg_seq);
  }
}

// mk: the completion flags the last kernel raises itself (mark_arm(&mk,
// true) before its launch), else the marker kernel
static int finish(mx_comm *c, hipStream_t s, const Mark *mk = nullptr) {
  if (c->defer) return MX_SUCCESS;   // request path: completion through the request's event
  if (mx::p2p_rx_active()) {
    // receives of this process are in flight: a peer may be in a blocking
    // send that waits for one of them to be launched again after a yield
    // (mx_p2p.hip) before it joins this collective, so the wait
    // polls the stream and progresses them instead of blocking
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      mx::p2p_progress();
      const hipError_t e = hipStreamQuery(s);
      if (e == hipSuccess) break;
      if (e != hipErrorNotReady) return MX_ERR_HIP;
      if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > 2000.0)
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  } else if (mk && (mk->flags || mk->word)) {
    if (mark_wait(*mk, s) != MX_SUCCESS) return MX_ERR_HIP;
  } else if (fast_sync() ? mx_stream_sync_fast(s) != MX_SUCCESS : hipStreamSynchronize(s) != hipSuccess) {
    return MX_ERR_HIP;
  }
  c->tail_valid = 0;                 // everything enqueued before is done
  if (!c->pending) prof_collect(c);
  if (c->err_host && *(volatile int *)c->err_host) {
    int e = *(volatile int *)c->err_host;
    *c->err_host = 0;
    if (e == MX_ERR_TIMEOUT) {
      c->poisoned = e;   // sticky: the device side is poisoned too
      timeout_dump(c, "device wait");
    }
    return e;
  }
  return MX_SUCCESS;
}

// A collective about to be enqueued on `s` waits for the previous deferred
// collective of the communicator when that one went to another stream.
static int order(mx_comm *c, hipStream_t s) {
  if (c->poisoned) return c->poisoned;   // a peer wait timed out earlier: nothing more on this communicator
  if (c->tail_valid && c->tail_stream != s && hipStreamWaitEvent(s, c->tail, 0) != hipSuccess) return MX_ERR_HIP;
  return MX_SUCCESS;
}

static int run_fold(mx_comm *c, fold_launch_fn fl, const Seg &sg, size_t part_lo, const char *const *src_base,
                    int nsrc, char *const *dst_base, int ndst, size_t es, hipStream_t s, bool nt_force = false) {
  // src_base / dst_base point at element part_lo of each operand/destination
  FoldArgs a;
  memset(&a, 0, sizeof a);
  const size_t shift = (sg.lo - part_lo) * es;
  for (int j = 0; j < nsrc; j++) a.src[j] = src_base[j] + shift;
  for (int d = 0; d < ndst; d++) a.dst[d] = dst_base[d] + shift;
  a.ndst = ndst;
  a.n = sg.hi - sg.lo;
  a.p = sg.p;
  a.poison = c ? c->poison : nullptr;
  a.nt_force = nt_force;
  lag_launch(c, s);   // tests only
  prof_begin(c, s);
  const int rc = fl(a, s);
  prof_end(c, s, 0, (double)(nsrc + ndst) * (double)a.n * (double)es);
  return rc;
}

}  // namespace

// ---------------------------------------------------------------------------
// local communicators: all ranks' buffers in this process
// ---------------------------------------------------------------------------
extern "C" int mx_allreduce_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs, size_t count,
                                  int type, int op, int alg, void *stream) {
  if (!c || !c->local || !rbufs) return MX_ERR_ARG;
  fold_launch_fn fl = fold_fns(op, type).fold;
  if (!fl) return MX_ERR_UNSUPPORTED;
  const size_t es = type_size(type);
  const int n = c->size;
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  if (count == 0) return MX_SUCCESS;
  const char *src[MAXR];
  char *dst[MAXR];
  for (int j = 0; j < n; j++) {
    const void *sb = (sbufs && sbufs[j] != MX_IN_PLACE) ? sbufs[j] : rbufs[j];
    src[j] = (const char *)sb;
    dst[j] = (char *)rbufs[j];
  }
  if (n == 1) {
    if (int rc = copy_async(dst[0], src[0], count * es, s)) return rc;
    return finish(c, s);
  }
  if ((alg & 0xff) == MX_ALLREDUCE_NONOVERLAPPING) {
    // coll_base_allreduce.c:54-86: coll_reduce to rank 0 (rank 0 passes
    // MPI_IN_PLACE when the call is in place), then coll_bcast from 0
    const void *sb2[MAXR];
    for (int j = 0; j < n; j++) sb2[j] = (sbufs && sbufs[j] != MX_IN_PLACE) ? sbufs[j] : (j ? rbufs[j] : MX_IN_PLACE);
    if (int rc = mx_reduce_local(c, sb2, rbufs, count, type, op, 0, reduce_word_of(alg), stream)) return rc;
    return mx_bcast_local(c, rbufs, count * es, 0, stream);
  }
  size_t off[MAXR], len[MAXR];
  blockcount(count, n, off, len);
  for (int p = 0; p < n; p++) {
    std::vector<Seg> segs;
    int rc = allreduce_segments(alg & 0xff, n, count, es, off[p], off[p] + len[p], segs);
    if (rc) return rc;
    const char *sp[MAXR];
    char *dp[MAXR];
    for (int j = 0; j < n; j++) { sp[j] = src[j] + off[p] * es; dp[j] = dst[j] + off[p] * es; }
    for (const Seg &sg : segs) {
      rc = run_fold(c, fl, sg, off[p], sp, n, dp, n, es, s);
      if (rc) return rc;
    }
  }
  return finish(c, s);
}

// reduce_scatter NONOVERLAPPING (coll_base_reduce_scatter.c:47-110): the
// rooted reduce DAG to rank 0, every rank folding its own block of it
// (defined with the fold VM below)
static int rs_nonoverlapping(mx_comm *c, const char *sb, char *rb, const size_t *rcounts, int type, int op, int alg,
                             bool allow_zc, hipStream_t s);
static int rs_nonoverlapping_local(mx_comm *c, const char *const *src, void *const *rbufs, const size_t *rcounts,
                                   int type, int op, int alg, bool inplace, hipStream_t s);

extern "C" int mx_reduce_scatter_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs,
                                       const size_t *rcounts, int type, int op, int alg, void *stream) {
  if (!c || !c->local || !rbufs || !rcounts) return MX_ERR_ARG;
  fold_launch_fn fl = fold_fns(op, type).fold;
  if (!fl) return MX_ERR_UNSUPPORTED;
  const size_t es = type_size(type);
  const int n = c->size;
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  size_t disp[MAXR], total = 0;
  for (int j = 0; j < n; j++) { disp[j] = total; total += rcounts[j]; }
  const char *src[MAXR];
  for (int j = 0; j < n; j++) {
    const void *sb = (sbufs && sbufs[j] != MX_IN_PLACE) ? sbufs[j] : rbufs[j];
    src[j] = (const char *)sb;
  }
  if (n == 1) {
    if (int rc = copy_async(rbufs[0], src[0], total * es, s)) return rc;
    return finish(c, s);
  }
  if ((alg & 0xff) == MX_RS_NONOVERLAPPING)
    return rs_nonoverlapping_local(c, src, rbufs, rcounts, type, op, alg, !sbufs || sbufs[0] == MX_IN_PLACE, s);
  alg &= 0xff;
  // IN_PLACE (or rbuf aliasing sbuf): rank p's result lands at rbufs[p][0..)
  // while other blocks of rbufs[p] are still inputs, so results go to a
  // temporary laid out like the full vector and are copied back at the end.
  bool any_alias = false;
  for (int p = 0; p < n; p++)
    if ((const char *)rbufs[p] == src[p]) any_alias = true;
  char *tmp = nullptr;
  if (any_alias && hipMallocAsync((void **)&tmp, total * es + 16, s) != hipSuccess) return MX_ERR_NOMEM;
  for (int p = 0; p < n; p++) {
    if (!rcounts[p]) continue;
    std::vector<Seg> segs;
    int rc = reduce_scatter_segments(alg, n, rcounts, es, p, segs);
    if (rc) return rc;
    const char *sp[MAXR];
    for (int j = 0; j < n; j++) sp[j] = src[j] + disp[p] * es;
    char *dp[1] = {tmp ? tmp + disp[p] * es : (char *)rbufs[p]};
    for (const Seg &sg : segs)
      if ((rc = run_fold(c, fl, sg, disp[p], sp, n, dp, 1, es, s))) return rc;
  }
  if (tmp) {
    CopyArgs ca;
    memset(&ca, 0, sizeof ca);
    for (int p = 0; p < n; p++)
      if (rcounts[p]) ca.j[ca.n++] = CopyJob{tmp + disp[p] * es, (char *)rbufs[p], rcounts[p] * es};
    int rc = copy_launch(c, ca, s);
    (void)hipFreeAsync(tmp, s);
    if (rc) return rc;
  }
  return finish(c, s);
}

extern "C" int mx_allgather_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs, size_t bytes,
                                  void *stream) {
  if (!c || !c->local || !rbufs) return MX_ERR_ARG;
  const int n = c->size;
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  if (!bytes) return MX_SUCCESS;
  // all-peer: rank j's block goes to every rank in one launch per source
  for (int j = 0; j < n; j++) {
    const char *sb = (sbufs && sbufs[j] != MX_IN_PLACE) ? (const char *)sbufs[j]
                                                        : (const char *)rbufs[j] + (size_t)j * bytes;
    CopyArgs a;
    memset(&a, 0, sizeof a);
    for (int r = 0; r < n; r++) {
      char *d = (char *)rbufs[r] + (size_t)j * bytes;
      if (d == sb) continue;
      a.j[a.n++] = CopyJob{sb, d, bytes};
    }
    int rc = copy_launch(c, a, s);
    if (rc) return rc;
  }
  return finish(c, s);
}

extern "C" int mx_bcast_local(mx_comm_t *c, void *const *bufs, size_t bytes, int root, void *stream) {
  if (!c || !c->local || !bufs || root < 0 || root >= c->size) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  if (!bytes) return MX_SUCCESS;
  CopyArgs a;
  memset(&a, 0, sizeof a);
  for (int r = 0; r < c->size; r++)
    if (r != root) a.j[a.n++] = CopyJob{(const char *)bufs[root], (char *)bufs[r], bytes};
  int rc = copy_launch(c, a, s);
  if (rc) return rc;
  return finish(c, s);
}

// Exchanges: the n x n jobs of the call in ONE launch of k_exchange
// (mx_exchange.hip).  Jobs are listed source by source, so neighbours in the
// table go to different ranks.
extern "C" int mx_alltoallv_local(mx_comm_t *c, const void *const *sbufs, const size_t *sbytes, const size_t *soffs,
                                  void *const *rbufs, const size_t *rbytes, const size_t *roffs, void *stream) {
  if (!c || !c->local || !rbufs || !rbytes || !roffs) return MX_ERR_ARG;
  const int n = c->size;
  const bool inplace = !sbufs || sbufs[0] == MX_IN_PLACE;
  if (!inplace && (!sbytes || !soffs)) return MX_ERR_ARG;
  for (int i = 0; i < n; i++) {
    if (int rc = xcheck_row(n, rbytes + (size_t)i * n, roffs + (size_t)i * n)) return rc;
    if (!inplace && xcheck_row(n, sbytes + (size_t)i * n, soffs + (size_t)i * n)) return MX_ERR_ARG;
    if (inplace && !xranges_disjoint(n, rbytes + (size_t)i * n, roffs + (size_t)i * n)) return MX_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  xcount(c, 0);
  std::vector<XJob> jobs;
  jobs.reserve((size_t)n * n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const size_t ij = (size_t)i * n + j, ji = (size_t)j * n + i;
      const size_t len = std::min(inplace ? rbytes[ij] : sbytes[ij], rbytes[ji]);   // never past the receiver's size
      const char *src = inplace ? (const char *)rbufs[i] + roffs[ij] : (const char *)sbufs[i] + soffs[ij];
      char *dst = (char *)rbufs[j] + roffs[ji];
      if (len && src != dst) jobs.push_back(XJob{src, dst, len});
    }
  if (jobs.size() > (size_t)kXInline && !c->xtab) c->xtab = xtable_new();   // null: launches of kXInline jobs
  char *tmp = nullptr;
  int rc = MX_SUCCESS;
  if (inplace && !jobs.empty()) {
    // every range is read and overwritten by the same launch: the sent
    // ranges go through a temporary copy first (each keeps its misalignment)
    size_t total = 0;
    std::vector<XJob> first = jobs;
    for (XJob &jb : first) total += (jb.bytes + 15) / 16 * 16 + 16;
    if (hipMallocAsync((void **)&tmp, total, s) != hipSuccess) return MX_ERR_NOMEM;
    size_t o = 0;
    for (size_t q = 0; q < jobs.size(); q++) {
      first[q].dst = tmp + o + ((uintptr_t)jobs[q].src & 15);
      jobs[q].src = first[q].dst;
      o += (jobs[q].bytes + 15) / 16 * 16 + 16;
    }
    rc = exchange_launch(first.data(), first.size(), c->poison, s, c->xtab);
  }
  if (!rc) rc = exchange_launch(jobs.data(), jobs.size(), c->poison, s, c->xtab);
  if (tmp) (void)hipFreeAsync(tmp, s);
  if (rc) return rc;
  return finish(c, s);
}

extern "C" int mx_alltoall_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs, size_t bytes,
                                 void *stream) {
  if (!c || !c->local) return MX_ERR_ARG;
  const int n = c->size;
  if ((size_t)n * bytes / (size_t)n != bytes) return MX_ERR_ARG;
  std::vector<size_t> len((size_t)n * n, bytes), off((size_t)n * n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) off[(size_t)i * n + j] = (size_t)j * bytes;
  return mx_alltoallv_local(c, sbufs, len.data(), off.data(), rbufs, len.data(), off.data(), stream);
}

extern "C" int mx_allgatherv_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs, const size_t *rbytes,
                                   const size_t *roffs, void *stream) {
  if (!c || !c->local || !rbufs) return MX_ERR_ARG;
  const int n = c->size;
  if (int rc = xcheck_row(n, rbytes, roffs)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  xcount(c, 0);
  std::vector<XJob> jobs;
  jobs.reserve((size_t)n * n);
  for (int i = 0; i < n; i++) {
    const char *src = (sbufs && sbufs[i] != MX_IN_PLACE) ? (const char *)sbufs[i] : (const char *)rbufs[i] + roffs[i];
    for (int j = 0; j < n; j++) {
      char *dst = (char *)rbufs[j] + roffs[i];
      if (rbytes[i] && src != dst) jobs.push_back(XJob{src, dst, rbytes[i]});
    }
  }
  if (jobs.size() > (size_t)kXInline && !c->xtab) c->xtab = xtable_new();
  if (int rc = exchange_launch(jobs.data(), jobs.size(), c->poison, s, c->xtab)) return rc;
  return finish(c, s);
}

// ---- the strided forms (k_exchange_vec, mx_exchange_vec.hip) -----------------
// a pointer moved by a signed byte offset kept modulo 2^64
static inline char *padd(const char *p, uint64_t off) { return (char *)((uintptr_t)p + (uintptr_t)off); }
// One side of a call: the layout the kernel reads or writes by, the stream
// bytes and the extent of one instance.  A NULL datatype is bytes.
struct XDSide {
  XLay lay;
  size_t size;
  int64_t ext;
  const DdtLayout *L;
  bool ok;   // the datatype qualifies (mx_ddt_strided)
};
static XDSide xd_side(const mx_ddt_t *d, bool receive_side) {
  XDSide sd{xlay_flat(), 1, 1, nullptr, true};
  if (!d) return sd;
  sd.ok = false;
  if (d == MX_DDT_NONE) return sd;
  sd.L = ddt_layout(d);
  sd.size = sd.L->size;
  sd.ext = sd.L->ub - sd.L->lb;
  sd.ok = sd.size && xlay_from(*sd.L, receive_side, &sd.lay);
  return sd;
}
// widens [*lo, *hi) by the bytes `count` instances `displ` extents in touch
static void xd_span(const XDSide &sd, size_t count, int64_t displ, int64_t *lo, int64_t *hi) {
  if (!count) return;
  int64_t a = 0, b = (int64_t)count;
  if (sd.L) ddt_span(*sd.L, count, &a, &b);
  *lo = std::min(*lo, a + displ * sd.ext);
  *hi = std::max(*hi, b + displ * sd.ext);
}
// the access unit of one rank's side: layout, address, every block's offset and length
static unsigned xd_unit(const XDSide &sd, const void *buf, int n, const size_t *counts, const int64_t *displs) {
  unsigned u = xlay_unit(sd.lay, (uintptr_t)buf);
  for (int p = 0; p < n; p++) {
    if (!counts[p]) continue;
    u = xunit_of(xabs(displs[p] * sd.ext), u);
    u = xunit_of((uint64_t)counts[p] * sd.size, u);
  }
  return u;
}
static bool xd_counts_ok(const XDSide &sd, int n, const size_t *counts) {
  for (int p = 0; p < n; p++)
    if (sd.size && counts[p] > (((size_t)1 << 47) / sd.size)) return false;
  return true;
}

extern "C" int mx_alltoallv_ddt_local(mx_comm_t *c, const void *const *sbufs, const size_t *scounts,
                                      const int64_t *sdispls, const mx_ddt_t *sddt, void *const *rbufs,
                                      const size_t *rcounts, const int64_t *rdispls, const mx_ddt_t *rddt,
                                      void *stream) {
  if (!c || !c->local || !rbufs || !rcounts || !rdispls) return MX_ERR_ARG;
  const int n = c->size;
  const bool inplace = !sbufs || sbufs[0] == MX_IN_PLACE;
  if (inplace) { scounts = rcounts; sdispls = rdispls; sddt = rddt; }   // the receive description serves both sides
  else if (!scounts || !sdispls) return MX_ERR_ARG;
  const XDSide S = xd_side(sddt, false), R = xd_side(rddt, true);
  if (!S.ok || !R.ok) return MX_ERR_UNSUPPORTED;
  if (!xd_counts_ok(S, n * n, scounts) || !xd_counts_ok(R, n * n, rcounts)) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  // every job is planned before any is launched: a word below 4 bytes anywhere declines the call
  std::vector<XVJob> jobs, first;
  std::vector<size_t> tmp_off;
  size_t total = 0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const size_t ij = (size_t)i * n + j, ji = (size_t)j * n + i;
      const size_t len = std::min(scounts[ij] * S.size, rcounts[ji] * R.size);   // never past the receiver's room
      if (!len || (inplace && i == j)) continue;
      const char *src = padd((const char *)(inplace ? rbufs[i] : sbufs[i]), (uint64_t)(sdispls[ij] * S.ext));
      char *dst = padd((const char *)rbufs[j], (uint64_t)(rdispls[ji] * R.ext));
      XVJob jb;
      int rc;
      if (inplace) {
        // every block is read and overwritten by the same call: the sent
        // blocks go through a flat temporary first (offsets known after the loop)
        XVJob f;
        if ((rc = xvjob_make(src, S.lay, 0, (char *)(uintptr_t)16, xlay_flat(), 0, len, &f))) return rc;
        if ((rc = xvjob_make((const char *)(uintptr_t)16, xlay_flat(), 0, dst, R.lay, 0, len, &jb))) return rc;
        first.push_back(f);
        tmp_off.push_back(total);
        total += (len + 255) & ~(size_t)255;
      } else if ((rc = xvjob_make(src, S.lay, 0, dst, R.lay, 0, len, &jb))) {
        return rc;
      }
      jobs.push_back(jb);
    }
  if (int orc = order(c, s)) return orc;
  xcount(c, 0, true);
  char *tmp = nullptr;
  int rc = MX_SUCCESS;
  if (inplace && !jobs.empty()) {
    if (hipMallocAsync((void **)&tmp, total, s) != hipSuccess) return MX_ERR_NOMEM;
    for (size_t q = 0; q < jobs.size(); q++) {
      first[q].dst = tmp + tmp_off[q];
      jobs[q].src = tmp + tmp_off[q];
    }
    rc = exchange_vec_launch(first.data(), first.size(), c->poison, s);
  }
  if (!rc) rc = exchange_vec_launch(jobs.data(), jobs.size(), c->poison, s);
  if (tmp) (void)hipFreeAsync(tmp, s);
  if (rc) return rc;
  return finish(c, s);
}

extern "C" int mx_alltoall_ddt_local(mx_comm_t *c, const void *const *sbufs, size_t scount, const mx_ddt_t *sddt,
                                     void *const *rbufs, size_t rcount, const mx_ddt_t *rddt, void *stream) {
  if (!c || !c->local) return MX_ERR_ARG;
  const int n = c->size;
  std::vector<size_t> sc((size_t)n * n, scount), rc((size_t)n * n, rcount);
  std::vector<int64_t> sd((size_t)n * n), rd((size_t)n * n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      sd[(size_t)i * n + j] = (int64_t)j * (int64_t)scount;
      rd[(size_t)i * n + j] = (int64_t)j * (int64_t)rcount;
    }
  return mx_alltoallv_ddt_local(c, sbufs, sc.data(), sd.data(), sddt, rbufs, rc.data(), rd.data(), rddt, stream);
}

extern "C" int mx_comm_exchange_ddt_stats(mx_comm_t *c, uint64_t out[4]) {
  if (!out) return MX_ERR_ARG;
  for (int k = 0; k < 4; k++) out[k] = c ? c->xdst[k] : g_xdst[k].load(std::memory_order_relaxed);
  return MX_SUCCESS;
}

extern "C" int mx_comm_exchange_stats(mx_comm_t *c, uint64_t out[4]) {
  if (!out) return MX_ERR_ARG;
  for (int k = 0; k < 4; k++) out[k] = c ? c->xst[k] : g_xst[k].load(std::memory_order_relaxed);
  return MX_SUCCESS;
}

// ---------------------------------------------------------------------------
// multi-process all-peer path (IPC staging + flags)
// ---------------------------------------------------------------------------
namespace {

// mk: the blocking call's completion word, raised by this signal as the
// call's last kernel (finish then waits for it instead of a marker kernel)
static int signal_all(mx_comm *c, int kind, uint64_t value, hipStream_t s, const Mark *mk = nullptr) {
  SignalArgs a = signal_args(c, kind * MAXR, value);
  a.poison = c->poison;
  if (mk && mk->word) {
    a.mark = mk->word;
    a.mark_v = mk->v;
  }
  hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, s, a);
  return mx_check_launch();
}

// A blocking call's completion word raised by its last DONE signal (the
// call's last kernel): armed at the start of the call, attached to the final
// signal only, and used by finish only if that signal went out.
struct DoneMark {
  Mark mk{nullptr, nullptr, 0};
  bool sent = false;
};
static void done_mark_arm(mx_comm *c, DoneMark &d) {
  if (c && !c->defer && fast_sync() && done_self_mark()) mark_arm(&d.mk, false);
}
static int signal_done(mx_comm *c, uint64_t value, hipStream_t s, DoneMark *last) {
  const Mark *mk = last && last->mk.word ? &last->mk : nullptr;
  const int rc = signal_all(c, FLAG_DONE, value, s, mk);
  if (!rc && mk) last->sent = true;
  return rc;
}
static int finish_done(mx_comm *c, hipStream_t s, const DoneMark &d) { return finish(c, s, d.sent ? &d.mk : nullptr); }

// signal_all(kind, svalue) + wait_all(kind, wvalue) as one launch
static int signal_wait_all(mx_comm *c, int kind, uint64_t svalue, uint64_t wvalue, hipStream_t s) {
  SignalArgs a = signal_args(c, kind * MAXR, svalue);
  a.poison = c->poison;
  const uint32_t all = all_ranks_mask(c->size);
  hipLaunchKernelGGL(k_signal_wait, dim3(kWaitBlocks), dim3(64), 0, s, a, (const uint64_t *)(c->flagmem + kind * MAXR),
                     all & ~(1u << c->rank), wvalue, c->timeout_ticks, c->err_dev, c->poison);
  return mx_check_launch();
}

// signal_all(kind, value), then a wait for the same value from the ranks in `mask` only
static int signal_wait_mask(mx_comm *c, int kind, uint64_t value, uint32_t mask, hipStream_t s) {
  if (!mask) return signal_all(c, kind, value, s);
  SignalArgs a = signal_args(c, kind * MAXR, value);
  a.poison = c->poison;
  hipLaunchKernelGGL(k_signal_wait, dim3(kWaitBlocks), dim3(64), 0, s, a, (const uint64_t *)(c->flagmem + kind * MAXR),
                     mask & ~(1u << c->rank), value, c->timeout_ticks, c->err_dev, c->poison);
  return mx_check_launch();
}

static int wait_mask(mx_comm *c, int kind, uint32_t mask, uint64_t value, hipStream_t s) {
  hipLaunchKernelGGL(k_wait, dim3(kWaitBlocks), dim3(64), 0, s, (const uint64_t *)(c->flagmem + kind * MAXR), mask, value,
                     c->timeout_ticks, c->err_dev, c->poison);
  return mx_check_launch();
}
static int wait_all(mx_comm *c, int kind, uint64_t value, hipStream_t s) {
  const uint32_t all = all_ranks_mask(c->size);
  return wait_mask(c, kind, all & ~(1u << c->rank), value, s);
}

static inline size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

// staging layout for a chunk of `ce` elements of size es
struct Layout { size_t slot, gather_off; };
// gather_only: the contributions are read where they are (registered user
// buffers), so the staging holds only the gather area
static Layout layout_for(int n, size_t ce, size_t es, bool gather_only = false) {
  Layout L;
  L.slot = gather_only ? 0 : rup((ce + n - 1) / n * es + 16, 256);
  L.gather_off = rup(L.slot * n, 256);
  return L;
}
static size_t chunk_elems(const mx_comm *c, size_t count, size_t es, bool gather_only = false) {
  const int n = c->size;
  auto fits = [&](size_t ce) {
    const Layout L = layout_for(n, ce, es, gather_only);
    return L.gather_off + ce * es + 16 <= c->main_bytes;
  };
  if (fits(count)) return count;
  // n slots of ce/n elements + a gather area of ce elements, plus padding
  size_t ce = c->main_bytes > (size_t)(n + 2) * 512 ? (c->main_bytes - (size_t)(n + 2) * 512) / ((gather_only ? 1 : 2) * es)
                                                    : 1;
  if (ce >= count) ce = count - 1;
  while (ce > 1 && !fits(ce)) ce -= std::max<size_t>(1, ce / 64);
  return ce ? ce : 1;
}

// MX_OS_SELF_MARK=0: a blocking one-shot allreduce ends with the marker
// kernel instead of raising its own completion flags (A/B switch)
static bool os_self_mark() { static const bool v = env_default_on("MX_OS_SELF_MARK"); return v; }

// a call the resident service completed: nothing is pending on the stream;
// the device side's error word as finish() reports it
static int finish_served(mx_comm *c) {
  if (c->err_host && *(volatile int *)c->err_host) {
    const int e = *(volatile int *)c->err_host;
    *c->err_host = 0;
    if (e == MX_ERR_TIMEOUT) {
      c->poisoned = e;
      timeout_dump(c, "device wait (service)");
    }
    return e;
  }
  return MX_SUCCESS;
}

// one-shot allreduce (small messages): one kernel, see k_oneshot
static int allreduce_oneshot(mx_comm *c, oneshot_launch_fn ol, const std::vector<Seg> &segs, const char *sb,
                             char *rb, size_t count, size_t es, hipStream_t s, int op, int type) {
  const int n = c->size, r = c->rank;
  const uint64_t g = ++c->gen;
  const size_t bytes = count * es;
  // tagged words (os_ll in mx_fold.hpp) for one-workgroup calls of 4- and
  // 8-byte elements: decided from size and type alone, so every rank agrees
  const bool ll = (es == 4 || es == 8) && bytes <= c->os_ll;
  const size_t sub = ll ? c->os_cap + 256 : 0;   // the slot's LL area
  char *const region = c->staging + c->main_bytes + (g & 1) * (size_t)n * c->os_slot;
  OneShotArgs a;
  memset(&a, 0, sizeof a);
  a.sb = sb;
  a.rb = rb;
  a.ll = ll;
  for (int p = 0; p < n; p++) {
    const size_t peer_region = c->main_bytes + (g & 1) * (size_t)n * c->os_slot;
    a.peer_slot[p] = p == r ? nullptr : c->peer_staging[p] + peer_region + (size_t)r * c->os_slot + sub;
    a.src[p] = p == r ? sb : region + (size_t)p * c->os_slot + sub;
    a.peer_ready[p] = p == r ? nullptr : c->peer_flags[p] + OS_FLAG_BASE + (size_t)r * OSWG;
    a.peer_done[p] = p == r ? nullptr : c->peer_flags[p] + FLAG_DONE * MAXR + r;
  }
  a.my_ready = c->flagmem + OS_FLAG_BASE;
  a.my_done = c->flagmem + FLAG_DONE * MAXR;
  a.counter = c->flagmem + OS_COUNTER;
  a.gen = g;
  a.timeout_ticks = c->timeout_ticks;
  a.err = c->err_dev;
  a.poison = c->poison;
  a.n = n;
  a.rank = r;
  a.count = count;
  a.es = es;
  // slices of ~4 KiB, 16-byte aligned when the element size allows
  size_t nwg = std::min<size_t>(OSWG, std::max<size_t>(1, (bytes + 4095) / 4096));
  size_t slice = (count + nwg - 1) / nwg;
  if (16 % es == 0) slice = rup(slice, 16 / es);
  nwg = (count + slice - 1) / slice;
  if (ll) {   // one workgroup per OS_LL_MAX bytes; a single one needs no completion counter
    slice = OS_LL_MAX / es;
    nwg = (count + slice - 1) / slice;
    if (nwg == 1) slice = count;
  }
  a.slice = slice;
  a.counter_last = c->os_count + nwg - 1;
  if (!ll || nwg > 1) c->os_count += nwg;
  a.nseg = (int)segs.size();
  for (size_t i = 0; i < segs.size(); i++) a.seg[i] = OsSeg{segs[i].lo, segs[i].hi, segs[i].p};
  // the resident service takes the call when it can (the same arguments and
  // protocol: peers cannot tell), else the launch below
  if (!c->defer) {
    const int sv = csv_allreduce(c, a, op, type, s);
    if (sv < 0) return sv;
    if (sv == 1) {
      c->st.service_calls++;
      return finish_served(c);
    }
  }
  Mark mk{nullptr, nullptr, 0};
  if (!c->defer && fast_sync() && os_self_mark()) mark_arm(&mk, true);
  a.mflags = mk.flags;
  a.mv = mk.v;
  prof_begin(c, s);
  int rc = ol(a, (int)nwg, s);
  prof_end(c, s, 0, (double)(n + 1) * (double)bytes);
  if (rc) return rc;
  return finish(c, s, &mk);
}

// Autotuning: publish this rank's elapsed time of a trial call, return the
// maximum over the ranks (the same on every rank, so every rank keeps the same
// choice).  Bounded by the communicator's wait timeout like reg_wait.
static int tune_exchange(mx_comm *c, double el, double *tmax) {
  RegRec *R = (RegRec *)c->reg_shm;
  const uint64_t k = ++c->tune_seq;
  R[c->rank].t = el;
  R[c->rank].tseq.store(k, std::memory_order_release);
  const auto t0 = std::chrono::steady_clock::now();
  double m = 0;
  for (int p = 0; p < c->size; p++) {
    unsigned spins = 0;
    while (R[p].tseq.load(std::memory_order_acquire) < k) {
      if (++spins > 256) {
        sched_yield();
        if (c->timeout_s > 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > c->timeout_s) {
          c->poisoned = MX_ERR_TIMEOUT;
          timeout_dump(c, "tuning exchange");
          return MX_ERR_TIMEOUT;
        }
      }
    }
    m = std::max(m, R[p].t);
  }
  *tmax = m;
  return MX_SUCCESS;
}

// Autotuning bookkeeping shared by the tuned collectives.  tune_pick: the
// candidate this call runs (-1: the defaults, untuned), *bucket its size
// class.  tune_done: after a successful call, record its time (trial calls
// exchange the max over ranks) and keep the fastest once every candidate ran.
enum { TUNE_ALLREDUCE = 0, TUNE_REDUCE_SCATTER = 1, TUNE_ALLGATHER = 2, TUNE_BCAST = 3 };
// smallest size class tuned per kind: allreduce and bcast cover their
// one-shot / direct crossovers, reduce_scatter and allgather the zero-copy one
static size_t tune_min(int kind) {
  return (kind == TUNE_ALLREDUCE || kind == TUNE_BCAST) ? kTuneMin : kTuneMinMove;
}
// trial calls per candidate: small calls are noisy, each runs 3 times and its
// fastest counts
static int tune_reps(int bucket) { return bucket < 22 ? 3 : 1; }
static int tune_pick(const mx_comm *c, int kind, size_t bytes, int ncand, int *bucket) {
  *bucket = -1;
  if (!c->tune_on || !c->reg_shm || c->defer || bytes < tune_min(kind)) return -1;
  const int b = 63 - __builtin_clzll((unsigned long long)bytes);
  *bucket = b;
  if (c->tune_best[kind][b]) return c->tune_best[kind][b] - 1;
  const int k = c->tune_calls[kind][b];
  return k == 0 ? 0 : (k - 1) % ncand;   // call 0 warms up (and maps the peers' buffers) on candidate 0
}
static int tune_done(mx_comm *c, int kind, int bucket, int cand, int ncand, double el) {
  if (cand < 0 || c->tune_best[kind][bucket]) return MX_SUCCESS;
  const int k = c->tune_calls[kind][bucket]++;
  if (k == 0) return MX_SUCCESS;
  double tmax = 0;
  if (int rc = tune_exchange(c, el, &tmax)) return rc;
  double &t = c->tune_t[kind][bucket][cand];
  if (k <= ncand || tmax < t) t = tmax;   // the first run of a candidate, or a faster one
  if (k == ncand * tune_reps(bucket)) {
    int best = 0;
    for (int i = 1; i < ncand; i++)
      if (c->tune_t[kind][bucket][i] < c->tune_t[kind][bucket][best]) best = i;
    c->tune_best[kind][bucket] = (int8_t)(best + 1);
  }
  return MX_SUCCESS;
}
static double secs_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
// zero-copy modes of the tuned data paths: never (a staged candidate), the
// default (calls of reg_min bytes and more), always (the zero-copy
// candidate, at any size; reg_min == 0 still switches zero-copy off)
enum { ZC_NEVER = 0, ZC_DEFAULT = 1, ZC_ALWAYS = 2 };
static bool zc_allowed(const mx_comm *c, int zc_mode, size_t bytes) {
  if (zc_mode == ZC_NEVER || !c->reg_shm || c->defer || !c->reg_min) return false;
  return zc_mode == ZC_ALWAYS || bytes >= c->reg_min;
}
// the zero-copy mode of a tuned call's candidate (0 is the zero-copy one)
static int zc_mode_of(int cand) { return cand < 0 ? ZC_DEFAULT : cand == 0 ? ZC_ALWAYS : ZC_NEVER; }

// the allocation holding [p, p+bytes): IPC handle, identity, offset of p.
// Handles of recent allocations are kept per process (the runtime buffer id
// tells a live allocation from one re-made at the same address).
static bool reg_export(const void *p, size_t bytes, RegBuf *b) {
  struct Exp { uint64_t base, size, id; hipIpcMemHandle_t h; };
  static std::mutex mu;
  static std::vector<Exp> recent;   // most recent last, at most 16
  void *base = nullptr;
  size_t size = 0;
  unsigned long long id = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess || !base ||
      (const char *)p + bytes > (const char *)base + size ||
      hipPointerGetAttribute(&id, HIP_POINTER_ATTRIBUTE_BUFFER_ID, (hipDeviceptr_t)base) != hipSuccess) {
    (void)hipGetLastError();   // clear only the error this call raised
    return false;
  }
  bool hit = false;
  {
    std::lock_guard<std::mutex> lk(mu);
    for (const Exp &e : recent)
      if (e.base == (uint64_t)(uintptr_t)base && e.size == size && e.id == id) {
        b->h = e.h;
        hit = true;
        break;
      }
  }
  if (!hit) {
    if (export_remade((uint64_t)(uintptr_t)base, size, id)) return false;
    if (hipIpcGetMemHandle(&b->h, base) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    std::lock_guard<std::mutex> lk(mu);
    if (recent.size() >= 16) recent.erase(recent.begin());
    recent.push_back(Exp{(uint64_t)(uintptr_t)base, size, id, b->h});
  }
  b->base = (uint64_t)(uintptr_t)base;
  b->size = size;
  b->id = id;
  b->off = (uint64_t)((const char *)p - (const char *)base);
  return true;
}

// peer p's allocation, mapped once and kept (LRU, kRegCachePerPeer per
// peer).  A cached mapping of an allocation the peer has since freed (same
// peer range, other buffer id) is closed before the new handle is opened,
// and the open is checked against the imports closed at that range
// (ipc_open_checked: the runtime may hand the closed import back -- then the
// call declines, every rank takes the staged path, and the next call tries
// again).  Closing is safe: no kernel of this communicator is in flight
// between blocking calls.
static char *reg_import(mx_comm *c, int p, const RegBuf &b, const RegBuf *own, int nown) {
  std::vector<mx_reg_import> &v = *c->reg_imp;
  for (mx_reg_import &m : v)
    if (m.peer == p && m.base == b.base && m.size == b.size && m.id == b.id) {
      m.used = ++c->reg_tick;
      return m.ptr;
    }
  size_t held = 0;
  bool closed = false;
  mx_reg_import old{};   // (diagnostic MX_REG_DIAG) the stale import closed here
  for (size_t i = 0; i < v.size();) {
    const mx_reg_import &m = v[i];
    if (m.peer == p && m.base < b.base + b.size && b.base < m.base + m.size) {   // overlaps: stale
      // the stale import must be closed before the new handle opens; while
      // another communicator's work is pending it stays in the cache and this
      // call declines (every rank falls back to the staged path), so the next
      // call finds it and tries again -- it is never dropped unclosed
      ipc_gone_add(*c->reg_gone, p, m.base, m.size, m.ptr);
      old = m;
      old.used = ipc_object_id(m.ptr);
      if (!release_now_or_keep(m.ptr, REL_IPC)) return nullptr;
      v.erase(v.begin() + (long)i);
      closed = true;
      continue;
    }
    held += m.peer == p;
    i++;
  }
  if (held >= kRegCachePerPeer) {
    size_t lru = (size_t)-1;
    for (size_t i = 0; i < v.size(); i++)
      if (v[i].peer == p && (lru == (size_t)-1 || v[i].used < v[lru].used)) lru = i;
    ipc_gone_add(*c->reg_gone, p, v[lru].base, v[lru].size, v[lru].ptr);
    release_later(v[lru].ptr, REL_IPC);
    v.erase(v.begin() + (long)lru);
  }
  char *ptr = nullptr;
  uint64_t oid = 0;
  const int oc = ipc_open_checked(&b.h, *c->reg_gone, p, b.base, b.size, &ptr, &oid);
  if (oc <= 0) {
    if (oc == 0) c->st.reg_stale_refused++;
    return nullptr;
  }
  static const bool diag = env_default_off("MX_REG_DIAG");
  if (diag && closed)
    fprintf(stderr, "[mx diag] rank %d call %llu peer %d: re-made base %#llx id %llu->%llu handle %s ptr %p->%p oid %llu->%llu\n",
            c->rank, (unsigned long long)c->reg_seq, p, (unsigned long long)b.base, (unsigned long long)old.id,
            (unsigned long long)b.id, memcmp(old.h, &b.h, sizeof old.h) ? "differs" : "IDENTICAL", (void *)old.ptr,
            (void *)ptr, (unsigned long long)old.used, (unsigned long long)oid);
  // a mapping must never overlap one of this rank's own allocations (the
  // round-1 IPC aliasing symptom): refuse it, the call takes the
  // staged path
  for (int i = 0; i < nown; i++)
    if ((uint64_t)(uintptr_t)ptr < own[i].base + own[i].size && own[i].base < (uint64_t)(uintptr_t)ptr + b.size) {
      release_later(ptr, REL_IPC);
      return nullptr;
    }
  mx_reg_import ni{p, b.base, b.size, b.id, ptr, ++c->reg_tick, {}};
  memcpy(ni.h, &b.h, sizeof ni.h);
  v.push_back(ni);
  return ptr;
}

// host wait until every rank's record field reaches k (the communicator's
// wait timeout bounds it; 0 = forever)
static int reg_wait(mx_comm *c, bool verdict, uint64_t k) {
  RegRec *R = (RegRec *)c->reg_shm + (k & 1) * (size_t)c->size;   // call k's bank
  const auto t0 = std::chrono::steady_clock::now();
  for (int p = 0; p < c->size; p++) {
    unsigned spins = 0;
    while ((verdict ? R[p].vseq : R[p].seq).load(std::memory_order_acquire) < k) {
      if (++spins > 256) {
        sched_yield();
        if (c->timeout_s > 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > c->timeout_s) {
          c->poisoned = MX_ERR_TIMEOUT;
          timeout_dump(c, verdict ? "registration verdicts" : "registration records");
          return MX_ERR_TIMEOUT;
        }
      }
    }
  }
  return MX_SUCCESS;
}

static bool reg_fast_on() { static const bool v = env_default_on("MX_REG_FAST"); return v; }

static bool regbuf_eq(const RegBuf &a, const RegBuf &b) {
  return a.base == b.base && a.size == b.size && a.id == b.id && a.off == b.off &&
         !memcmp(&a.h, &b.h, sizeof a.h);
}

// Registration exchange of one call: 1 = every rank's buffers are mapped by
// every peer (ps / pr filled: peer j's sbuf / rbuf in this process), 0 = the
// call takes the staged path (on every rank), < 0 = error.  `mis` must be
// equal on every rank and `local_ok` true on every rank (the caller's
// conditions for the 16-byte vector path and for its data flow).
//
// Records live in two banks of the page, call k in bank k % 2: a rank reads
// its peers' bank-k records while a faster peer may already write call k+1's
// (bank k+1); it cannot reach call k+2 before this rank has published call
// k+1, i.e. finished reading bank k.  That lets a call whose records are
// exactly the last exchange's (the same buffers, buffer ids, misalignments;
// the last verdict 1 -- every rank sees the same records and remembers the
// same last exchange, so every rank decides alike) skip the verdict round:
// the mappings are the cached ones.  MX_REG_FAST=0 always runs both rounds.
static int reg_exchange(mx_comm *c, const char *sb, size_t sbytes, char *rb, size_t rbytes, int mis, bool local_ok,
                        const char **ps, char **pr) {
  const int n = c->size, r = c->rank;
  const uint64_t k = ++c->reg_seq;
  RegRec *R = (RegRec *)c->reg_shm + (k & 1) * (size_t)n;
  RegRec &me = R[r];
  int ok = local_ok && reg_export(sb, sbytes, &me.sb) && reg_export(rb, rbytes, &me.rb);
  me.mis = mis;
  me.ok = ok;
  me.seq.store(k, std::memory_order_release);
  if (int rc = reg_wait(c, false, k)) return rc;
  RegFast *F = (RegFast *)c->reg_fast;
  if (!F && reg_fast_on()) c->reg_fast = F = new (std::nothrow) RegFast();
  if (F && F->valid && reg_fast_on()) {
    bool same = true;
    for (int p = 0; same && p < n; p++)
      same = R[p].ok && F->ok[p] && R[p].mis == F->mis[p] && regbuf_eq(R[p].sb, F->sb[p]) &&
             regbuf_eq(R[p].rb, F->rb[p]);
    if (same) {
      c->st.reg_fast_calls++;
      for (int p = 0; p < n; p++) {
        ps[p] = F->ps[p];
        pr[p] = F->pr[p];
      }
      return 1;
    }
  }
  int verdict = 1;
  for (int p = 0; p < n; p++)
    if (!R[p].ok || R[p].mis != me.mis) verdict = 0;
  const RegBuf own[2] = {me.sb, me.rb};   // this rank's allocations (valid: the verdict needs ok)
  for (int p = 0; verdict && p < n; p++) {
    if (p == r) { ps[p] = sb; pr[p] = rb; continue; }
    const RegBuf &bs = R[p].sb, &br = R[p].rb;
    char *s0 = reg_import(c, p, bs, own, 2);
    char *r0 = s0 && br.base == bs.base && br.id == bs.id ? s0 : reg_import(c, p, br, own, 2);
    if (!s0 || !r0) { verdict = 0; break; }
    ps[p] = s0 + bs.off;
    pr[p] = r0 + br.off;
  }
  me.verdict = verdict;
  me.vseq.store(k, std::memory_order_release);
  if (int rc = reg_wait(c, true, k)) return rc;
  int all = 1;
  for (int p = 0; p < n; p++)
    if (!R[p].verdict) all = 0;
  if (F) {   // remember this exchange (the same on every rank)
    F->valid = all == 1;
    F->sb.resize(n);
    F->rb.resize(n);
    F->mis.resize(n);
    F->ok.resize(n);
    for (int p = 0; p < n; p++) {
      F->sb[p] = R[p].sb;
      F->rb[p] = R[p].rb;
      F->mis[p] = R[p].mis;
      F->ok[p] = R[p].ok;
      if (all) {
        F->ps[p] = ps[p];
        F->pr[p] = pr[p];
      }
    }
  }
  return all;
}

}  // namespace

// The staged / zero-copy allreduce above the one-shot range (mx_allreduce)
static int allreduce_staged(mx_comm *c, fold_launch_fn fl, int alg, const char *sb, char *rb, size_t count,
                            size_t es, int zc_mode, hipStream_t s) {
  const int n = c->size, r = c->rank;
  // Zero-copy: with every rank's sbuf and rbuf registered, the fold of part
  // r reads the peers' parts straight from their sbufs over xGMI and
  // (zc_direct, the default) stores the result straight into every peer's
  // rbuf: one kernel moves every byte of the call, both directions of every
  // link at once, and no staging is used (no gather area, no gather copy, no
  // chunking).  Coherence of those remote writes into cacheable memory
  // (DESIGN 7.1 rule 1'): the writer's fold ends before its PUSHED signal,
  // whose system-scope release writes its L2 back; the owner returns only
  // after its PUSHED wait, whose workgroups take a system-scope acquire on
  // every XCD.  zc_direct = 0: results travel through the peers' uncached
  // gather areas and a local gather copy (round 4).
  const char *ps[MAXR];
  char *pr[MAXR];
  int zc = 0;
  // the misalignments mod 16 of sbuf and rbuf must agree across ranks (the
  // fold's 16-byte vector path needs one misalignment for all operands)
  const int mis_sr = (int)((uintptr_t)sb & 15) | (c->zc_direct ? (int)(((uintptr_t)rb & 15) << 4) : 0);
  if (zc_allowed(c, zc_mode, count * es)) {
    zc = reg_exchange(c, sb, count * es, rb, count * es, mis_sr, true, ps, pr);
    if (zc < 0) return zc;
  }
  const bool direct = zc && c->zc_direct && (((uintptr_t)sb ^ (uintptr_t)rb) & 15) == 0;
  const size_t ce = direct ? count : chunk_elems(c, count, es, zc);
  if (zc) c->st.zero_copy_calls++;
  else c->st.staged_calls++;
  if (direct) c->st.direct_calls++;
  DoneMark dm;   // a blocking call: the last round's DONE signal raises the completion word
  done_mark_arm(c, dm);
  for (size_t c0 = 0; c0 < count; c0 += ce) {
    const size_t cl = std::min(ce, count - c0);
    const Layout L = layout_for(n, ce, es, zc);
    size_t off[MAXR], len[MAXR];
    blockcount(cl, n, off, len);
    const uint64_t g = ++c->gen;
    int rc;
    const bool pull = c->proto == MX_PROTO_PULL;
    // (a) peers finished the previous round with their staging.  Only PUSH
    // writes into peers' staging before the READY exchange; otherwise a peer's
    // READY(g) -- raised on its stream after everything it did in round g-1 --
    // already implies it (DONE(g-1) comes earlier on the same stream).
    if (!zc && !pull && (rc = wait_all(c, FLAG_DONE, g - 1, s))) return rc;
    const size_t mis0 = (c0 * es) & 15;
    CopyArgs ca;
    memset(&ca, 0, sizeof ca);
    if (zc) {
      // (b) nothing to move: the peers read my sbuf where it is
    } else if (pull) {
      // (b) copy the parts the peers fold (all but mine) into my own
      // staging, laid out as the chunk at its own misalignment mod 16
      const size_t lo = off[r], hi = off[r] + len[r];
      if (lo) ca.j[ca.n++] = CopyJob{sb + c0 * es, c->staging + mis0, lo * es};
      if (hi < cl) ca.j[ca.n++] = CopyJob{sb + (c0 + hi) * es, c->staging + mis0 + hi * es, (cl - hi) * es};
    } else {
      // (b) push my contribution for part p into rank p's slot `r`
      for (int p = 0; p < n; p++) {
        if (p == r || !len[p]) continue;
        const size_t e0 = c0 + off[p];
        ca.j[ca.n++] =
            CopyJob{sb + e0 * es, c->peer_staging[p] + (size_t)r * L.slot + ((e0 * es) & 15), len[p] * es};
      }
    }
    prof_begin(c, s);
    if ((rc = copy_launch(c, ca, s))) return rc;
    prof_end(c, s, 1, 0);
    if ((rc = signal_wait_all(c, FLAG_READY, g << 1, g << 1, s))) return rc;
    // (c) fold my part, store to my rbuf and every peer's gather area
    // (PULL: the peers' contributions are read from their staging over xGMI)
    if (len[r]) {
      const size_t e0 = c0 + off[r];
      const size_t mis = (e0 * es) & 15;
      const char *sp[MAXR];
      char *dp[MAXR];
      int nd = 0;
      for (int j = 0; j < n; j++)
        sp[j] = (j == r) ? sb + e0 * es
                : zc     ? ps[j] + e0 * es
                : pull   ? c->peer_staging[j] + mis0 + off[r] * es
                         : c->staging + (size_t)j * L.slot + mis;
      dp[nd++] = rb + e0 * es;
      for (int p = 0; p < n; p++)
        if (p != r) dp[nd++] = direct ? pr[p] + e0 * es
                                      : c->peer_staging[p] + L.gather_off + ((c0 * es) & 15) + off[r] * es;
      std::vector<Seg> segs;
      if ((rc = allreduce_segments(alg, n, count, es, e0, e0 + len[r], segs))) return rc;
      for (const Seg &sg : segs)
        if ((rc = run_fold(c, fl, sg, e0, sp, n, dp, nd, es, s, zc))) return rc;
    }
    // every peer's fold has stored its part into my rbuf (direct) or my
    // gather area, and has finished reading my sbuf
    if ((rc = signal_wait_all(c, FLAG_PUSHED, g, g, s))) return rc;
    if (direct) {
      if ((rc = signal_done(c, g, s, c0 + cl >= count ? &dm : nullptr))) return rc;
      continue;
    }
    // (d) copy the other parts from my gather area into rbuf
    memset(&ca, 0, sizeof ca);
    for (int p = 0; p < n; p++) {
      if (p == r || !len[p]) continue;
      ca.j[ca.n++] = CopyJob{c->staging + L.gather_off + ((c0 * es) & 15) + off[p] * es, rb + (c0 + off[p]) * es,
                             len[p] * es};
    }
    prof_begin(c, s);
    if ((rc = copy_launch(c, ca, s))) return rc;
    prof_end(c, s, 2, 0);
    if ((rc = signal_done(c, g, s, c0 + cl >= count ? &dm : nullptr))) return rc;
  }
  return finish_done(c, s, dm);
}

extern "C" int mx_allreduce(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                            void *stream) {
  if (!c || !rbuf) return MX_ERR_ARG;
  if (c->local) {
    const void *sb[1] = {sbuf};
    void *rb[1] = {rbuf};
    if (c->size != 1) return MX_ERR_STATE;
    return mx_allreduce_local(c, sb, rb, count, type, op, alg, stream);
  }
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  const size_t es = type_size(type);
  if (!es) return MX_ERR_ARG;
  const int n = c->size;
  const char *sb = (sbuf == MX_IN_PLACE || !sbuf) ? (const char *)rbuf : (const char *)sbuf;
  char *rb = (char *)rbuf;
  if (count == 0) return MX_SUCCESS;
  if (alg == MX_ALLREDUCE_RCCL) {
    if (!c->nccl) return MX_ERR_STATE;
    ncclDataType_t dt;
    ncclRedOp_t ro;
    switch (type) {
      case MX_TYPE_INT8_T: case MX_TYPE_INTEGER1: dt = ncclInt8; break;
      case MX_TYPE_UINT8_T: dt = ncclUint8; break;
      case MX_TYPE_INT32_T: case MX_TYPE_INTEGER: case MX_TYPE_INTEGER4: dt = ncclInt32; break;
      case MX_TYPE_UINT32_T: dt = ncclUint32; break;
      case MX_TYPE_INT64_T: case MX_TYPE_INTEGER8: dt = ncclInt64; break;
      case MX_TYPE_UINT64_T: dt = ncclUint64; break;
      case MX_TYPE_FLOAT: case MX_TYPE_REAL: case MX_TYPE_REAL4: dt = ncclFloat32; break;
      case MX_TYPE_DOUBLE: case MX_TYPE_REAL8: case MX_TYPE_DOUBLE_PRECISION: dt = ncclFloat64; break;
      default: return MX_ERR_UNSUPPORTED;
    }
    switch (op) {
      case MX_OP_SUM: ro = ncclSum; break;
      case MX_OP_PROD: ro = ncclProd; break;
      case MX_OP_MAX: ro = ncclMax; break;
      case MX_OP_MIN: ro = ncclMin; break;
      default: return MX_ERR_UNSUPPORTED;
    }
    if (ncclAllReduce(sb, rb, count, dt, ro, c->nccl, s) != ncclSuccess) return MX_ERR_RCCL;
    return finish(c, s);
  }
  fold_launch_fn fl = fold_fns(op, type).fold;
  if (!fl) return MX_ERR_UNSUPPORTED;
  if (n == 1) {
    if (int rc = copy_async(rb, sb, count * es, s)) return rc;
    return finish(c, s);
  }
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  if ((alg & 0xff) == MX_ALLREDUCE_NONOVERLAPPING) {
    // coll_base_allreduce.c:54-86: coll_reduce to rank 0, then coll_bcast;
    // in place, rank 0 reduces MPI_IN_PLACE and the others send their rbuf
    const bool inplace = sbuf == MX_IN_PLACE || !sbuf;
    const void *rsb = (inplace && c->rank == 0) ? MX_IN_PLACE : (const void *)sb;
    if (int rc = mx_reduce(c, rsb, c->rank == 0 ? rb : nullptr, count, type, op, 0, reduce_word_of(alg), stream))
      return rc;
    return mx_bcast(c, rb, count * es, 0, stream);
  }
  alg &= 0xff;
  const size_t bytes = count * es;
  // one-shot: possible up to the slot capacity os_cap, the default up to os_max
  std::vector<Seg> ossegs;
  oneshot_launch_fn ol = fold_fns(op, type).oneshot;
  bool os_ok = false;
  if (c->os_cap && bytes <= c->os_cap && ol) {
    if (int rc = allreduce_segments(alg, n, count, es, 0, count, ossegs)) return rc;
    os_ok = ossegs.size() <= (size_t)OS_MAXSEG;
  }
  {  // validate the algorithm once for the whole vector
    std::vector<Seg> probe;
    int rc = allreduce_segments(alg, n, count, es, 0, 0, probe);
    if (rc) return rc;
  }
  // autotuning: cand 0 zero-copy, 1 staged PULL, 2 staged PUSH,
  // 3 one-shot (size classes within the one-shot capacity); -1 the defaults
  // one-shot is a candidate only where it can run (os_ok depends on op,
  // type, size and algorithm only: the same on every rank)
  int bucket;
  const int ncand = os_ok ? 4 : 3;
  int cand = tune_pick(c, TUNE_ALLREDUCE, bytes, ncand, &bucket);
  if (cand == 3 || (cand < 0 && os_ok && bytes <= c->os_max)) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = allreduce_oneshot(c, ol, ossegs, sb, rb, count, es, s, op, type);
    return rc || cand < 0 ? rc : tune_done(c, TUNE_ALLREDUCE, bucket, cand, ncand, secs_since(t0));
  }
  const int proto0 = c->proto;
  if (cand == 1) c->proto = MX_PROTO_PULL;
  if (cand == 2) c->proto = MX_PROTO_PUSH;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = allreduce_staged(c, fl, alg, sb, rb, count, es, zc_mode_of(cand), s);
  c->proto = proto0;
  return rc || cand < 0 ? rc : tune_done(c, TUNE_ALLREDUCE, bucket, cand, ncand, secs_since(t0));
}

static int reduce_scatter_impl(mx_comm_t *c, const void *sbuf, void *rbuf, const size_t *rcounts, int type, int op,
                               int alg, void *stream, int zc_mode) {
  DoneMark dm;   // the call's last DONE signal raises the completion word (blocking calls)
  done_mark_arm(c, dm);
  if (!c || !rbuf || !rcounts) return MX_ERR_ARG;
  if (c->local) {
    if (c->size != 1) return MX_ERR_STATE;
    const void *sb[1] = {sbuf};
    void *rb[1] = {rbuf};
    return mx_reduce_scatter_local(c, sb, rb, rcounts, type, op, alg, stream);
  }
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  const size_t es = type_size(type);
  if (!es) return MX_ERR_ARG;
  const int n = c->size, r = c->rank;
  const char *sb = (sbuf == MX_IN_PLACE || !sbuf) ? (const char *)rbuf : (const char *)sbuf;
  size_t disp[MAXR], total = 0, maxc = 0;
  for (int j = 0; j < n; j++) { disp[j] = total; total += rcounts[j]; maxc = std::max(maxc, rcounts[j]); }
  if (total == 0) return MX_SUCCESS;
  fold_launch_fn fl = fold_fns(op, type).fold;
  if (!fl) return MX_ERR_UNSUPPORTED;
  if (n == 1) {
    if (int rc = copy_async(rbuf, sb, total * es, s)) return rc;
    return finish(c, s);
  }
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  if ((alg & 0xff) == MX_RS_NONOVERLAPPING) return rs_nonoverlapping(c, sb, (char *)rbuf, rcounts, type, op, alg, zc_mode != ZC_NEVER, s);
  alg &= 0xff;
  std::vector<Seg> segs;
  int rc = reduce_scatter_segments(alg, n, rcounts, es, r, segs);
  if (rc) return rc;
  // IN_PLACE with my block not first: my result would overwrite input still
  // to be read -> fold into a spare slot after the n slots, then copy
  // (the slot geometry must be the same on every rank: it depends only on
  // the collective IN_PLACE choice, not on this rank's block)
  const bool inplace = sb == (const char *)rbuf;
  if (zc_allowed(c, zc_mode, total * es) && !inplace) {
    // zero-copy: rank r folds block r straight from every rank's registered
    // sbuf into its own rbuf (IN_PLACE stays staged: block 0 of a rank's
    // input is its output area, which rank 0 would still be reading)
    const char *ps[MAXR];
    char *pr[MAXR];
    const bool lok = (((uintptr_t)rbuf - ((uintptr_t)sb + disp[r] * es)) & 15) == 0;
    const int zc = reg_exchange(c, sb, total * es, (char *)rbuf, rcounts[r] * es, (int)((uintptr_t)sb & 15), lok,
                                ps, pr);
    if (zc < 0) return zc;
    if (zc) {
      const uint64_t g = ++c->gen;
      c->st.zero_copy_calls++;
      if ((rc = signal_wait_all(c, FLAG_READY, g << 1, g << 1, s))) return rc;
      if (rcounts[r]) {
        const char *sp[MAXR];
        for (int j = 0; j < n; j++) sp[j] = ps[j] + disp[r] * es;
        char *dp[1] = {(char *)rbuf};
        for (const Seg &sg : segs)
          if ((rc = run_fold(c, fl, sg, disp[r], sp, n, dp, 1, es, s, true))) return rc;
      }
      if ((rc = signal_wait_all(c, FLAG_PUSHED, g, g, s))) return rc;     // every peer is done with my sbuf
      if ((rc = signal_done(c, g, s, &dm))) return rc;
      return finish_done(c, s, dm);
    }
  }
  const bool overlap = inplace && disp[r] != 0;
  const size_t nslots = (size_t)n + (inplace ? 1 : 0);
  // chunks of every block (piece k0 of block q goes to rank q's slot r):
  // blocks of any size run through the staging
  size_t kc = maxc;
  while (kc > 1 && nslots * rup(kc * es + 16, 256) > c->main_bytes) kc = (kc + 1) / 2;
  const size_t slot = rup(kc * es + 16, 256);
  if (nslots * slot > c->main_bytes) return MX_ERR_NOMEM;
  for (size_t k0 = 0; k0 < maxc; k0 += kc) {
    const uint64_t g = ++c->gen;
    if ((rc = wait_all(c, FLAG_DONE, g - 1, s))) return rc;
    CopyArgs ca;
    memset(&ca, 0, sizeof ca);
    for (int p = 0; p < n; p++) {
      if (p == r || k0 >= rcounts[p]) continue;
      const size_t e0 = disp[p] + k0;
      ca.j[ca.n++] = CopyJob{sb + e0 * es, c->peer_staging[p] + (size_t)r * slot + ((e0 * es) & 15),
                             std::min(kc, rcounts[p] - k0) * es};
    }
    prof_begin(c, s);
    if ((rc = copy_launch(c, ca, s))) return rc;
    prof_end(c, s, 1, 0);
    if ((rc = signal_wait_all(c, FLAG_READY, g << 1, g << 1, s))) return rc;
    if (k0 < rcounts[r]) {
      const size_t kl = std::min(kc, rcounts[r] - k0), e0 = disp[r] + k0, mis = (e0 * es) & 15;
      const char *sp[MAXR];
      for (int j = 0; j < n; j++) sp[j] = (j == r) ? sb + e0 * es : c->staging + (size_t)j * slot + mis;
      char *dst = overlap ? c->staging + (size_t)n * slot + mis : (char *)rbuf + k0 * es;
      char *dp[1] = {dst};
      // padded types are stored field by field: the spare slot starts as the
      // bytes the result replaces, so the copy back keeps rbuf's padding
      if (overlap && (rc = copy_async(dst, (char *)rbuf + k0 * es, kl * es, s))) return rc;
      for (const Seg &sg : segs) {
        const Seg piece{std::max(sg.lo, e0), std::min(sg.hi, e0 + kl), sg.p};
        if (piece.lo < piece.hi && (rc = run_fold(c, fl, piece, e0, sp, n, dp, 1, es, s))) return rc;
      }
      if (overlap && (rc = copy_async((char *)rbuf + k0 * es, dst, kl * es, s))) return rc;
    }
    if ((rc = signal_done(c, g, s, k0 + kc >= maxc ? &dm : nullptr))) return rc;
  }
  return finish_done(c, s, dm);
}

static int allgather_impl(mx_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, void *stream, int zc_mode) {
  DoneMark dm;   // the call's last DONE signal raises the completion word (blocking calls)
  done_mark_arm(c, dm);
  if (!c || !rbuf) return MX_ERR_ARG;
  if (c->local) {
    if (c->size != 1) return MX_ERR_STATE;
    const void *sb[1] = {sbuf};
    void *rb[1] = {rbuf};
    return mx_allgather_local(c, sb, rb, bytes, stream);
  }
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  const int n = c->size, r = c->rank;
  char *rb = (char *)rbuf;
  const char *sb = (sbuf == MX_IN_PLACE || !sbuf) ? rb + (size_t)r * bytes : (const char *)sbuf;
  if (!bytes) return MX_SUCCESS;
  if (n == 1) {
    if (int rc = copy_async(rb, sb, bytes, s)) return rc;
    return finish(c, s);
  }
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  if (zc_allowed(c, zc_mode, (size_t)n * bytes)) {
    // zero-copy: every rank reads the peers' blocks straight from their
    // registered sbufs into its own rbuf (remote reads, local writes only)
    const char *ps[MAXR];
    char *pr[MAXR];
    const bool lok = ((uintptr_t)sb & 15) == (((uintptr_t)rb + (size_t)r * bytes) & 15);
    const int zc = reg_exchange(c, sb, bytes, rb, (size_t)n * bytes, (int)((uintptr_t)rb & 15), lok, ps, pr);
    if (zc < 0) return zc;
    if (zc) {
      const uint64_t g = ++c->gen;
      int rc;
      c->st.zero_copy_calls++;
      if ((rc = signal_wait_all(c, FLAG_READY, g << 1, g << 1, s))) return rc;   // every sbuf holds its block
      CopyArgs ca;
      memset(&ca, 0, sizeof ca);
      for (int p = 0; p < n; p++)
        if (p != r) ca.j[ca.n++] = CopyJob{ps[p], rb + (size_t)p * bytes, bytes};
      if (sb != rb + (size_t)r * bytes) ca.j[ca.n++] = CopyJob{sb, rb + (size_t)r * bytes, bytes};
      if ((rc = copy_launch(c, ca, s))) return rc;
      if ((rc = signal_wait_all(c, FLAG_PUSHED, g, g, s))) return rc;     // done reading the peers' sbufs
      if ((rc = signal_done(c, g, s, &dm))) return rc;
      return finish_done(c, s, dm);
    }
  }
  // n slots of `slot` bytes; each round moves up to `cb` bytes per rank
  const size_t slot = (c->main_bytes / n) & ~(size_t)255;
  if (slot < 512) return MX_ERR_NOMEM;
  const size_t cb = slot - 256;
  for (size_t o = 0; o < bytes; o += cb) {
    const size_t l = std::min(cb, bytes - o);
    const uint64_t g = ++c->gen;
    int rc;
    if ((rc = wait_all(c, FLAG_DONE, g - 1, s))) return rc;
    CopyArgs ca;
    memset(&ca, 0, sizeof ca);
    for (int p = 0; p < n; p++)
      if (p != r) ca.j[ca.n++] = CopyJob{sb + o, c->peer_staging[p] + (size_t)r * slot + ((r * bytes + o) & 15), l};
    if (sb != rb + (size_t)r * bytes) ca.j[ca.n++] = CopyJob{sb + o, rb + (size_t)r * bytes + o, l};
    if ((rc = copy_launch(c, ca, s))) return rc;
    if ((rc = signal_wait_all(c, FLAG_READY, g << 1, g << 1, s))) return rc;
    memset(&ca, 0, sizeof ca);
    for (int p = 0; p < n; p++)
      if (p != r)
        ca.j[ca.n++] = CopyJob{c->staging + (size_t)p * slot + ((p * bytes + o) & 15), rb + (size_t)p * bytes + o, l};
    if ((rc = copy_launch(c, ca, s))) return rc;
    if ((rc = signal_done(c, g, s, o + cb >= bytes ? &dm : nullptr))) return rc;
  }
  return finish_done(c, s, dm);
}

// ---------------------------------------------------------------------------
// exchanges: alltoall, alltoallv, allgatherv (k_exchange, mx_exchange.hip)
// ---------------------------------------------------------------------------
namespace {

// One rank's view of an exchange.  Every field but the buffers is known to
// -- and equal on -- every rank that needs it: the collective decisions
// (data path, round count) depend only on zc_bytes, max_pair and inplace.
struct XCall {
  const char *sb;              // what this rank sends from (in place: its rbuf)
  char *rb;
  size_t sb_span, rb_span;     // bytes of sb / rb the call may touch (registration)
  size_t send_off[MAXR], send_len[MAXR];   // my block for p, in sb
  size_t pull_off[MAXR];       // my block in p's sb
  size_t mis, peer_mis[MAXR];  // sb's address mod 16, mine and p's, where the ranks exchanged it (else 0)
  size_t recv_off[MAXR], recv_len[MAXR];   // where p's block lands in rb; what of it is taken
  size_t max_pair;             // the largest block any rank sends
  size_t zc_bytes;             // the size the zero-copy threshold sees
  bool inplace;
  // the strided forms: offsets are displacement x extent (signed, kept modulo
  // 2^64), lengths stream bytes, and sb / rb the `user` pointers of the layouts
  bool ddt;
  XLay slay, rlay;             // my send / receive layout
  XLay peer_slay[MAXR];        // p's send layout (what a zero-copy pull reads by)
  int64_t sb_lo, rb_lo;        // where the spans sb_span / rb_span start, from sb / rb
  int64_t peer_lo[MAXR];       // p's sb_lo
};


static int xrow_exchange(mx_comm *c, const size_t *bytes, const size_t *offs, uint64_t flags, const XRow **rows,
                         const XRowExt *ext = nullptr) {
  const int n = c->size;
  const uint64_t k = ++c->xrow_seq;
  XRow *X = (XRow *)((char *)c->reg_shm + 2 * (size_t)n * sizeof(RegRec)) + (k & 1) * (size_t)n;
  XRow &me = X[c->rank];
  me.flags = flags;
  if (ext) me.e = *ext;
  for (int p = 0; p < n; p++) {
    me.bytes[p] = bytes[p];
    me.offs[p] = offs[p];
  }
  me.seq.store(k, std::memory_order_release);
  const auto t0 = std::chrono::steady_clock::now();
  for (int p = 0; p < n; p++) {
    unsigned spins = 0;
    while (X[p].seq.load(std::memory_order_acquire) < k) {
      if (++spins > 256) {
        sched_yield();
        if (c->timeout_s > 0 && secs_since(t0) > c->timeout_s) {
          c->poisoned = MX_ERR_TIMEOUT;
          timeout_dump(c, "alltoallv rows");
          return MX_ERR_TIMEOUT;
        }
      }
    }
  }
  *rows = X;
  return MX_SUCCESS;
}

static int exchange_mp(mx_comm *c, const XCall &x, hipStream_t s) {
  DoneMark dm;   // the call's last DONE signal raises the completion word
  done_mark_arm(c, dm);
  const int n = c->size, r = c->rank;
  xcount(c, 0, x.ddt);
  if (!x.max_pair) return MX_SUCCESS;   // nothing moves on any rank
  const size_t self_len = std::min(x.send_len[r], x.recv_len[r]);
  XJob jobs[MAXR];
  XVJob vjobs[MAXR];
  int nj, rc;
  // the strided forms: the same jobs with a layout on either side
  auto vadd = [&](const char *src, const XLay &sl, uint64_t pos_s, char *dst, const XLay &dl, uint64_t pos_d,
                  size_t len) { return len ? xvjob_make(src, sl, pos_s, dst, dl, pos_d, len, &vjobs[nj++]) : MX_SUCCESS; };
  const XLay flat = xlay_flat();
  if (!x.inplace && zc_allowed(c, ZC_DEFAULT, x.zc_bytes)) {
    // zero-copy: rank r pulls its block from every peer's registered sbuf
    // straight into its rbuf (remote reads, local writes only).  The kernel
    // takes any pair of alignments, so the ranks need not agree on one.
    const char *ps[MAXR];
    char *pr[MAXR];
    // (the strided forms register the true spans: sb_lo / rb_lo may be negative)
    const int zc = reg_exchange(c, padd(x.sb, x.sb_lo), x.sb_span, padd(x.rb, x.rb_lo), x.rb_span, 0, true, ps, pr);
    if (zc < 0) return zc;
    if (zc) {
      const uint64_t g = ++c->gen;
      xcount(c, 1, x.ddt);
      if ((rc = signal_wait_all(c, FLAG_READY, g << 1, g << 1, s))) return rc;   // every sbuf holds its blocks
      nj = 0;
      if (x.ddt) {   // both sides strided, the source layout from the peer's row
        for (int p = 0; p < n && !rc; p++)
          if (p != r)
            rc = vadd(padd(ps[p], x.pull_off[p] - (uint64_t)x.peer_lo[p]), x.peer_slay[p], 0, padd(x.rb, x.recv_off[p]),
                      x.rlay, 0, x.recv_len[p]);
        if (!rc) rc = vadd(padd(x.sb, x.send_off[r]), x.slay, 0, padd(x.rb, x.recv_off[r]), x.rlay, 0, self_len);
        if (rc || (rc = exchange_vec_launch(vjobs, nj, c->poison, s))) return rc;
      } else {
        for (int p = 0; p < n; p++)
          if (p != r) jobs[nj++] = XJob{ps[p] + x.pull_off[p], x.rb + x.recv_off[p], x.recv_len[p]};
        if (x.sb + x.send_off[r] != x.rb + x.recv_off[r])
          jobs[nj++] = XJob{x.sb + x.send_off[r], x.rb + x.recv_off[r], self_len};
        if ((rc = exchange_launch(jobs, nj, c->poison, s))) return rc;
      }
      if ((rc = signal_wait_all(c, FLAG_PUSHED, g, g, s))) return rc;   // done reading the peers' sbufs
      if ((rc = signal_done(c, g, s, &dm))) return rc;
      return finish_done(c, s, dm);
    }
  }
  // staged: n slots; the sender pushes its block for p into p's slot r, and
  // after READY the receiver moves slot p to its place in rbuf.  A slot
  // offset keeps the source address mod 16, so the push needs no shifting:
  // exactly where the ranks exchanged their buffers' misalignment
  // (alltoallv); alltoall and allgatherv exchange nothing, both sides take
  // the block's offset in the sender's buffer mod 16, which is the address's
  // for a 16-byte aligned sbuf -- a misaligned one pushes through the
  // kernel's shift path (correct, slower).
  // In place the pushes read what the moves overwrite: a rank's moves follow
  // its own pushes on the stream and every peer's pushes through READY.
  size_t slot, cap;
  if (!xstage_slots(c->main_bytes, n, &slot, &cap)) return MX_ERR_NOMEM;
  const uint64_t rounds = xrounds(x.max_pair, cap);
  xcount(c, 2, x.ddt);
  for (uint64_t q = 0; q < rounds; q++) {
    const uint64_t g = ++c->gen;
    size_t o, l;
    xcount(c, 3, x.ddt);
    if ((rc = wait_all(c, FLAG_DONE, g - 1, s))) return rc;
    nj = 0;
    if (x.ddt) {
      // strided -> flat slot, then flat slot -> strided.  A round cuts every
      // pair's stream at q * cap (a multiple of 256), inside a block or an
      // instance as it falls; the slots start 256-byte aligned.
      rc = MX_SUCCESS;
      for (int p = 0; p < n && !rc; p++) {
        if (p == r) continue;
        xround_piece(x.send_len[p], cap, q, &o, &l);
        rc = vadd(padd(x.sb, x.send_off[p]), x.slay, o, c->peer_staging[p] + (size_t)r * slot, flat, 0, l);
      }
      xround_piece(self_len, cap, q, &o, &l);
      if (!rc && !x.inplace) rc = vadd(padd(x.sb, x.send_off[r]), x.slay, o, padd(x.rb, x.recv_off[r]), x.rlay, o, l);
      if (rc || (rc = exchange_vec_launch(vjobs, nj, c->poison, s))) return rc;
      if ((rc = signal_wait_all(c, FLAG_READY, g << 1, g << 1, s))) return rc;
      nj = 0;
      for (int p = 0; p < n && !rc; p++) {
        if (p == r) continue;
        xround_piece(x.recv_len[p], cap, q, &o, &l);
        rc = vadd(c->staging + (size_t)p * slot, flat, 0, padd(x.rb, x.recv_off[p]), x.rlay, o, l);
      }
      if (rc || (rc = exchange_vec_launch(vjobs, nj, c->poison, s))) return rc;
      if ((rc = signal_done(c, g, s, q + 1 == rounds ? &dm : nullptr))) return rc;
      continue;
    }
    for (int p = 0; p < n; p++) {
      if (p == r) continue;
      xround_piece(x.send_len[p], cap, q, &o, &l);
      jobs[nj++] = XJob{x.sb + x.send_off[p] + o, c->peer_staging[p] + (size_t)r * slot + ((x.mis + x.send_off[p] + o) & 15), l};
    }
    xround_piece(self_len, cap, q, &o, &l);
    if (x.sb + x.send_off[r] != x.rb + x.recv_off[r])
      jobs[nj++] = XJob{x.sb + x.send_off[r] + o, x.rb + x.recv_off[r] + o, l};
    if ((rc = exchange_launch(jobs, nj, c->poison, s))) return rc;
    if ((rc = signal_wait_all(c, FLAG_READY, g << 1, g << 1, s))) return rc;
    nj = 0;
    for (int p = 0; p < n; p++) {
      if (p == r) continue;
      xround_piece(x.recv_len[p], cap, q, &o, &l);
      jobs[nj++] = XJob{c->staging + (size_t)p * slot + ((x.peer_mis[p] + x.pull_off[p] + o) & 15), x.rb + x.recv_off[p] + o, l};
    }
    if ((rc = exchange_launch(jobs, nj, c->poison, s))) return rc;
    if ((rc = signal_done(c, g, s, q + 1 == rounds ? &dm : nullptr))) return rc;
  }
  return finish_done(c, s, dm);
}

// the common prologue: a communicator of one process (local, size 1) or of
// one rank is served by the caller with a device copy
static int exchange_enter(mx_comm *c, hipStream_t s) {
  if (int orc = order(c, s)) return orc;
  if (c->size > 1 && !(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  return MX_SUCCESS;
}
static int exchange_self(mx_comm *c, const char *src, char *dst, size_t bytes, hipStream_t s) {
  xcount(c, 0);
  if (bytes && src != dst) {
    const XJob jb{src, dst, bytes};
    if (int rc = exchange_launch(&jb, 1, c->poison, s)) return rc;
  }
  return finish(c, s);
}

}  // namespace

extern "C" int mx_comm_set_exchange_min(mx_comm_t *c, size_t min_bytes) {
  if (!c) return MX_ERR_ARG;
  c->xmin = min_bytes;
  return MX_SUCCESS;
}

extern "C" long long mx_comm_exchange_rounds(const mx_comm_t *c, size_t max_pair) {
  if (!c) return MX_ERR_ARG;
  if (c->local || c->size < 2) return 0;
  size_t slot, cap;
  if (!xstage_slots(c->main_bytes, c->size, &slot, &cap)) return MX_ERR_NOMEM;
  return (long long)xrounds(max_pair, cap);
}

extern "C" int mx_alltoall(mx_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, void *stream) {
  if (!c || !rbuf || (c->local && c->size != 1)) return c && c->local ? MX_ERR_STATE : MX_ERR_ARG;
  const int n = c->size, r = c->rank;
  if ((size_t)n * bytes / (size_t)n != bytes) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = exchange_enter(c, s)) return rc;
  XCall x;
  memset(&x, 0, sizeof x);
  x.inplace = sbuf == MX_IN_PLACE || !sbuf;   // every rank sends `bytes`: NULL can only mean in place
  x.rb = (char *)rbuf;
  x.sb = x.inplace ? (const char *)rbuf : (const char *)sbuf;
  if (n == 1) return exchange_self(c, x.sb, x.rb, bytes, s);
  x.sb_span = x.rb_span = (size_t)n * bytes;
  for (int p = 0; p < n; p++) {
    x.send_off[p] = x.recv_off[p] = (size_t)p * bytes;
    x.pull_off[p] = (size_t)r * bytes;
    x.send_len[p] = x.recv_len[p] = bytes;
  }
  x.max_pair = bytes;
  x.zc_bytes = (size_t)n * bytes;
  return exchange_mp(c, x, s);
}

extern "C" int mx_allgatherv(mx_comm_t *c, const void *sbuf, size_t sbytes, void *rbuf, const size_t *rbytes,
                             const size_t *roffs, void *stream) {
  if (!c || !rbuf || (c->local && c->size != 1)) return c && c->local ? MX_ERR_STATE : MX_ERR_ARG;
  const int n = c->size, r = c->rank;
  if (int rc = xcheck_row(n, rbytes, roffs)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = exchange_enter(c, s)) return rc;
  XCall x;
  memset(&x, 0, sizeof x);
  // a rank with an empty block may pass any sbuf, NULL included, without
  // being in place: the data path must not depend on it (NULL with a block
  // to send is the other entry points' synonym of MX_IN_PLACE)
  x.inplace = sbuf == MX_IN_PLACE || (!sbuf && rbytes[r] != 0);
  x.rb = (char *)rbuf;
  // in place a rank's block sits at roffs[rank] of its rbuf, on every rank
  x.sb = (x.inplace || !sbuf) ? (const char *)rbuf : (const char *)sbuf;
  const size_t mine = x.inplace ? rbytes[r] : std::min(sbytes, rbytes[r]);
  if (n == 1) return exchange_self(c, x.sb + (x.inplace ? roffs[0] : 0), x.rb + roffs[0], mine, s);
  for (int p = 0; p < n; p++) {
    x.send_off[p] = x.inplace ? roffs[r] : 0;
    x.send_len[p] = mine;
    x.pull_off[p] = x.inplace ? roffs[p] : 0;
    x.recv_off[p] = roffs[p];
    x.recv_len[p] = p == r ? mine : rbytes[p];
    x.rb_span = std::max(x.rb_span, roffs[p] + rbytes[p]);
    x.max_pair = std::max(x.max_pair, rbytes[p]);
    x.zc_bytes += rbytes[p];
  }
  x.sb_span = x.inplace ? x.rb_span : mine;
  return exchange_mp(c, x, s);
}

extern "C" int mx_alltoallv(mx_comm_t *c, const void *sbuf, const size_t *sbytes, const size_t *soffs, void *rbuf,
                            const size_t *rbytes, const size_t *roffs, void *stream) {
  if (!c || (c->local && c->size != 1)) return c && c->local ? MX_ERR_STATE : MX_ERR_ARG;
  const int n = c->size, r = c->rank;
  if (int rc = xcheck_row(n, rbytes, roffs)) return rc;
  XCall x;
  memset(&x, 0, sizeof x);
  // Only MX_IN_PLACE is in place here: a rank that sends nothing may pass any
  // sbuf, NULL included, and one that receives nothing any rbuf, and the
  // data path must not depend on either (every rank has to choose alike)
  x.inplace = sbuf == MX_IN_PLACE;
  if (x.inplace) { sbytes = rbytes; soffs = roffs; }   // MPI: the receive row describes both sides
  else if (int rc = xcheck_row(n, sbytes, soffs)) return rc;
  size_t stotal = 0, rtotal = 0;
  for (int p = 0; p < n; p++) { stotal += sbytes[p]; rtotal += rbytes[p]; }
  if ((!rbuf && rtotal) || (!x.inplace && !sbuf && stotal)) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = exchange_enter(c, s)) return rc;
  x.rb = (char *)rbuf;
  x.sb = x.inplace ? (const char *)rbuf : (const char *)sbuf;
  if (!x.sb) x.sb = x.rb;     // nothing to send: any address serves (no byte of it is read)
  if (!x.rb) x.rb = (char *)x.sb;
  if (n == 1) return exchange_self(c, x.sb + soffs[0], x.rb + roffs[0], std::min(sbytes[0], rbytes[0]), s);
  // a rank knows neither where its block starts in a peer's sbuf nor the
  // largest pair of the call: the rows travel through the registration page
  if (!c->reg_shm) return MX_ERR_UNSUPPORTED;   // agreed at creation: every rank returns here
  const XRow *rows = nullptr;
  x.mis = (uintptr_t)x.sb & 15;
  if (int rc = xrow_exchange(c, sbytes, soffs, x.mis | (x.inplace ? 16 : 0), &rows)) return rc;
  for (int p = 0; p < n; p++) {
    if (((rows[p].flags >> 4) & 1) != (uint64_t)x.inplace) return MX_ERR_ARG;   // MPI_IN_PLACE on some ranks only: every rank sees it
    x.send_off[p] = soffs[p];
    x.send_len[p] = sbytes[p];
    x.pull_off[p] = (size_t)rows[p].offs[r];
    x.peer_mis[p] = (size_t)(rows[p].flags & 15);
    x.recv_off[p] = roffs[p];
    x.recv_len[p] = std::min((size_t)rows[p].bytes[r], rbytes[p]);   // never past the receiver's size
    x.sb_span = std::max(x.sb_span, soffs[p] + sbytes[p]);
    x.rb_span = std::max(x.rb_span, roffs[p] + rbytes[p]);
    for (int q = 0; q < n; q++) x.max_pair = std::max(x.max_pair, (size_t)rows[p].bytes[q]);
  }
  x.zc_bytes = (size_t)n * x.max_pair;
  if (c->xmin && x.zc_bytes <= c->xmin) return MX_ERR_UNSUPPORTED;   // the same on every rank
  return exchange_mp(c, x, s);
}

// The strided forms.  Every rank takes part in the row exchange whatever it
// thinks of its own datatypes, so a refusal anywhere is every rank's return
// value and nobody is left waiting.
extern "C" int mx_alltoallv_ddt(mx_comm_t *c, const void *sbuf, const size_t *scounts, const int64_t *sdispls,
                                const mx_ddt_t *sddt, void *rbuf, const size_t *rcounts, const int64_t *rdispls,
                                const mx_ddt_t *rddt, void *stream) {
  if (!c || (c->local && c->size != 1)) return c && c->local ? MX_ERR_STATE : MX_ERR_ARG;
  const int n = c->size, r = c->rank;
  if (!rcounts || !rdispls) return MX_ERR_ARG;
  XCall x;
  memset(&x, 0, sizeof x);
  x.ddt = true;
  x.inplace = sbuf == MX_IN_PLACE;
  if (x.inplace) { scounts = rcounts; sdispls = rdispls; sddt = rddt; }
  else if (!scounts || !sdispls) return MX_ERR_ARG;
  const XDSide S = xd_side(sddt, false), R = xd_side(rddt, true);
  if (!xd_counts_ok(S, n, scounts) || !xd_counts_ok(R, n, rcounts)) return MX_ERR_ARG;
  size_t stotal = 0, rtotal = 0;
  for (int p = 0; p < n; p++) { stotal += scounts[p]; rtotal += rcounts[p]; }
  if ((!rbuf && rtotal) || (!x.inplace && !sbuf && stotal)) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = exchange_enter(c, s)) return rc;
  x.rb = (char *)rbuf;
  x.sb = x.inplace ? (const char *)rbuf : (const char *)sbuf;
  if (!x.sb) x.sb = x.rb;     // nothing to send: any address serves (no byte of it is read)
  if (!x.rb) x.rb = (char *)x.sb;
  x.slay = S.lay;
  x.rlay = R.lay;
  // a buffer no byte moves through does not count (its address may be anything)
  const unsigned sunit = S.ok ? xd_unit(S, stotal ? x.sb : nullptr, n, scounts, sdispls) : 0;
  const unsigned runit = R.ok ? xd_unit(R, rtotal ? x.rb : nullptr, n, rcounts, rdispls) : 0;
  const bool mine = sunit >= 4 && runit >= 4;
  if (n == 1) {
    if (!mine) return MX_ERR_UNSUPPORTED;
    xcount(c, 0, true);
    XVJob jb;
    const size_t len = std::min(scounts[0] * S.size, rcounts[0] * R.size);
    const char *src = padd(x.sb, (uint64_t)(sdispls[0] * S.ext));
    char *dst = padd(x.rb, (uint64_t)(rdispls[0] * R.ext));
    if (len && !x.inplace) {
      if (int rc = xvjob_make(src, S.lay, 0, dst, R.lay, 0, len, &jb)) return rc;
      if (int rc = exchange_vec_launch(&jb, 1, c->poison, s)) return rc;
    }
    return finish(c, s);
  }
  if (!c->reg_shm) return MX_ERR_UNSUPPORTED;   // agreed at creation: every rank returns here
  // the spans this rank would register (the true bounds of what the call touches)
  int64_t slo = INT64_MAX, shi = INT64_MIN, rlo = INT64_MAX, rhi = INT64_MIN;
  size_t sbytes[MAXR], soffs[MAXR];
  for (int p = 0; p < n; p++) {
    sbytes[p] = S.ok ? scounts[p] * S.size : 0;
    soffs[p] = S.ok ? (size_t)(sdispls[p] * S.ext) : 0;
    if (S.ok) xd_span(S, scounts[p], sdispls[p], &slo, &shi);
    if (R.ok) xd_span(R, rcounts[p], rdispls[p], &rlo, &rhi);
  }
  if (slo > shi) slo = shi = 0;
  if (rlo > rhi) rlo = rhi = 0;
  XRowExt e;
  memset(&e, 0, sizeof e);
  e.slay = S.lay;
  e.lo = slo;
  e.sunit = sunit;
  e.runit = runit;
  e.verdict = mine;
  const XRow *rows = nullptr;
  if (int rc = xrow_exchange(c, sbytes, soffs, (x.inplace ? 16 : 0) | 32, &rows, &e)) return rc;
  bool all = true;
  for (int p = 0; p < n; p++) {
    if (!(rows[p].flags & 32) || ((rows[p].flags >> 4) & 1) != (uint64_t)x.inplace) return MX_ERR_ARG;   // every rank sees it
    all = all && rows[p].e.verdict && rows[p].e.sunit >= 4 && rows[p].e.runit >= 4;
  }
  if (!all) return MX_ERR_UNSUPPORTED;   // the same on every rank, before any byte moves
  for (int p = 0; p < n; p++) {
    x.send_off[p] = soffs[p];
    x.send_len[p] = sbytes[p];
    x.pull_off[p] = (size_t)rows[p].offs[r];
    x.peer_slay[p] = rows[p].e.slay;
    x.peer_lo[p] = rows[p].e.lo;
    x.recv_off[p] = (size_t)(rdispls[p] * R.ext);
    x.recv_len[p] = std::min((size_t)rows[p].bytes[r], rcounts[p] * R.size);   // never past the receiver's room
    for (int q = 0; q < n; q++) x.max_pair = std::max(x.max_pair, (size_t)rows[p].bytes[q]);
  }
  x.sb_lo = slo;
  x.sb_span = (size_t)(shi - slo);
  x.rb_lo = rlo;
  x.rb_span = (size_t)(rhi - rlo);
  x.zc_bytes = (size_t)n * x.max_pair;
  if (c->xmin && x.zc_bytes <= c->xmin) return MX_ERR_UNSUPPORTED;   // the same on every rank
  return exchange_mp(c, x, s);
}

extern "C" int mx_alltoall_ddt(mx_comm_t *c, const void *sbuf, size_t scount, const mx_ddt_t *sddt, void *rbuf,
                               size_t rcount, const mx_ddt_t *rddt, void *stream) {
  if (!c || c->size < 1 || c->size > MAXR) return MX_ERR_ARG;
  size_t sc[MAXR], rc[MAXR];
  int64_t sd[MAXR], rd[MAXR];
  for (int p = 0; p < c->size; p++) {
    sc[p] = scount;
    rc[p] = rcount;
    sd[p] = (int64_t)p * (int64_t)scount;
    rd[p] = (int64_t)p * (int64_t)rcount;
  }
  return mx_alltoallv_ddt(c, sbuf ? sbuf : MX_IN_PLACE, sc, sd, sddt, rbuf, rc, rd, rddt, stream);
}

// ---------------------------------------------------------------------------
// rooted exchanges: gather, gatherv, scatter, scatterv.  Every decision --
// who launches which jobs, which flags a kernel waits for, how the staging
// is cut -- is planned on the host (mx_rooted_plan.hpp); here the plan's
// jobs are resolved to pointers and handed to the two exchange kernels
// between the flag kernels.  A rank knows only its own sides: the rows of
// the registration page carry what the others need, and the verdict is a
// function of the rows alone.
// ---------------------------------------------------------------------------
namespace {

struct RBufs {                  // what a job's ends resolve to in this process
  const char *single[MAXR];     // rank p's single-side user pointer (a peer's: where its span is mapped)
  const char *multi;            // the root's multi-side user pointer
  char *stage[MAXR];
};

static int rooted_launch(mx_comm *c, const RBufs &b, const std::vector<RJob> &jobs, hipStream_t s) {
  XJob bj[MAXR];
  XVJob vj[MAXR];
  int nb = 0, nv = 0;
  auto end_ptr = [&](const REnd &e) {
    const char *base = e.buf == RB_SINGLE ? b.single[e.rank] : e.buf == RB_MULTI ? b.multi : b.stage[e.rank];
    return padd(base, (uint64_t)e.off);
  };
  for (const RJob &j : jobs) {
    if (nb >= MAXR || nv >= MAXR) return MX_ERR_ARG;
    const char *src = end_ptr(j.s);
    char *dst = end_ptr(j.d);
    if (j.bytes) {   // flat -> flat: any length, any alignment
      bj[nb++] = XJob{padd(src, (uint64_t)xlay_off(j.s.lay, j.s.pos)), padd(dst, (uint64_t)xlay_off(j.d.lay, j.d.pos)),
                      (size_t)j.len};
    } else if (int rc = xvjob_make(src, j.s.lay, j.s.pos, dst, j.d.lay, j.d.pos, j.len, &vj[nv++])) {
      return rc;
    }
  }
  if (nb)
    if (int rc = exchange_launch(bj, (size_t)nb, c->poison, s)) return rc;
  return nv ? exchange_vec_launch(vj, (size_t)nv, c->poison, s) : MX_SUCCESS;
}

// One rank's arguments: its single side (what it sends to a gather, where
// it receives from a scatter) and, on the root, the multi side.
struct RArgs {
  const void *single;
  size_t count;
  const mx_ddt_t *ddt;
  const void *multi;
  const size_t *counts;
  const int64_t *displs;
  const mx_ddt_t *mddt;
  bool inplace;   // the root only
};

// the row `rank` publishes; span / mspan: the bytes from lo / mlo it would register
static int rooted_row(int n, int rank, int kind, int root, const RArgs &a, RRow *row, size_t *span, size_t *mspan) {
  memset(row, 0, sizeof *row);
  RRowHead &h = row->h;
  h.root = root;
  h.kind = kind;
  h.verdict = 1;
  h.lay = h.mlay = xlay_flat();
  h.unit = h.munit = 16;
  *span = *mspan = 0;
  const bool is_root = rank == root;
  h.inplace = is_root && a.inplace;
  if (!h.inplace) {
    const XDSide S = xd_side(a.ddt, kind == RK_SCATTER);
    if (!S.ok) {
      h.verdict = 0;
    } else {
      if (!xd_counts_ok(S, 1, &a.count)) return MX_ERR_ARG;
      h.bytes = a.count * S.size;
      if (h.bytes && !a.single) return MX_ERR_ARG;
      h.lay = S.lay;
      int64_t lo = INT64_MAX, hi = INT64_MIN;
      xd_span(S, a.count, 0, &lo, &hi);
      if (lo > hi) lo = hi = 0;
      h.lo = lo;
      *span = (size_t)(hi - lo);
      if (h.bytes) h.unit = xlay_unit(S.lay, (uintptr_t)a.single);
      h.mis = (uint32_t)(((uintptr_t)a.single + (uint64_t)S.lay.disp) & 15);
    }
  }
  if (!is_root) return MX_SUCCESS;
  const XDSide M = xd_side(a.mddt, kind == RK_GATHER);
  if (!M.ok) {
    h.verdict = 0;
    return MX_SUCCESS;
  }
  if (!a.counts || !a.displs || !xd_counts_ok(M, n, a.counts)) return MX_ERR_ARG;
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  uint64_t total = 0;
  for (int p = 0; p < n; p++) {
    row->mbytes[p] = a.counts[p] * M.size;
    row->moffs[p] = a.displs[p] * M.ext;
    if (p != root || !h.inplace) total += row->mbytes[p];
    xd_span(M, a.counts[p], a.displs[p], &lo, &hi);
  }
  if (total && !a.multi) return MX_ERR_ARG;
  if (lo > hi) lo = hi = 0;
  h.mlay = M.lay;
  h.mlo = lo;
  *mspan = (size_t)(hi - lo);
  if (total) h.munit = xlay_unit(M.lay, (uintptr_t)a.multi);
  h.mmis = (uint32_t)(((uintptr_t)a.multi + (uint64_t)M.lay.disp) & 15);
  return MX_SUCCESS;
}

// a communicator of one process (and a communicator of one rank): every
// block in one launch per kernel, planned before anything is launched
static int rooted_local(mx_comm *c, int kind, int root, const RArgs *args, hipStream_t s) {
  const int n = c->size;
  std::vector<RRow> rows((size_t)n);
  size_t span, mspan;
  for (int p = 0; p < n; p++)
    if (int rc = rooted_row(n, p, kind, root, args[p], &rows[(size_t)p], &span, &mspan)) return rc;
  RHead h;
  if (int rc = rooted_verdict(rows.data(), n, 0, &h)) return rc;
  if (int orc = order(c, s)) return orc;
  rcount(c, 0);
  RBufs b;
  memset(&b, 0, sizeof b);
  for (int p = 0; p < n; p++) b.single[p] = (const char *)args[p].single;
  b.multi = (const char *)args[root].multi;
  std::vector<RJob> jobs;
  rooted_local_jobs(h, rows.data(), jobs);
  if (int rc = rooted_launch(c, b, jobs, s)) return rc;
  return finish(c, s);
}

static int rooted_mp(mx_comm *c, int kind, int root, const RArgs &a, hipStream_t s) {
  const int n = c->size, r = c->rank;
  RRow all[MAXR];
  size_t span, mspan;
  if (int rc = rooted_row(n, r, kind, root, a, &all[r], &span, &mspan)) return rc;
  if (!c->reg_shm) return MX_ERR_UNSUPPORTED;   // agreed at creation: every rank returns here
  XRowExt e;
  memset(&e, 0, sizeof e);
  e.r = all[r].h;
  e.verdict = all[r].h.verdict;
  const XRow *rows = nullptr;
  if (int rc = xrow_exchange(c, (const size_t *)all[r].mbytes, (const size_t *)all[r].moffs, 64, &rows, &e)) return rc;
  for (int p = 0; p < n; p++) {
    if (!(rows[p].flags & 64)) return MX_ERR_ARG;   // another collective on some rank: every rank sees it
    all[p].h = rows[p].e.r;
    for (int q = 0; q < n; q++) {
      all[p].mbytes[q] = rows[p].bytes[q];
      all[p].moffs[q] = (int64_t)rows[p].offs[q];
    }
  }
  RHead h;
  if (int rc = rooted_verdict(all, n, c->xmin, &h)) return rc;   // the same on every rank, before any byte moves
  DoneMark dm;
  done_mark_arm(c, dm);
  rcount(c, 0);
  if (!h.max_block) return MX_SUCCESS;   // nothing moves on any rank
  RBufs b;
  memset(&b, 0, sizeof b);
  b.single[r] = (const char *)a.single;
  b.multi = (const char *)a.multi;
  for (int p = 0; p < n; p++) b.stage[p] = c->peer_staging[p];
  std::vector<RJob> jobs;
  int rc;
  if (!h.inplace && zc_allowed(c, ZC_DEFAULT, (size_t)n * (size_t)h.max_block)) {
    // zero-copy: the gather's root pulls every block from the peers'
    // registered send spans; a scatter's non-root pulls its block from the
    // root's.  A rank registers its single side, the root its multi side too.
    const char *ps[MAXR];
    char *pr[MAXR];
    const char *A = padd((const char *)a.single, (uint64_t)all[r].h.lo);
    const char *B = r == root ? padd((const char *)a.multi, (uint64_t)all[r].h.mlo) : A;
    const size_t bspan = r == root ? mspan : span;
    const int zc = reg_exchange(c, A, span, (char *)B, bspan, 0, span && bspan, ps, pr);
    if (zc < 0) return zc;
    if (zc) {
      const uint64_t g = ++c->gen;
      rcount(c, 1);
      for (int p = 0; p < n; p++)
        if (p != r) b.single[p] = padd(ps[p], (uint64_t)0 - (uint64_t)all[p].h.lo);
      if (r != root) b.multi = padd(pr[root], (uint64_t)0 - (uint64_t)all[root].h.mlo);
      if ((rc = signal_wait_mask(c, FLAG_READY, g << 1, rooted_zc_ready_mask(h, r), s))) return rc;   // the source holds its block
      rooted_zc_jobs(h, all, r, jobs);
      if ((rc = rooted_launch(c, b, jobs, s))) return rc;
      if ((rc = signal_wait_mask(c, FLAG_PUSHED, g, rooted_zc_pushed_mask(h, r), s))) return rc;   // my buffer's readers are done
      if ((rc = signal_done(c, g, s, &dm))) return rc;
      return finish_done(c, s, dm);
    }
  }
  RGeom geo;
  if (!rooted_geom(c->main_bytes, n, kind, h.max_block, &geo)) return MX_ERR_NOMEM;
  rcount(c, 2);
  for (uint64_t q = 0; q < geo.rounds; q++) {
    const uint64_t g = ++c->gen;
    rcount(c, 3);
    // The stagings this rank writes must be free.  Between the rounds of this
    // call only their owners read them: the owners' DONE(g - 1).  Before the
    // first round the generation before was another collective's, in which
    // any rank may have read a peer's staging (the PULL allreduce folds from
    // it), so there a writer waits for every rank's DONE(g - 1).
    if (uint32_t dmask = rooted_staged_done_mask(h, geo, r, q)) {
      if (q == 0) dmask = all_ranks_mask(n) & ~(1u << r);
      if ((rc = wait_mask(c, FLAG_DONE, dmask, g - 1, s))) return rc;
    }
    rooted_staged_jobs(h, all, geo, r, q, 0, jobs);
    if ((rc = rooted_launch(c, b, jobs, s))) return rc;
    if ((rc = signal_wait_mask(c, FLAG_READY, g << 1, rooted_staged_ready_mask(h, geo, r, q), s))) return rc;
    rooted_staged_jobs(h, all, geo, r, q, 1, jobs);
    if ((rc = rooted_launch(c, b, jobs, s))) return rc;
    if ((rc = signal_done(c, g, s, q + 1 == geo.rounds ? &dm : nullptr))) return rc;
  }
  return finish_done(c, s, dm);
}

static int rooted_call(mx_comm *c, int kind, int root, const RArgs &a, void *stream) {
  if (!c || (c->local && c->size != 1)) return c && c->local ? MX_ERR_STATE : MX_ERR_ARG;
  if (root < 0 || root >= c->size) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (c->size == 1) return rooted_local(c, kind, root, &a, s);   // at most one job on the caller's stream
  if (int rc = exchange_enter(c, s)) return rc;
  return rooted_mp(c, kind, root, a, s);
}

// the blocks of gather / scatter in the multi side: rank p's at p x count
struct REven {
  size_t counts[MAXR];
  int64_t displs[MAXR];
  REven(int n, size_t count) {
    for (int p = 0; p < MAXR; p++) {
      counts[p] = p < n ? count : 0;
      displs[p] = (int64_t)p * (int64_t)count;
    }
  }
};

static int rooted_local_call(mx_comm_t *c, int kind, const void *const *singles, const size_t *counts1,
                             const mx_ddt_t *ddt, const void *const *multis, const size_t *counts,
                             const int64_t *displs, const mx_ddt_t *mddt, int root, void *stream) {
  if (!c || !c->local) return MX_ERR_ARG;
  if (root < 0 || root >= c->size || !singles || !multis || !counts1) return MX_ERR_ARG;
  RArgs args[MAXR];
  for (int p = 0; p < c->size; p++) {
    const bool inplace = p == root && singles[p] == MX_IN_PLACE;
    args[p] = RArgs{singles[p], counts1[p], ddt, p == root ? multis[p] : nullptr, counts, displs, mddt, inplace};
  }
  return rooted_local(c, kind, root, args, (hipStream_t)stream);
}

}  // namespace

extern "C" int mx_gatherv(mx_comm_t *c, const void *sbuf, size_t scount, const mx_ddt_t *sddt, void *rbuf,
                          const size_t *rcounts, const int64_t *rdispls, const mx_ddt_t *rddt, int root,
                          void *stream) {
  const bool is_root = c && c->rank == root;
  return rooted_call(c, RK_GATHER, root,
                     RArgs{sbuf, scount, sddt, rbuf, rcounts, rdispls, rddt, is_root && sbuf == MX_IN_PLACE}, stream);
}

extern "C" int mx_gather(mx_comm_t *c, const void *sbuf, size_t scount, const mx_ddt_t *sddt, void *rbuf,
                         size_t rcount, const mx_ddt_t *rddt, int root, void *stream) {
  const REven ev(c ? c->size : 0, rcount);
  return mx_gatherv(c, sbuf, scount, sddt, rbuf, ev.counts, ev.displs, rddt, root, stream);
}

extern "C" int mx_scatterv(mx_comm_t *c, const void *sbuf, const size_t *scounts, const int64_t *sdispls,
                           const mx_ddt_t *sddt, void *rbuf, size_t rcount, const mx_ddt_t *rddt, int root,
                           void *stream) {
  const bool is_root = c && c->rank == root;
  return rooted_call(c, RK_SCATTER, root,
                     RArgs{rbuf, rcount, rddt, sbuf, scounts, sdispls, sddt, is_root && rbuf == MX_IN_PLACE}, stream);
}

extern "C" int mx_scatter(mx_comm_t *c, const void *sbuf, size_t scount, const mx_ddt_t *sddt, void *rbuf,
                          size_t rcount, const mx_ddt_t *rddt, int root, void *stream) {
  const REven ev(c ? c->size : 0, scount);
  return mx_scatterv(c, sbuf, ev.counts, ev.displs, sddt, rbuf, rcount, rddt, root, stream);
}

extern "C" int mx_gatherv_local(mx_comm_t *c, const void *const *sbufs, const size_t *scounts, const mx_ddt_t *sddt,
                                void *const *rbufs, const size_t *rcounts, const int64_t *rdispls,
                                const mx_ddt_t *rddt, int root, void *stream) {
  return rooted_local_call(c, RK_GATHER, sbufs, scounts, sddt, (const void *const *)rbufs, rcounts, rdispls, rddt, root,
                           stream);
}

extern "C" int mx_gather_local(mx_comm_t *c, const void *const *sbufs, size_t scount, const mx_ddt_t *sddt,
                               void *const *rbufs, size_t rcount, const mx_ddt_t *rddt, int root, void *stream) {
  const REven one(c ? c->size : 0, scount), ev(c ? c->size : 0, rcount);
  return mx_gatherv_local(c, sbufs, one.counts, sddt, rbufs, ev.counts, ev.displs, rddt, root, stream);
}

extern "C" int mx_scatterv_local(mx_comm_t *c, const void *const *sbufs, const size_t *scounts,
                                 const int64_t *sdispls, const mx_ddt_t *sddt, void *const *rbufs,
                                 const size_t *rcounts, const mx_ddt_t *rddt, int root, void *stream) {
  return rooted_local_call(c, RK_SCATTER, (const void *const *)rbufs, rcounts, rddt, sbufs, scounts, sdispls, sddt, root,
                           stream);
}

extern "C" int mx_scatter_local(mx_comm_t *c, const void *const *sbufs, size_t scount, const mx_ddt_t *sddt,
                                void *const *rbufs, size_t rcount, const mx_ddt_t *rddt, int root, void *stream) {
  const REven ev(c ? c->size : 0, scount), one(c ? c->size : 0, rcount);
  return mx_scatterv_local(c, sbufs, ev.counts, ev.displs, sddt, rbufs, one.counts, rddt, root, stream);
}

extern "C" int mx_comm_rooted_stats(mx_comm_t *c, uint64_t out[4]) {
  if (!out) return MX_ERR_ARG;
  for (int k = 0; k < 4; k++) out[k] = c ? c->rst[k] : g_rst[k].load(std::memory_order_relaxed);
  return MX_SUCCESS;
}

extern "C" long long mx_comm_rooted_rounds(const mx_comm_t *c, int scatter, size_t max_block) {
  if (!c) return MX_ERR_ARG;
  if (c->local || c->size < 2) return 0;
  RGeom geo;
  if (!rooted_geom(c->main_bytes, c->size, scatter ? RK_SCATTER : RK_GATHER, max_block, &geo)) return MX_ERR_NOMEM;
  return (long long)geo.rounds;
}

// MPI_Bcast, all-peer scatter + allgather (the reference's large-message
// bcast pipelines segments down a tree, coll_base_bcast.c:38-300; over
// point-to-point xGMI a push of the whole buffer from the root loads each
// of its links with all S bytes).  Per round of l bytes: the root pushes
// part q (blockcount split over the n-1 non-roots) into non-root q's slot q
// (S/(n-1) per root link); every non-root forwards its part into the same
// slot of every other non-root (S/(n-1) per link again) and copies it into
// its buffer; after PUSHED from the other non-roots each copies their parts
// out.  Messages up to kBcastDirectMax (and n = 2) take one step: the root
// pushes the whole round to every peer.  Pure data movement: results are the
// root's bytes.
constexpr size_t kBcastDirectMax = 512 << 10;

// the tuned entry points: candidate 0 zero-copy, 1 staged (bcast:
// 1 scatter + allgather, 2 direct)
extern "C" int mx_reduce_scatter(mx_comm_t *c, const void *sbuf, void *rbuf, const size_t *rcounts, int type,
                                 int op, int alg, void *stream) {
  int bucket = -1, cand = -1;
  const size_t es = type_size(type);
  if (c && !c->local && rcounts && es) {
    size_t total = 0;
    for (int j = 0; j < c->size; j++) total += rcounts[j];
    cand = tune_pick(c, TUNE_REDUCE_SCATTER, total * es, 2, &bucket);
  }
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = reduce_scatter_impl(c, sbuf, rbuf, rcounts, type, op, alg, stream, zc_mode_of(cand));
  return rc || cand < 0 ? rc : tune_done(c, TUNE_REDUCE_SCATTER, bucket, cand, 2, secs_since(t0));
}

extern "C" int mx_allgather(mx_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, void *stream) {
  int bucket = -1, cand = -1;
  if (c && !c->local) cand = tune_pick(c, TUNE_ALLGATHER, (size_t)c->size * bytes, 2, &bucket);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = allgather_impl(c, sbuf, rbuf, bytes, stream, zc_mode_of(cand));
  return rc || cand < 0 ? rc : tune_done(c, TUNE_ALLGATHER, bucket, cand, 2, secs_since(t0));
}

// bcast data paths: 0 zero-copy, 1 scatter + allgather, 2 direct push; -1
// the defaults (zero-copy from reg_min, direct up to kBcastDirectMax)
static int bcast_impl(mx_comm_t *c, void *buf, size_t bytes, int root, void *stream, int path) {
  if (!c || !buf || root < 0 || root >= c->size) return MX_ERR_ARG;
  if (c->local) {
    if (c->size != 1) return MX_ERR_STATE;
    void *b[1] = {buf};
    return mx_bcast_local(c, b, bytes, root, stream);
  }
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  const int n = c->size, r = c->rank, m = n - 1;
  if (!bytes || n == 1) return MX_SUCCESS;
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  char *ub = (char *)buf;
  // n slots (indexed by rank; the root's stays unused), each a part + alignment pad
  const size_t slot = (c->main_bytes / n) & ~(size_t)255;
  if (slot < 512) return MX_ERR_NOMEM;
  const size_t cb = (slot - 32) * (size_t)m;
  const uint32_t all = all_ranks_mask(n);
  auto part_of = [&](int rank) { return rank < root ? rank : rank - 1; };   // non-root -> part index
  if (zc_allowed(c, zc_mode_of(path), bytes)) {
    // zero-copy scatter + allgather: non-root q reads its part from the
    // root's registered buffer, then the other parts from their owners'
    // buffers (remote reads, local writes only)
    const char *ps[MAXR];
    char *pr[MAXR];
    const int zc = reg_exchange(c, ub, bytes, ub, bytes, (int)((uintptr_t)ub & 15), true, ps, pr);
    if (zc < 0) return zc;
    if (zc) {
      size_t off[MAXR], len[MAXR];
      blockcount(bytes, m, off, len);
      const uint64_t g = ++c->gen;
      const uint32_t nonroot = all & ~(1u << root);
      int rc;
      c->st.zero_copy_calls++;
      if ((rc = signal_all(c, FLAG_READY, g << 1, s))) return rc;
      if (r != root) {
        const int p0 = part_of(r);
        if ((rc = wait_mask(c, FLAG_READY, 1u << root, g << 1, s))) return rc;
        CopyArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.j[ca.n++] = CopyJob{ps[root] + off[p0], ub + off[p0], len[p0]};
        if ((rc = copy_launch(c, ca, s))) return rc;
        if ((rc = signal_all(c, FLAG_PUSHED, g, s))) return rc;   // my part is in my buffer
        if ((rc = wait_mask(c, FLAG_PUSHED, nonroot & ~(1u << r), g, s))) return rc;
        memset(&ca, 0, sizeof ca);
        for (int q = 0; q < n; q++)
          if (q != root && q != r) ca.j[ca.n++] = CopyJob{ps[q] + off[part_of(q)], ub + off[part_of(q)], len[part_of(q)]};
        if ((rc = copy_launch(c, ca, s))) return rc;
      }
      // nobody reads my buffer any more once every non-root is done
      if ((rc = signal_all(c, FLAG_DONE, g, s))) return rc;
      if ((rc = wait_mask(c, FLAG_DONE, nonroot & ~(1u << r), g, s))) return rc;
      return finish(c, s);
    }
  }
  const bool direct = m == 1 || (path < 0 ? bytes <= kBcastDirectMax : path == 2);
  for (size_t o = 0; o < bytes; o += cb) {
    const size_t l = std::min(cb, bytes - o);
    size_t off[MAXR], len[MAXR];
    blockcount(l, m, off, len);
    const uint64_t g = ++c->gen;
    int rc;
    if ((rc = wait_all(c, FLAG_DONE, g - 1, s))) return rc;
    auto slot_ptr = [&](char *base, int q) {   // non-root q's part in a staging area
      const size_t e = o + off[part_of(q)];
      return base + (size_t)q * slot + (e & 15);
    };
    CopyArgs ca;
    memset(&ca, 0, sizeof ca);
    if (direct) {   // small message: the root pushes it whole, one dependent step fewer
      if (r == root) {
        for (int q = 0; q < n; q++)
          if (q != root) ca.j[ca.n++] = CopyJob{ub + o, c->peer_staging[q] + (o & 15), l};
        if ((rc = copy_launch(c, ca, s))) return rc;
        if ((rc = signal_all(c, FLAG_READY, g << 1, s))) return rc;
      } else {
        if ((rc = wait_mask(c, FLAG_READY, 1u << root, g << 1, s))) return rc;
        ca.j[ca.n++] = CopyJob{c->staging + (o & 15), ub + o, l};
        if ((rc = copy_launch(c, ca, s))) return rc;
      }
    } else if (r == root) {
      for (int q = 0; q < n; q++)
        if (q != root) ca.j[ca.n++] = CopyJob{ub + o + off[part_of(q)], slot_ptr(c->peer_staging[q], q), len[part_of(q)]};
      if ((rc = copy_launch(c, ca, s))) return rc;
      if ((rc = signal_all(c, FLAG_READY, g << 1, s))) return rc;
    } else {
      const int pr = part_of(r);
      if ((rc = wait_mask(c, FLAG_READY, 1u << root, g << 1, s))) return rc;
      const char *mine = slot_ptr(c->staging, r);
      for (int q = 0; q < n; q++)
        if (q != root && q != r) ca.j[ca.n++] = CopyJob{mine, slot_ptr(c->peer_staging[q], r), len[pr]};
      ca.j[ca.n++] = CopyJob{mine, ub + o + off[pr], len[pr]};
      if ((rc = copy_launch(c, ca, s))) return rc;
      if ((rc = signal_all(c, FLAG_PUSHED, g, s))) return rc;
      if ((rc = wait_mask(c, FLAG_PUSHED, all & ~(1u << root) & ~(1u << r), g, s))) return rc;
      memset(&ca, 0, sizeof ca);
      for (int q = 0; q < n; q++)
        if (q != root && q != r) ca.j[ca.n++] = CopyJob{slot_ptr(c->staging, q), ub + o + off[part_of(q)], len[part_of(q)]};
      if ((rc = copy_launch(c, ca, s))) return rc;
    }
    if ((rc = signal_all(c, FLAG_DONE, g, s))) return rc;
  }
  return finish(c, s);
}

extern "C" int mx_bcast(mx_comm_t *c, void *buf, size_t bytes, int root, void *stream) {
  int bucket = -1, cand = -1;
  if (c && !c->local && c->size > 2) cand = tune_pick(c, TUNE_BCAST, bytes, 3, &bucket);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = bcast_impl(c, buf, bytes, root, stream, cand);
  return rc || cand < 0 ? rc : tune_done(c, TUNE_BCAST, bucket, cand, 3, secs_since(t0));
}

// ---------------------------------------------------------------------------
// rooted reduce, scan, exscan, reduce_scatter_block.
//
// The reference runs these as trees / chains of point-to-point steps
// (coll_base_reduce.c, coll_base_scan.c, coll_base_exscan.c,
// coll_base_reduce_scatter_block.c).  Here the per-element reduction order
// of the selected algorithm is derived on the host as an expression DAG over
// the n contributions -- restating the reference's topology builders
// (coll_base_topo.c) and operand roles -- compiled to a VM program
// (mx_fold.hpp k_vm), and evaluated by the owner of each element part after
// an all-peer exchange, exactly like the allreduce.  Expression nodes are
// COMB(target, source) = ompi_op_reduce(op, source, target).
// ---------------------------------------------------------------------------
namespace {

// local communicators: one VM launch over elements [lo, hi)
static int vm_run_local(vm_launch_fn vl, const VmProg &p, const char *const *src, char *const *dst, size_t lo,
                        size_t hi, size_t es, hipStream_t s) {
  if (hi <= lo) return MX_SUCCESS;
  VmArgs a;
  memset(&a, 0, sizeof a);
  for (int j = 0; j < p.nsrc; j++) a.src[j] = src[j] + lo * es;
  for (int d = 0; d < MAXR; d++) a.dst[d] = dst[d];
  a.n = hi - lo;
  a.p = p;
  return vl(a, s);
}

// multi-process: all-peer exchange of the element parts, VM fold of my part
// by every destination's program, results to the destinations' gather areas
// (or my rbuf), destinations copy the other parts in (the allreduce scheme
// of mx_allreduce with per-output destinations).
// info_rank >= 0: that rank's READY word carries the info bit of the
// guarded instructions (info_bit is this rank's own bit, sent if it is
// info_rank).
struct VmSeg { size_t lo, hi; VmProg p; };   // program for elements [lo, hi)

static int vm_partitioned(mx_comm *c, vm_launch_fn vl, const std::vector<VmSeg> &segs, const char *sb, char *rb,
                          size_t count, size_t es, uint32_t dest_mask, int info_rank, int info_bit, hipStream_t s) {
  DoneMark dm;   // the call's last DONE signal raises the completion word (blocking calls)
  done_mark_arm(c, dm);
  const int n = c->size, r = c->rank;
  const bool me_dest = (dest_mask >> r) & 1;
  // zero-copy input (as mx_allreduce): part owners read the contributions
  // straight from the registered sbufs; outputs still go through the
  // destinations' uncached gather areas
  const char *ps[MAXR];
  char *pr[MAXR];
  int zc = 0;
  if (c->reg_shm && !c->defer && c->reg_min && count * es >= c->reg_min) {
    // a rank without an output (reduce: non-root, whose rbuf MPI ignores) exports only its input
    const bool out = me_dest && rb;
    zc = reg_exchange(c, sb, count * es, out ? rb : (char *)sb, out ? count * es : 0, (int)((uintptr_t)sb & 15),
                      true, ps, pr);
    if (zc < 0) return zc;
  }
  if (zc) c->st.zero_copy_calls++;
  const size_t ce = chunk_elems(c, count, es, zc);
  for (size_t c0 = 0; c0 < count; c0 += ce) {
    const size_t cl = std::min(ce, count - c0);
    const Layout L = layout_for(n, ce, es, zc);
    size_t off[MAXR], len[MAXR];
    blockcount(cl, n, off, len);
    const uint64_t g = ++c->gen;
    int rc;
    // zero-copy writes nothing of a peer's before READY(g), which implies DONE(g-1) (mx_allreduce)
    if (!zc && (rc = wait_all(c, FLAG_DONE, g - 1, s))) return rc;
    CopyArgs ca;
    memset(&ca, 0, sizeof ca);
    for (int q = 0; q < n && !zc; q++) {
      if (q == r || !len[q]) continue;
      const size_t e0 = c0 + off[q];
      ca.j[ca.n++] = CopyJob{sb + e0 * es, c->peer_staging[q] + (size_t)r * L.slot + ((e0 * es) & 15), len[q] * es};
    }
    prof_begin(c, s);
    if ((rc = copy_launch(c, ca, s))) return rc;
    prof_end(c, s, 1, 0);
    if ((rc = signal_wait_all(c, FLAG_READY, (g << 1) | (uint64_t)(r == info_rank ? info_bit : 0), g << 1, s)))
      return rc;
    // my part [e0, e1) of this chunk, one launch per program segment in it
    const size_t e0 = c0 + off[r], e1 = e0 + len[r];
    for (const VmSeg &sg : segs) {
      const size_t lo = std::max(e0, sg.lo), hi = std::min(e1, sg.hi);
      if (lo >= hi) continue;
      const size_t mis = (e0 * es) & 15, sh = (lo - e0) * es;
      VmArgs a;
      memset(&a, 0, sizeof a);
      a.poison = c->poison;
      if (info_rank >= 0 && info_rank != r) a.info = c->flagmem + FLAG_READY * MAXR + info_rank;
      a.info_host = info_bit;
      for (int j = 0; j < n; j++)
        a.src[j] = ((j == r) ? sb + e0 * es : zc ? ps[j] + e0 * es : c->staging + (size_t)j * L.slot + mis) + sh;
      for (int d = 0; d < n; d++) {
        if (!((dest_mask >> d) & 1)) continue;
        a.dst[d] = ((d == r) ? rb + e0 * es : c->peer_staging[d] + L.gather_off + ((c0 * es) & 15) + off[r] * es) + sh;
      }
      a.n = hi - lo;
      a.p = sg.p;
      int nemit = 0;
      for (int i = 0; i < sg.p.nins; i++) nemit += (sg.p.ins[i].op & 3) == VM_EMIT;
      lag_launch(c, s);   // tests only
      prof_begin(c, s);
      if ((rc = vl(a, s))) return rc;
      prof_end(c, s, 0, (double)(n + nemit) * (double)a.n * (double)es);
    }
    if ((rc = signal_all(c, FLAG_PUSHED, g, s))) return rc;
    // zero-copy: every rank waits -- its sbuf is read by the peers' folds
    if (me_dest || zc) {
      if ((rc = wait_all(c, FLAG_PUSHED, g, s))) return rc;
    }
    if (me_dest) {
      memset(&ca, 0, sizeof ca);
      for (int q = 0; q < n; q++) {
        if (q == r || !len[q]) continue;
        ca.j[ca.n++] = CopyJob{c->staging + L.gather_off + ((c0 * es) & 15) + off[q] * es,
                               rb + (c0 + off[q]) * es, len[q] * es};
      }
      prof_begin(c, s);
      if ((rc = copy_launch(c, ca, s))) return rc;
      prof_end(c, s, 2, 0);
    }
    if ((rc = signal_done(c, g, s, c0 + ce >= count ? &dm : nullptr))) return rc;
  }
  return finish_done(c, s, dm);
}
static int vm_partitioned(mx_comm *c, vm_launch_fn vl, const VmProg &p, const char *sb, char *rb, size_t count,
                          size_t es, uint32_t dest_mask, int info_rank, int info_bit, hipStream_t s) {
  return vm_partitioned(c, vl, std::vector<VmSeg>{VmSeg{0, count, p}}, sb, rb, count, es, dest_mask, info_rank,
                        info_bit, s);
}

// Each rank folds its own block (MPI_Reduce_scatter / _block shapes): the
// pieces of block q go to rank q's slots, q evaluates `p` for its block into
// its rbuf.  Chunked over the largest block.
static int vm_scatter_blocks(mx_comm *c, vm_launch_fn vl, const VmProg &p, const char *sb, char *rb,
                             const size_t *rcounts, size_t es, hipStream_t s) {
  DoneMark dm;   // the call's last DONE signal raises the completion word (blocking calls)
  done_mark_arm(c, dm);
  const int n = c->size, r = c->rank;
  size_t disp[MAXR], total = 0, maxc = 0;
  for (int j = 0; j < n; j++) { disp[j] = total; total += rcounts[j]; maxc = std::max(maxc, rcounts[j]); }
  if (!maxc) return finish(c, s);
  if (c->reg_shm && !c->defer && c->reg_min && total * es >= c->reg_min && sb != rb) {
    // zero-copy (as mx_reduce_scatter): block r folded from every rank's
    // registered sbuf into my rbuf; IN_PLACE stays staged
    const char *ps[MAXR];
    char *pr[MAXR];
    const bool lok = (((uintptr_t)rb - ((uintptr_t)sb + disp[r] * es)) & 15) == 0;
    const int zc = reg_exchange(c, sb, total * es, rb, rcounts[r] * es, (int)((uintptr_t)sb & 15), lok, ps, pr);
    if (zc < 0) return zc;
    if (zc) {
      const uint64_t gen = ++c->gen;
      int rc;
      c->st.zero_copy_calls++;
      if ((rc = signal_wait_all(c, FLAG_READY, gen << 1, gen << 1, s))) return rc;
      if (rcounts[r]) {
        VmArgs a;
        memset(&a, 0, sizeof a);
        a.poison = c->poison;
        for (int j = 0; j < n; j++) a.src[j] = ps[j] + disp[r] * es;
        a.dst[r] = rb;
        a.n = rcounts[r];
        a.p = p;
        prof_begin(c, s);
        if ((rc = vl(a, s))) return rc;
        prof_end(c, s, 0, (double)(n + 1) * (double)rcounts[r] * (double)es);
      }
      if ((rc = signal_wait_all(c, FLAG_PUSHED, gen, gen, s))) return rc;   // done reading the peers' sbufs
      if ((rc = signal_done(c, gen, s, &dm))) return rc;
      return finish_done(c, s, dm);
    }
  }
  // IN_PLACE with my block starting inside the range my result overwrites:
  // fold into a spare slot after the n slots, then copy
  const bool overlap = sb == rb && disp[r] != 0 && disp[r] < rcounts[r];
  const size_t nslots = (size_t)n + (sb == rb ? 1 : 0);   // same geometry on every rank
  size_t kc = maxc;
  while (kc > 1 && nslots * rup(kc * es + 16, 256) > c->main_bytes) kc = (kc + 1) / 2;
  const size_t slot = rup(kc * es + 16, 256);
  if (nslots * slot > c->main_bytes) return MX_ERR_NOMEM;
  for (size_t k0 = 0; k0 < maxc; k0 += kc) {
    const uint64_t gen = ++c->gen;
    int rc;
    if ((rc = wait_all(c, FLAG_DONE, gen - 1, s))) return rc;
    CopyArgs ca;
    memset(&ca, 0, sizeof ca);
    for (int q = 0; q < n; q++) {
      if (q == r || k0 >= rcounts[q]) continue;
      const size_t e0 = disp[q] + k0;
      ca.j[ca.n++] = CopyJob{sb + e0 * es, c->peer_staging[q] + (size_t)r * slot + ((e0 * es) & 15),
                             std::min(kc, rcounts[q] - k0) * es};
    }
    prof_begin(c, s);
    if ((rc = copy_launch(c, ca, s))) return rc;
    prof_end(c, s, 1, 0);
    if ((rc = signal_wait_all(c, FLAG_READY, gen << 1, gen << 1, s))) return rc;
    if (k0 < rcounts[r]) {
      const size_t kl = std::min(kc, rcounts[r] - k0), e0 = disp[r] + k0, mis = (e0 * es) & 15;
      VmArgs a;
      memset(&a, 0, sizeof a);
      a.poison = c->poison;
      for (int j = 0; j < n; j++) a.src[j] = (j == r) ? sb + e0 * es : c->staging + (size_t)j * slot + mis;
      char *dst = overlap ? c->staging + (size_t)n * slot + mis : rb + k0 * es;
      a.dst[r] = dst;
      a.n = kl;
      a.p = p;
      // the fold stores the fields of an element only: the spare slot starts
      // as the bytes the result replaces, so the copy back keeps rbuf's padding
      if (overlap && (rc = copy_async(dst, rb + k0 * es, kl * es, s))) return rc;
      prof_begin(c, s);
      if ((rc = vl(a, s))) return rc;
      prof_end(c, s, 0, (double)(n + 1) * (double)kl * (double)es);
      if (overlap && (rc = copy_async(rb + k0 * es, dst, kl * es, s))) return rc;
    }
    if ((rc = signal_done(c, gen, s, k0 + kc >= maxc ? &dm : nullptr))) return rc;
  }
  return finish_done(c, s, dm);
}

static int vm_setup(int op, int type, vm_launch_fn *vl, size_t *es) {
  *vl = fold_fns(op, type).vm;
  if (!*vl) return MX_ERR_UNSUPPORTED;
  *es = type_size(type);
  return *es ? MX_SUCCESS : MX_ERR_ARG;
}

}  // namespace

// coll_base_reduce_scatter.c:66-88: coll_reduce of the whole vector to rank
// 0 (with MPI_IN_PLACE the root reduces in place: its own data is the
// accumulator of its combination) and a scatterv; rank q's block of that
// reduction is folded by q itself.
static int rs_nonoverlapping(mx_comm *c, const char *sb, char *rb, const size_t *rcounts, int type, int op, int alg,
                             bool allow_zc, hipStream_t s) {
  vm_launch_fn vl;
  size_t es, total = 0;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  for (int j = 0; j < c->size; j++) total += rcounts[j];
  Dag g(c->size);
  if ((rc = reduce_dag(g, reduce_word_of(alg), total, es, 0, sb == rb ? 1 : 0))) return rc;
  g.out.back().dst = -1;   // the block's owner
  VmProg p;
  if ((rc = dag_compile(g, c->rank, p))) return rc;
  const size_t keep = c->reg_min;
  if (!allow_zc) c->reg_min = 0;   // the autotuner's staged candidate
  rc = vm_scatter_blocks(c, vl, p, sb, rb, rcounts, es, s);
  c->reg_min = keep;
  return rc;
}

static int rs_nonoverlapping_local(mx_comm *c, const char *const *src, void *const *rbufs, const size_t *rcounts,
                                   int type, int op, int alg, bool inplace, hipStream_t s) {
  vm_launch_fn vl;
  size_t es, disp[MAXR], total = 0;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  const int n = c->size;
  for (int j = 0; j < n; j++) { disp[j] = total; total += rcounts[j]; }
  Dag g(n);
  if ((rc = reduce_dag(g, reduce_word_of(alg), total, es, 0, inplace ? 1 : 0))) return rc;
  g.out.back().dst = -1;
  // results go to a temporary laid out like the full vector when any rank's
  // rbuf aliases its input (they are read until the last block is folded)
  bool any_alias = false;
  for (int q = 0; q < n; q++)
    if ((const char *)rbufs[q] == src[q]) any_alias = true;
  char *tmp = nullptr;
  if (any_alias && hipMallocAsync((void **)&tmp, total * es + 16, s) != hipSuccess) return MX_ERR_NOMEM;
  for (int q = 0; q < n && !rc; q++) {
    if (!rcounts[q]) continue;
    VmProg p;
    if ((rc = dag_compile(g, q, p))) break;
    char *dst[MAXR] = {};
    dst[q] = tmp ? tmp + disp[q] * es : (char *)rbufs[q];
    rc = vm_run_local(vl, p, src, dst, disp[q], disp[q] + rcounts[q], es, s);
  }
  if (tmp) {
    CopyArgs ca;
    memset(&ca, 0, sizeof ca);
    for (int q = 0; q < n; q++)
      if (rcounts[q]) ca.j[ca.n++] = CopyJob{tmp + disp[q] * es, (char *)rbufs[q], rcounts[q] * es};
    if (!rc) rc = copy_launch(c, ca, s);
    (void)hipFreeAsync(tmp, s);
  }
  return rc ? rc : finish(c, s);
}

// ---- rooted reduce ------------------------------------------------------
extern "C" int mx_reduce_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs, size_t count, int type,
                               int op, int root, int alg, void *stream) {
  if (!c || !c->local || !rbufs || root < 0 || root >= c->size) return MX_ERR_ARG;
  vm_launch_fn vl;
  size_t es;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  const int n = c->size;
  if (count == 0) return MX_SUCCESS;
  const bool inplace = !sbufs || sbufs[root] == MX_IN_PLACE;
  const char *src[MAXR];
  char *dst[MAXR] = {};
  for (int j = 0; j < n; j++) {
    const void *sb = (sbufs && sbufs[j] != MX_IN_PLACE) ? sbufs[j] : rbufs[j];
    if (!sb) return MX_ERR_ARG;
    src[j] = (const char *)sb;
  }
  dst[root] = (char *)rbufs[root];
  if (!dst[root]) return MX_ERR_ARG;
  if ((rc = order(c, (hipStream_t)stream))) return rc;
  Dag g(n);
  if ((rc = reduce_dag(g, alg, count, es, root, inplace ? 1 : 0))) return rc;
  VmProg p;
  if ((rc = dag_compile(g, root, p))) return rc;
  if ((rc = vm_run_local(vl, p, src, dst, 0, count, es, (hipStream_t)stream))) return rc;
  return finish(c, (hipStream_t)stream);
}

extern "C" int mx_reduce(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int root,
                         int alg, void *stream) {
  if (!c || root < 0 || root >= c->size) return MX_ERR_ARG;
  const int r = c->rank;
  if (r == root && !rbuf) return MX_ERR_ARG;
  if (c->local) {
    if (c->size != 1) return MX_ERR_STATE;
    const void *sb[1] = {sbuf};
    void *rb[1] = {rbuf};
    return mx_reduce_local(c, sb, rb, count, type, op, root, alg, stream);
  }
  vm_launch_fn vl;
  size_t es;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  if (count == 0) return MX_SUCCESS;
  const bool inplace = (r == root) && (sbuf == MX_IN_PLACE || !sbuf);
  const char *sb = (sbuf == MX_IN_PLACE || !sbuf) ? (const char *)rbuf : (const char *)sbuf;
  if (!sb) return MX_ERR_ARG;
  if (c->size == 1) {
    if ((rc = copy_async(rbuf, sb, count * es, s))) return rc;
    return finish(c, s);
  }
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  // Part owners fold for the root, whose MPI_IN_PLACE choice sets the
  // operand roles of its own combination: the program carries both
  // variants, and the root's READY word tells the owners which one.
  Dag g(c->size);
  if ((rc = reduce_dag(g, alg, count, es, root, 2))) return rc;
  VmProg p;
  if ((rc = dag_compile(g, root, p))) return rc;
  return vm_partitioned(c, vl, p, sb, (char *)rbuf, count, es, 1u << root, root, inplace ? 1 : 0, s);
}

// ---- scan / exscan ------------------------------------------------------
static int scan_local_impl(mx_comm_t *c, const void *const *sbufs, void *const *rbufs, size_t count, int type,
                           int op, int alg, bool exclusive, void *stream) {
  if (!c || !c->local || !rbufs) return MX_ERR_ARG;
  vm_launch_fn vl;
  size_t es;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  const int n = c->size;
  if (count == 0) return MX_SUCCESS;
  const char *src[MAXR];
  char *dst[MAXR] = {};
  for (int j = 0; j < n; j++) {
    const void *sb = (sbufs && sbufs[j] != MX_IN_PLACE) ? sbufs[j] : rbufs[j];
    if (!sb) return MX_ERR_ARG;
    src[j] = (const char *)sb;
    dst[j] = (char *)rbufs[j];
  }
  if ((rc = order(c, (hipStream_t)stream))) return rc;
  Dag g(n);
  if ((rc = scan_dag(g, alg, exclusive))) return rc;
  if (g.out.empty()) return finish(c, (hipStream_t)stream);
  VmProg p;
  if ((rc = dag_compile(g, 0, p))) return rc;
  if ((rc = vm_run_local(vl, p, src, dst, 0, count, es, (hipStream_t)stream))) return rc;
  return finish(c, (hipStream_t)stream);
}

static int scan_impl(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                     bool exclusive, void *stream) {
  if (!c || !rbuf) return MX_ERR_ARG;
  if (c->local) {
    if (c->size != 1) return MX_ERR_STATE;
    const void *sb[1] = {sbuf};
    void *rb[1] = {rbuf};
    return scan_local_impl(c, sb, rb, count, type, op, alg, exclusive, stream);
  }
  vm_launch_fn vl;
  size_t es;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  if (count == 0) return MX_SUCCESS;
  const char *sb = (sbuf == MX_IN_PLACE || !sbuf) ? (const char *)rbuf : (const char *)sbuf;
  if (c->size == 1) {   // scan: a copy; exscan: rank 0's rbuf is undefined (left untouched)
    if (!exclusive && (rc = copy_async(rbuf, sb, count * es, s))) return rc;
    return finish(c, s);
  }
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  Dag g(c->size);
  if ((rc = scan_dag(g, alg, exclusive))) return rc;
  VmProg p;
  if ((rc = dag_compile(g, c->rank, p))) return rc;
  return vm_partitioned(c, vl, p, sb, (char *)rbuf, count, es, dest_mask_of(g, c->rank), -1, 0, s);
}

extern "C" int mx_scan_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs, size_t count, int type,
                             int op, int alg, void *stream) {
  return scan_local_impl(c, sbufs, rbufs, count, type, op, alg, false, stream);
}
extern "C" int mx_exscan_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs, size_t count, int type,
                               int op, int alg, void *stream) {
  return scan_local_impl(c, sbufs, rbufs, count, type, op, alg, true, stream);
}
extern "C" int mx_scan(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                       void *stream) {
  return scan_impl(c, sbuf, rbuf, count, type, op, alg, false, stream);
}
extern "C" int mx_exscan(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                         void *stream) {
  return scan_impl(c, sbuf, rbuf, count, type, op, alg, true, stream);
}

// ---- reduce_scatter_block -------------------------------------------------
// coll/tuned's fixed rule is basic_linear (coll_tuned_decision_fixed.c:522-532):
// coll_reduce to root 0 of rcount*n elements (the tuned reduce decision on
// that size; sbuf = rbuf for MPI_IN_PLACE, so never an IN_PLACE root) and
// a scatter (coll_base_reduce_scatter_block.c:55-110).  Rank p's block is
// folded by rank p itself.
extern "C" int mx_reduce_scatter_block_local(mx_comm_t *c, const void *const *sbufs, void *const *rbufs,
                                             size_t rcount, int type, int op, int alg, void *stream) {
  if (!c || !c->local || !rbufs) return MX_ERR_ARG;
  vm_launch_fn vl;
  size_t es;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  const int n = c->size;
  if (rcount == 0) return MX_SUCCESS;
  const char *src[MAXR];
  for (int j = 0; j < n; j++) {
    const void *sb = (sbufs && sbufs[j] != MX_IN_PLACE) ? sbufs[j] : rbufs[j];
    if (!sb || !rbufs[j]) return MX_ERR_ARG;
    src[j] = (const char *)sb;
  }
  if ((rc = order(c, (hipStream_t)stream))) return rc;
  Dag g(n);
  if ((rc = reduce_dag(g, alg, rcount * n, es, 0, 0))) return rc;
  g.out.back().dst = -1;   // the block's owner
  // block p, in order 0..n-1: with MPI_IN_PLACE rank p's result overwrites
  // its own block 0, which block 0's launch consumed first
  for (int q = 0; q < n; q++) {
    VmProg p;
    if ((rc = dag_compile(g, q, p))) return rc;
    char *dst[MAXR] = {};
    dst[q] = (char *)rbufs[q];
    if ((rc = vm_run_local(vl, p, src, dst, (size_t)q * rcount, (size_t)(q + 1) * rcount, es, (hipStream_t)stream)))
      return rc;
    // vm_run_local offsets the sources by the block start; the destination is rbufs[q][0..rcount)
  }
  return finish(c, (hipStream_t)stream);
}

extern "C" int mx_reduce_scatter_block(mx_comm_t *c, const void *sbuf, void *rbuf, size_t rcount, int type, int op,
                                       int alg, void *stream) {
  if (!c || !rbuf) return MX_ERR_ARG;
  if (c->local) {
    if (c->size != 1) return MX_ERR_STATE;
    const void *sb[1] = {sbuf};
    void *rb[1] = {rbuf};
    return mx_reduce_scatter_block_local(c, sb, rb, rcount, type, op, alg, stream);
  }
  vm_launch_fn vl;
  size_t es;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int orc = order(c, s)) return orc;
  const int n = c->size, r = c->rank;
  if (rcount == 0) return MX_SUCCESS;
  const char *sb = (sbuf == MX_IN_PLACE || !sbuf) ? (const char *)rbuf : (const char *)sbuf;
  if (n == 1) {
    if ((rc = copy_async(rbuf, sb, rcount * es, s))) return rc;
    return finish(c, s);
  }
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  Dag g(n);
  if ((rc = reduce_dag(g, alg, rcount * n, es, 0, 0))) return rc;
  g.out.back().dst = -1;
  VmProg p;
  if ((rc = dag_compile(g, r, p))) return rc;
  size_t rcounts[MAXR];
  for (int q = 0; q < n; q++) rcounts[q] = rcount;
  return vm_scatter_blocks(c, vl, p, sb, (char *)rbuf, rcounts, es, s);
}

// ---------------------------------------------------------------------------
// Non-blocking and persistent collectives.
//
// The reference runs MPI_I<coll> / MPI_<Coll>_init in coll/libnbc: a
// schedule of sends, receives and local ompi_op_reduce calls (nbc.c:523)
// that the host must progress (ompi_coll_libnbc_progress,
// coll_libnbc_component.c:426-482).  Here every collective already runs as a
// chain of kernels with device-side flag waits, so a non-blocking collective
// is the same enqueue without the final stream synchronisation: the GPU
// progresses it on its own, and the request is an event after the last
// kernel.  Reduction orders follow libnbc's schedules (its algorithm
// selection and its operand roles), not coll/tuned's, so MPI_Iallreduce
// results are bit-identical to what libnbc computes:
//   iallreduce  binomial (allred_sched_diss :365-455, root 0, then bcast),
//               ring (allred_sched_ring :629-860), Rabenseifner
//               (allred_sched_redscat_allgather :976-1180 == coll/base's),
//               recursive doubling (allred_sched_recursivedoubling
//               :512-625 == coll/base's)
//   ireduce     binomial (red_sched_binomial nbc_ireduce.c:356-458), chain
//               (red_sched_chain :461-536), Rabenseifner reduce
//               (red_sched_redscat_gather :649-: steps 1-2 == allreduce's)
//   ireduce_scatter(_block)  binomial reduce to 0 + scatter
//               (nbc_ireduce_scatter.c:103-186, nbc_ireduce_scatter_block.c)
//   iscan/iexscan  linear / recursive doubling (== coll/base's,
//               nbc_iscan.c:183-320, nbc_iexscan.c:213-350)
//   iallgather/ibcast  data movement only
// ---------------------------------------------------------------------------
namespace {

static int nbc_allreduce(mx_comm *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                         hipStream_t s) {
  const size_t es = type_size(type);
  if (!es) return MX_ERR_ARG;
  const int n = c->size;
  const bool inplace = sbuf == MX_IN_PLACE || !sbuf || sbuf == rbuf;
  if (alg == MX_IALLREDUCE_AUTO) alg = mx_iallreduce_decision(n, count, type, inplace ? 1 : 0);
  if (n == 1 || c->local || count == 0) return mx_allreduce(c, sbuf, rbuf, count, type, op, MX_ALLREDUCE_RING, s);
  switch (alg) {
    case MX_IALLREDUCE_BINOMIAL: {
      vm_launch_fn vl;
      size_t es2;
      int rc = vm_setup(op, type, &vl, &es2);
      if (rc) return rc;
      if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
      if ((rc = order(c, s))) return rc;
      Dag g(n);
      const int e = nbc_binomial_expr(g, 0);
      for (int d = 0; d < n; d++) g.emit(e, d);
      VmProg p;
      if ((rc = dag_compile(g, c->rank, p))) return rc;
      const char *sb = inplace ? (const char *)rbuf : (const char *)sbuf;
      const uint32_t all = all_ranks_mask(n);
      return vm_partitioned(c, vl, p, sb, (char *)rbuf, count, es, all, -1, 0, s);
    }
    case MX_IALLREDUCE_RECURSIVE_DOUBLING:
      return mx_allreduce(c, sbuf, rbuf, count, type, op, MX_ALLREDUCE_RECURSIVE_DOUBLING, s);
    case MX_IALLREDUCE_RABENSEIFNER:
      if (count >= (size_t)pof2_le(n))   // :121-124; otherwise ring
        return mx_allreduce(c, sbuf, rbuf, count, type, op, MX_ALLREDUCE_RABENSEIFNER, s);
      return mx_allreduce(c, sbuf, rbuf, count, type, op, kArNbcRing, s);
    default:   // 1 and anything unknown: ring (:125-127)
      return mx_allreduce(c, sbuf, rbuf, count, type, op, kArNbcRing, s);
  }
}

static int nbc_reduce(mx_comm *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int root, int alg,
                      hipStream_t s) {
  if (root < 0 || root >= c->size) return MX_ERR_ARG;
  const int n = c->size, r = c->rank;
  if (n == 1 || c->local || count == 0) return mx_reduce(c, sbuf, rbuf, count, type, op, root, MX_REDUCE_LINEAR, s);
  vm_launch_fn vl;
  size_t es;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  if (r == root && !rbuf) return MX_ERR_ARG;
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  if ((rc = order(c, s))) return rc;
  const bool inplace = (r == root) && (sbuf == MX_IN_PLACE || !sbuf || sbuf == rbuf);
  const char *sb = (sbuf == MX_IN_PLACE || !sbuf) ? (const char *)rbuf : (const char *)sbuf;
  if (!sb) return MX_ERR_ARG;
  if (alg == MX_IREDUCE_AUTO) alg = mx_ireduce_decision(n, count, type);
  else if (alg == MX_IREDUCE_RABENSEIFNER && !(n > 2 && count >= (size_t)pof2_le(n))) alg = MX_IREDUCE_CHAIN;
  else if (alg != MX_IREDUCE_BINOMIAL && alg != MX_IREDUCE_RABENSEIFNER) alg = MX_IREDUCE_CHAIN;   // :117-125
  std::vector<VmSeg> segs;
  if (alg == MX_IREDUCE_RABENSEIFNER) {
    // steps 1-2 are the allreduce's reduce-scatter: same per-element trees
    std::vector<Seg> fs;
    if ((rc = allreduce_segments(MX_ALLREDUCE_RABENSEIFNER, n, count, es, 0, count, fs))) return rc;
    for (const Seg &f : fs) {
      Dag g(n);
      g.emit(fold_expr(g, f.p), root);
      VmSeg v{f.lo, f.hi, {}};
      if ((rc = dag_compile(g, r, v.p))) return rc;
      segs.push_back(v);
    }
    return vm_partitioned(c, vl, segs, sb, (char *)rbuf, count, es, 1u << root, -1, 0, s);
  }
  Dag g(n);
  if (alg == MX_IREDUCE_BINOMIAL) {
    g.emit(nbc_binomial_expr(g, root), root);   // commutative ops: vroot = root (:369-373)
  } else {
    const int e1 = nbc_chain_expr(g, root, true), e0 = nbc_chain_expr(g, root, false);
    g.emit(e1, root, VM_IF_SET);
    g.emit(e0, root, VM_IF_CLEAR);
  }
  VmProg p;
  if ((rc = dag_compile(g, r, p))) return rc;
  return vm_partitioned(c, vl, p, sb, (char *)rbuf, count, es, 1u << root, root, inplace ? 1 : 0, s);
}

static int nbc_reduce_scatter(mx_comm *c, const void *sbuf, void *rbuf, const size_t *rcounts, int type, int op,
                              hipStream_t s) {
  const int n = c->size;
  if (n == 1 || c->local) return mx_reduce_scatter(c, sbuf, rbuf, rcounts, type, op, MX_RS_RING, s);
  vm_launch_fn vl;
  size_t es;
  int rc = vm_setup(op, type, &vl, &es);
  if (rc) return rc;
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  if ((rc = order(c, s))) return rc;
  const char *sb = (sbuf == MX_IN_PLACE || !sbuf) ? (const char *)rbuf : (const char *)sbuf;
  Dag g(n);
  g.emit(nbc_binomial_expr(g, 0), -1);   // reduce to rank 0, scatter (:103-186)
  VmProg p;
  if ((rc = dag_compile(g, c->rank, p))) return rc;
  return vm_scatter_blocks(c, vl, p, sb, (char *)rbuf, rcounts, es, s);
}

}  // namespace

namespace {

static int req_dispatch(mx_request *q, hipStream_t *done_stream) {
  mx_comm *c = q->c;
  *done_stream = q->s;
  switch (q->kind) {
    case RQ_SEND:
    case RQ_RECV: return p2p_enqueue(q, done_stream);
    case RQ_ALLREDUCE: return nbc_allreduce(c, q->sbuf, q->rbuf, q->count, q->type, q->op, q->alg, q->s);
    case RQ_REDUCE: return nbc_reduce(c, q->sbuf, q->rbuf, q->count, q->type, q->op, q->root, q->alg, q->s);
    case RQ_REDUCE_SCATTER:
    case RQ_REDUCE_SCATTER_BLOCK:
      return nbc_reduce_scatter(c, q->sbuf, q->rbuf, q->rcounts.data(), q->type, q->op, q->s);
    case RQ_SCAN:
    case RQ_EXSCAN: {
      // nbc_iscan.c:75-84 / nbc_iexscan.c:75-84: 2 = recursive doubling, else linear
      const int alg = q->alg == MX_SCAN_RECURSIVE_DOUBLING ? MX_SCAN_RECURSIVE_DOUBLING : MX_SCAN_LINEAR;
      return scan_impl(c, q->sbuf, q->rbuf, q->count, q->type, q->op, alg, q->kind == RQ_EXSCAN, q->s);
    }
    case RQ_ALLGATHER: return mx_allgather(c, q->sbuf, q->rbuf, q->count, q->s);
    case RQ_BCAST: return mx_bcast(c, q->rbuf, q->count, q->root, q->s);
  }
  return MX_ERR_ARG;
}

static int req_start(mx_request *q) {
  mx_comm *c = q->c;
  if (q->active) return MX_ERR_STATE;
  if (!c->tail && hipEventCreateWithFlags(&c->tail, hipEventDisableTiming) != hipSuccess) return MX_ERR_HIP;
  hipStream_t ds;
  c->defer = 1;
  const int rc = req_dispatch(q, &ds);
  c->defer = 0;
  if (q->kind != RQ_SEND && q->kind != RQ_RECV) {
    // whatever this call enqueued orders the communicator's next collective
    if (hipEventRecord(c->tail, q->s) != hipSuccess) return MX_ERR_HIP;
    c->tail_valid = 1;
    c->tail_stream = q->s;
  }
  if (rc) return rc;
  if (hipEventRecord(q->done, ds) != hipSuccess) return MX_ERR_HIP;
  q->active = 1;
  c->pending++;
  return MX_SUCCESS;
}

static int req_complete(mx_request *q) {
  mx_comm *c = q->c;
  q->active = 0;
  if (q->kind == RQ_SEND || q->kind == RQ_RECV) mx::p2p_finish(q);
  if (--c->pending == 0) prof_collect(c);
  if (c->err_host && *(volatile int *)c->err_host) {
    const int e = *(volatile int *)c->err_host;
    *c->err_host = 0;
    if (e == MX_ERR_TIMEOUT) c->poisoned = e;
    return e;
  }
  if (q->kind == RQ_RECV && q->status && q->status[2]) return (int)q->status[2];   // truncation / tag
  return MX_SUCCESS;
}

// Completion events of requests come from a process-wide free list: a
// hipEventCreate + hipEventDestroy pair per request is a large part of a
// small message's host cost.
static std::mutex g_ev_mu;
static std::vector<hipEvent_t> g_ev_free;

static int req_event_get(hipEvent_t *e) {
  {
    std::lock_guard<std::mutex> lk(g_ev_mu);
    if (!g_ev_free.empty()) {
      *e = g_ev_free.back();
      g_ev_free.pop_back();
      return MX_SUCCESS;
    }
  }
  return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess ? MX_SUCCESS : MX_ERR_HIP;
}

static void req_event_put(hipEvent_t e) {
  if (!e) return;
  std::lock_guard<std::mutex> lk(g_ev_mu);
  if (g_ev_free.size() < 1024) g_ev_free.push_back(e);
  else (void)hipEventDestroy(e);
}

static int req_new(mx_comm *c, int kind, int persistent, void *stream, mx_request_t **out, mx_request **q) {
  if (!c || !out) return MX_ERR_ARG;
  *out = nullptr;
  mx_request *r = new (std::nothrow) mx_request();
  if (!r) return MX_ERR_NOMEM;
  if (req_event_get(&r->done) != MX_SUCCESS) {
    delete r;
    return MX_ERR_HIP;
  }
  r->c = c;
  r->kind = kind;
  r->persistent = persistent;
  r->s = (hipStream_t)stream;
  *q = r;
  return MX_SUCCESS;
}

// non-blocking: start now; persistent: hand back an inactive request
static int req_post(mx_request *q, mx_request_t **out) {
  if (!q->persistent) {
    const int rc = req_start(q);
    if (rc) {
      req_event_put(q->done);
      mx::p2p_status_put(q->status);
      delete q;
      return rc;
    }
  }
  *out = q;
  return MX_SUCCESS;
}

static int req_reduction(mx_comm_t *c, int kind, int persistent, const void *sbuf, void *rbuf, size_t count,
                         int type, int op, int root, int alg, void *stream, mx_request_t **req) {
  mx_request *q;
  int rc = req_new(c, kind, persistent, stream, req, &q);
  if (rc) return rc;
  if (!type_size(type) || (kind != RQ_REDUCE && !rbuf)) rc = MX_ERR_ARG;
  else if (!fold_fns(op, type).vm) rc = MX_ERR_UNSUPPORTED;
  if (rc) {
    req_event_put(q->done);
    delete q;
    return rc;
  }
  q->sbuf = sbuf;
  q->rbuf = rbuf;
  q->count = count;
  q->type = type;
  q->op = op;
  q->root = root;
  q->alg = alg;
  return req_post(q, req);
}

}  // namespace

namespace mx {
int req_create(mx_comm *c, int kind, int persistent, void *stream, mx_request **q) {
  mx_request_t *dummy;
  return req_new(c, kind, persistent, stream, &dummy, q);
}
int req_submit(mx_request *q, mx_request_t **out) { return req_post(q, out); }
void req_discard(mx_request *q) {
  req_event_put(q->done);
  mx::p2p_status_put(q->status);
  delete q;
}
}  // namespace mx

extern "C" int mx_iallreduce(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                             void *stream, mx_request_t **req) {
  return req_reduction(c, RQ_ALLREDUCE, 0, sbuf, rbuf, count, type, op, 0, alg, stream, req);
}
extern "C" int mx_allreduce_init(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op,
                                 int alg, void *stream, mx_request_t **req) {
  return req_reduction(c, RQ_ALLREDUCE, 1, sbuf, rbuf, count, type, op, 0, alg, stream, req);
}
extern "C" int mx_ireduce(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int root,
                          int alg, void *stream, mx_request_t **req) {
  if (c && (root < 0 || root >= c->size)) return MX_ERR_ARG;
  return req_reduction(c, RQ_REDUCE, 0, sbuf, rbuf, count, type, op, root, alg, stream, req);
}
extern "C" int mx_reduce_init(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int root,
                              int alg, void *stream, mx_request_t **req) {
  if (c && (root < 0 || root >= c->size)) return MX_ERR_ARG;
  return req_reduction(c, RQ_REDUCE, 1, sbuf, rbuf, count, type, op, root, alg, stream, req);
}
extern "C" int mx_iscan(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                        void *stream, mx_request_t **req) {
  return req_reduction(c, RQ_SCAN, 0, sbuf, rbuf, count, type, op, 0, alg, stream, req);
}
extern "C" int mx_scan_init(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                            void *stream, mx_request_t **req) {
  return req_reduction(c, RQ_SCAN, 1, sbuf, rbuf, count, type, op, 0, alg, stream, req);
}
extern "C" int mx_iexscan(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                          void *stream, mx_request_t **req) {
  return req_reduction(c, RQ_EXSCAN, 0, sbuf, rbuf, count, type, op, 0, alg, stream, req);
}
extern "C" int mx_exscan_init(mx_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, int alg,
                              void *stream, mx_request_t **req) {
  return req_reduction(c, RQ_EXSCAN, 1, sbuf, rbuf, count, type, op, 0, alg, stream, req);
}

static int req_reduce_scatter(mx_comm_t *c, int kind, int persistent, const void *sbuf, void *rbuf,
                              const size_t *rcounts, size_t rcount, int type, int op, void *stream,
                              mx_request_t **req) {
  if (!c || (kind == RQ_REDUCE_SCATTER && !rcounts)) return MX_ERR_ARG;
  mx_request *q;
  int rc = req_new(c, kind, persistent, stream, req, &q);
  if (rc) return rc;
  if (!type_size(type) || !rbuf) rc = MX_ERR_ARG;
  else if (!fold_fns(op, type).vm) rc = MX_ERR_UNSUPPORTED;
  if (rc) {
    req_event_put(q->done);
    delete q;
    return rc;
  }
  q->sbuf = sbuf;
  q->rbuf = rbuf;
  q->type = type;
  q->op = op;
  q->rcounts.resize(c->size);
  for (int i = 0; i < c->size; i++) q->rcounts[i] = kind == RQ_REDUCE_SCATTER ? rcounts[i] : rcount;
  return req_post(q, req);
}

extern "C" int mx_ireduce_scatter(mx_comm_t *c, const void *sbuf, void *rbuf, const size_t *rcounts, int type,
                                  int op, void *stream, mx_request_t **req) {
  return req_reduce_scatter(c, RQ_REDUCE_SCATTER, 0, sbuf, rbuf, rcounts, 0, type, op, stream, req);
}
extern "C" int mx_reduce_scatter_init(mx_comm_t *c, const void *sbuf, void *rbuf, const size_t *rcounts, int type,
                                      int op, void *stream, mx_request_t **req) {
  return req_reduce_scatter(c, RQ_REDUCE_SCATTER, 1, sbuf, rbuf, rcounts, 0, type, op, stream, req);
}
extern "C" int mx_ireduce_scatter_block(mx_comm_t *c, const void *sbuf, void *rbuf, size_t rcount, int type,
                                        int op, void *stream, mx_request_t **req) {
  return req_reduce_scatter(c, RQ_REDUCE_SCATTER_BLOCK, 0, sbuf, rbuf, nullptr, rcount, type, op, stream, req);
}
extern "C" int mx_reduce_scatter_block_init(mx_comm_t *c, const void *sbuf, void *rbuf, size_t rcount, int type,
                                            int op, void *stream, mx_request_t **req) {
  return req_reduce_scatter(c, RQ_REDUCE_SCATTER_BLOCK, 1, sbuf, rbuf, nullptr, rcount, type, op, stream, req);
}

static int req_move(mx_comm_t *c, int kind, int persistent, const void *sbuf, void *buf, size_t bytes, int root,
                    void *stream, mx_request_t **req) {
  if (!c || !buf || (kind == RQ_BCAST && (root < 0 || root >= c->size))) return MX_ERR_ARG;
  mx_request *q;
  int rc = req_new(c, kind, persistent, stream, req, &q);
  if (rc) return rc;
  q->sbuf = sbuf;
  q->rbuf = buf;
  q->count = bytes;
  q->root = root;
  return req_post(q, req);
}
extern "C" int mx_iallgather(mx_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, void *stream,
                             mx_request_t **req) {
  return req_move(c, RQ_ALLGATHER, 0, sbuf, rbuf, bytes, 0, stream, req);
}
extern "C" int mx_allgather_init(mx_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, void *stream,
                                 mx_request_t **req) {
  return req_move(c, RQ_ALLGATHER, 1, sbuf, rbuf, bytes, 0, stream, req);
}
extern "C" int mx_ibcast(mx_comm_t *c, void *buf, size_t bytes, int root, void *stream, mx_request_t **req) {
  return req_move(c, RQ_BCAST, 0, nullptr, buf, bytes, root, stream, req);
}
extern "C" int mx_bcast_init(mx_comm_t *c, void *buf, size_t bytes, int root, void *stream, mx_request_t **req) {
  return req_move(c, RQ_BCAST, 1, nullptr, buf, bytes, root, stream, req);
}

extern "C" int mx_start(mx_request_t *q) {
  if (!q) return MX_ERR_ARG;
  if (!q->persistent) return MX_ERR_STATE;
  return req_start(q);
}

extern "C" int mx_startall(size_t n, mx_request_t *const *reqs) {
  if (n && !reqs) return MX_ERR_ARG;
  for (size_t i = 0; i < n; i++)
    if (int rc = mx_start(reqs[i])) return rc;
  return MX_SUCCESS;
}

// point-to-point requests whose transfer kernel is the last one complete
// through the mapped status word it raises (mx_p2p.hip, P2PDone)
static inline bool fast_done(const mx_request *q) {
  return q->fast && q->status && __atomic_load_n(&q->status[4], __ATOMIC_ACQUIRE) != 0;
}

// A rendezvous send completes only through its status word; a communicator
// error (a device wait that timed out, a corrupt channel) or poisoning ends
// the host's wait too, with that error.
static inline int rndv_failed(const mx_request *q) {
  const mx_comm *c = q->c;
  if (c->poisoned) return c->poisoned;
  return c->err_host ? *(volatile int *)c->err_host : 0;
}

extern "C" int mx_test(mx_request_t *q, int *flag) {
  if (!q || !flag) return MX_ERR_ARG;
  *flag = 1;
  if (!q->active) return MX_SUCCESS;   // completed or inactive persistent: MPI_Test gives true
  mx::p2p_progress();
  if (fast_done(q)) return req_complete(q);
  if (q->fast == 2) {                  // a rendezvous send: only its status word tells
    if (rndv_failed(q)) return req_complete(q);
    *flag = 0;
    return MX_SUCCESS;
  }
  const hipError_t e = hipEventQuery(q->done);
  if (e == hipErrorNotReady) {
    *flag = 0;
    return MX_SUCCESS;
  }
  if (e != hipSuccess) return MX_ERR_HIP;
  if (mx::p2p_rx_waiting(q)) {            // that launch yielded: launched again by p2p_progress
    *flag = 0;
    return MX_SUCCESS;
  }
  return req_complete(q);
}

// MPI_Wait: poll the completion event for up to kWaitSpinUs (a blocking
// hipEventSynchronize wakes tens of microseconds late, which is most of a
// small message's latency), then block.
constexpr double kWaitSpinUs = 2000.0;

// A point-to-point wait polls and never blocks in the runtime: every pass
// launches again the receives that yielded (mx_p2p.hip, p2p_progress) --
// this request's, or another one a peer's send waits for -- and a receive's
// event completes also when its launch yielded.
static int p2p_wait(mx_request *q) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    mx::p2p_progress();
    if (fast_done(q)) return req_complete(q);
    const bool late =
        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > kWaitSpinUs;
    if (q->fast == 2) {
      if (late) {
        if (rndv_failed(q)) return req_complete(q);
        std::this_thread::sleep_for(std::chrono::microseconds(20));
      }
      continue;
    }
    if (!q->fast || late) {
      const hipError_t e = hipEventQuery(q->done);
      if (e == hipSuccess && !mx::p2p_rx_waiting(q)) return req_complete(q);
      if (e != hipSuccess && e != hipErrorNotReady) return MX_ERR_HIP;
      if (late) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  }
}

extern "C" int mx_wait(mx_request_t *q) {
  if (!q) return MX_ERR_ARG;
  if (!q->active) return MX_SUCCESS;
  if (q->kind == RQ_SEND || q->kind == RQ_RECV) return p2p_wait(q);
  const auto t0 = std::chrono::steady_clock::now();
  if (q->fast && q->status) {
    for (;;) {
      if (fast_done(q)) return req_complete(q);
      if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > kWaitSpinUs) {
        if (q->fast != 2) break;
        if (rndv_failed(q)) return req_complete(q);
        std::this_thread::sleep_for(std::chrono::microseconds(20));   // a rendezvous send: no event to block on
      }
    }
  }
  for (;;) {
    const hipError_t e = hipEventQuery(q->done);
    if (e == hipSuccess) return req_complete(q);
    if (e != hipErrorNotReady) return MX_ERR_HIP;
    if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > kWaitSpinUs)
      break;
  }
  if (hipEventSynchronize(q->done) != hipSuccess) return MX_ERR_HIP;
  return req_complete(q);
}

// complete, without completing it (nothing changes): the tests of mx_test
static bool req_done_peek(mx_request *q) {
  if (!q->active || fast_done(q)) return true;
  if (q->fast == 2) return rndv_failed(q) != 0;
  const hipError_t e = hipEventQuery(q->done);
  if (e == hipErrorNotReady) return false;
  if (e != hipSuccess) return true;   // mx_wait reports it
  return !mx::p2p_rx_waiting(q);
}

extern "C" int mx_waitall(size_t n, mx_request_t *const *reqs) {
  if (n && !reqs) return MX_ERR_ARG;
  int rc = MX_SUCCESS;
  for (size_t i = 0; i < n; i++) {   // each wait progresses every yielded receive, not just its own
    if (!reqs[i]) continue;
    const int r = mx_wait(reqs[i]);
    if (r && !rc) rc = r;
  }
  return rc;
}

// one pass of Testany: the first complete active request (completed), or
// MX_UNDEFINED with *active = whether any entry is active
static int test_any_pass(size_t n, mx_request_t *const *reqs, int *index, bool *active) {
  mx::p2p_progress();
  *active = false;
  for (size_t i = 0; i < n; i++) {
    mx_request *q = reqs[i];
    if (!q || !q->active) continue;
    *active = true;
    if (req_done_peek(q)) {
      *index = (int)i;
      return mx_wait(q);
    }
  }
  *index = MX_UNDEFINED;
  return MX_SUCCESS;
}

extern "C" int mx_testany(size_t n, mx_request_t *const *reqs, int *index, int *flag) {
  if (!index || !flag || (n && !reqs)) return MX_ERR_ARG;
  bool active;
  const int rc = test_any_pass(n, reqs, index, &active);
  *flag = *index != MX_UNDEFINED || !active;
  return rc;
}

extern "C" int mx_waitany(size_t n, mx_request_t *const *reqs, int *index) {
  if (!index || (n && !reqs)) return MX_ERR_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    bool active;
    const int rc = test_any_pass(n, reqs, index, &active);
    if (*index != MX_UNDEFINED || !active) return rc;
    if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > kWaitSpinUs)
      std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

extern "C" int mx_testall(size_t n, mx_request_t *const *reqs, int *flag) {
  if (!flag || (n && !reqs)) return MX_ERR_ARG;
  mx::p2p_progress();
  *flag = 0;
  for (size_t i = 0; i < n; i++)
    if (reqs[i] && !req_done_peek(reqs[i])) return MX_SUCCESS;
  *flag = 1;
  return mx_waitall(n, reqs);
}

extern "C" int mx_request_stream_wait(mx_request_t *q, void *stream) {
  if (!q) return MX_ERR_ARG;
  if (!q->active) return MX_SUCCESS;
  if (q->fast == 2) {   // a rendezvous send has no event: the host waits for its status word
    while (!fast_done(q)) {
      mx::p2p_progress();
      if (const int e = rndv_failed(q)) return e;
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    return MX_SUCCESS;
  }
  if (q->kind == RQ_RECV) {
    // a receive may yield or leave a rendezvous for the host to pull: its
    // event is not its completion, so the host waits (launching yielded
    // receives again, pulls) until it is delivered
    for (;;) {
      mx::p2p_progress();
      if (fast_done(q)) return MX_SUCCESS;
      if (q->fast == 2) {   // pulled: only its status word tells
        if (const int e = rndv_failed(q)) return e;
        std::this_thread::sleep_for(std::chrono::microseconds(5));
        continue;
      }
      const hipError_t e = hipEventQuery(q->done);
      if (e == hipSuccess && !mx::p2p_rx_waiting(q)) return MX_SUCCESS;
      if (e != hipSuccess && e != hipErrorNotReady) return MX_ERR_HIP;
      std::this_thread::sleep_for(std::chrono::microseconds(5));
    }
  }
  return hipStreamWaitEvent((hipStream_t)stream, q->done, 0) == hipSuccess ? MX_SUCCESS : MX_ERR_HIP;
}

extern "C" int mx_request_is_active(const mx_request_t *q) { return q ? q->active : MX_ERR_ARG; }

extern "C" int mx_request_free(mx_request_t *q) {
  if (!q) return MX_SUCCESS;
  int rc = MX_SUCCESS;
  if (q->active) rc = mx_wait(q);   // MPI_Request_free lets an active operation finish
  req_event_put(q->done);
  mx::p2p_status_put(q->status);
  delete q;
  return rc;
}

// ---------------------------------------------------------------------------
// OpenSHMEM reductions through the allreduce (scoll/mpi, scoll_mpi_ops.c:212-275)
// ---------------------------------------------------------------------------
extern "C" int mx_shmem_to_mpi(int sop, int st, size_t dt_size, int *mx_op, int *mx_type) {
  if (!mx_op || !mx_type) return MX_ERR_ARG;
  switch (sop) {  // shmem_op_to_ompi_op
    case MX_SHMEM_AND: *mx_op = MX_OP_BAND; break;
    case MX_SHMEM_OR: *mx_op = MX_OP_BOR; break;
    case MX_SHMEM_XOR: *mx_op = MX_OP_BXOR; break;
    case MX_SHMEM_MAX: *mx_op = MX_OP_MAX; break;
    case MX_SHMEM_MIN: *mx_op = MX_OP_MIN; break;
    case MX_SHMEM_SUM: *mx_op = MX_OP_SUM; break;
    case MX_SHMEM_PROD: *mx_op = MX_OP_PROD; break;
    default: return MX_ERR_ARG;
  }
  switch (st) {  // shmem_dtype_to_ompi_dtype
    case MX_SHMEM_FLOAT: *mx_type = MX_TYPE_FLOAT; break;
    case MX_SHMEM_DOUBLE: *mx_type = MX_TYPE_DOUBLE; break;
    case MX_SHMEM_LDOUBLE: *mx_type = MX_TYPE_LONG_DOUBLE; break;
    case MX_SHMEM_FCOMPLEX: *mx_type = MX_TYPE_C_FLOAT_COMPLEX; break;
    case MX_SHMEM_DCOMPLEX: *mx_type = MX_TYPE_C_DOUBLE_COMPLEX; break;
    case MX_SHMEM_FINT4: *mx_type = MX_TYPE_INTEGER4; break;
    case MX_SHMEM_FINT8: *mx_type = MX_TYPE_INTEGER8; break;
    case MX_SHMEM_FREAL4: *mx_type = MX_TYPE_REAL4; break;
    case MX_SHMEM_FREAL8: *mx_type = MX_TYPE_REAL8; break;
    case MX_SHMEM_FREAL16: *mx_type = MX_TYPE_REAL16; break;   // no kernel (as in the reference)
    default:
      switch (dt_size * 8) {
        case 64: *mx_type = MX_TYPE_INT64_T; break;
        case 32: *mx_type = MX_TYPE_INT32_T; break;
        case 16: *mx_type = MX_TYPE_INT16_T; break;
        case 8: *mx_type = MX_TYPE_INT8_T; break;
        default: return MX_ERR_ARG;   // ompi_mpi_datatype_null
      }
  }
  return MX_SUCCESS;
}

// scoll/basic's reduce (recursive doubling, shmem_basic_rd_dag above) on the
// device: what mca_scoll_mpi_reduce runs instead of the allreduce when the
// element count exceeds INT_MAX (scoll_mpi_ops.c:246-259).  The reference's
// scoll/basic folds through oshmem's own op table, whose FINT2 AND / XOR /
// MAX / MIN / SUM functions are instantiated on ompi_fortran_integer4_t
// while the op object's dt_size is sizeof(integer2) (oshmem/op/op.c:195,
// 221, 237, 258, 281 vs :342-423): count = nlong / 2 four-byte elements,
// twice the bytes of the buffers -- an overrun of the caller's target and of
// scoll/basic's malloc(nlong) scratch.  That is not reproduced: FINT2 folds
// 2-byte integers here, as scoll/mpi's mapping gives (scoll_mpi_dtypes.h,
// FINT2 by size -> MPI_INT16_T).
extern "C" int mx_shmem_reduce_basic(mx_comm_t *c, int sop, int st, size_t dt_size, void *target, const void *source,
                                     size_t nreduce, void *stream) {
  int op, type;
  int rc = mx_shmem_to_mpi(sop, st, dt_size, &op, &type);
  if (rc) return rc;
  if (!c || !target) return MX_ERR_ARG;
  vm_launch_fn vl;
  size_t es;
  if ((rc = vm_setup(op, type, &vl, &es))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = order(c, s))) return rc;
  if (nreduce == 0) return MX_SUCCESS;
  if (c->local) {
    if (c->size != 1) return MX_ERR_STATE;
    if ((rc = copy_async(target, source, nreduce * es, s))) return rc;
    return finish(c, s);
  }
  if (c->size == 1) {
    if ((rc = copy_async(target, source, nreduce * es, s))) return rc;
    return finish(c, s);
  }
  if (!(c->flags & MX_COMM_IPC)) return MX_ERR_STATE;
  Dag g(c->size);
  if ((rc = shmem_basic_rd_dag(g))) return rc;
  VmProg p;
  if ((rc = dag_compile(g, c->rank, p))) return rc;
  return vm_partitioned(c, vl, p, (const char *)source, (char *)target, nreduce, es, dest_mask_of(g, c->rank), -1,
                        0, s);
}

extern "C" int mx_shmem_reduce(mx_comm_t *c, int sop, int st, size_t dt_size, void *target, const void *source,
                               size_t nreduce, void *stream) {
  int op, type;
  int rc = mx_shmem_to_mpi(sop, st, dt_size, &op, &type);
  if (rc) return rc;
  if (!op_has_kernel(op, type)) return MX_ERR_UNSUPPORTED;
  if (nreduce == 0) return MX_SUCCESS;
  // scoll/mpi casts the count to int for coll_allreduce and falls back to
  // the previous scoll module above INT_MAX (scoll_mpi_ops.c:246-259)
  if (nreduce > (size_t)INT_MAX)
    return mx_shmem_reduce_basic(c, sop, st, dt_size, target, source, nreduce, stream);
  return mx_allreduce(c, source == target ? MX_IN_PLACE : source, target, nreduce, type, op, MX_ALLREDUCE_AUTO,
                      stream);
}

// ---------------------------------------------------------------------------
// Device symmetric heap for OpenSHMEM.
//
// The reference's symmetric heap is host memory (sshmem segment + memheap
// allocator); RUNTIME_CHECK_ADDR rejects anything else
// (oshmem/runtime/runtime.h:205-210), so device arrays cannot take part in
// shmem_*_to_all today.  Here every PE allocates its heap in device memory
// (uncached, IPC-exported -- the role of sshmem_<x>_segment_create/attach),
// maps every peer's heap (shmem_ptr, oshmem/shmem/c/shmem_ptr.c:32-70: the
// local-node shared-memory case), and the collective allocator hands out
// the same offsets on every PE (memheap's symmetric allocation).  Because
// every PE can load and store every other PE's symmetric arrays directly,
// the reduction needs no staging: each PE folds its element part reading
// all sources over xGMI and writes the result into every target.
// Synchronisation uses per-pair sequence numbers (both sides of a pair see
// the same order of collectives involving both -- the pSync discipline), so
// collectives over different active sets never desynchronise.
// ---------------------------------------------------------------------------
namespace mx {

struct SeqSignalArgs { uint64_t *flag[MAXR]; uint64_t value[MAXR]; const int *poison; };
struct SeqWaitArgs {
  const uint64_t *flag[MAXR];
  uint64_t value[MAXR];
  uint64_t timeout_ticks;
  int *err;
  int *poison;
};

__global__ void k_seq_signal(SeqSignalArgs a) {
  const int j = threadIdx.x;
  if (poisoned(a.poison)) return;
  __threadfence_system();
  if (j < MAXR && a.flag[j]) __hip_atomic_store(a.flag[j], a.value[j], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void k_seq_wait(SeqWaitArgs a) {
  const int j = threadIdx.x;
  if (j < MAXR && a.flag[j] && !poisoned(a.poison)) {
    const uint64_t t0 = wall_clock64();
    while (__hip_atomic_load(a.flag[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < a.value[j]) {
      __builtin_amdgcn_s_sleep(2);
      if (wall_clock64() - t0 > a.timeout_ticks) {
        raise_timeout(a.err, a.poison);
        break;
      }
    }
  }
  __syncthreads();
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

}  // namespace mx

constexpr size_t kHeapFlagBytes = 4096;   // flag page at the start of each heap allocation

struct mx_heap {
  mx_comm *c;
  size_t bytes;                 // usable symmetric bytes
  int carved;                   // 1: a slice of the communicator's heap region (no own IPC export)
  size_t region_off;            // offset of the slice in the region
  char *mem;                    // my allocation: flag page + heap
  char *base;                   // my heap
  char *peer[MAXR];             // every PE's heap, mapped here
  uint64_t *flags;              // my flag page: word p = sequence number signalled by PE p
  uint64_t *peer_flags[MAXR];
  uint64_t seq[MAXR];           // syncs done with PE p
  size_t brk;                   // symmetric allocator: bump pointer + first-fit free list
  std::map<size_t, size_t> live, freed;
};

namespace {
struct heap_info { hipIpcMemHandle_t h; uint64_t bytes; };

// one synchronisation step among the PEs in `mask` (this PE included)
static int heap_sync(mx_heap *h, uint32_t mask, hipStream_t s) {
  mx_comm *c = h->c;
  if (c->poisoned) return c->poisoned;
  SeqSignalArgs sa;
  SeqWaitArgs wa;
  memset(&sa, 0, sizeof sa);
  memset(&wa, 0, sizeof wa);
  for (int p = 0; p < c->size; p++) {
    if (p == c->rank || !((mask >> p) & 1)) continue;
    const uint64_t v = ++h->seq[p];
    sa.flag[p] = h->peer_flags[p] + c->rank;
    sa.value[p] = v;
    wa.flag[p] = h->flags + p;
    wa.value[p] = v;
  }
  wa.timeout_ticks = c->timeout_ticks;
  wa.err = c->err_dev;
  wa.poison = c->poison;
  sa.poison = c->poison;
  hipLaunchKernelGGL(k_seq_signal, dim3(1), dim3(64), 0, s, sa);
  int rc = mx_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(k_seq_wait, dim3(1), dim3(64), 0, s, wa);
  return mx_check_launch();
}

static bool heap_has(const mx_heap *h, const void *p, size_t bytes) {
  const uintptr_t q = (uintptr_t)p, b = (uintptr_t)h->base;
  return q >= b && bytes <= h->bytes && q - b <= h->bytes - bytes;
}
}  // namespace

namespace {
// every PE contributes `ok`; true iff all PEs are ok (and the exchange worked)
static bool heap_agree(mx_comm *c, int ok) {
  std::vector<int> all(c->size, 0);
  if (c->ag(&ok, all.data(), sizeof(int), c->ag_ctx) != 0) return false;
  for (int v : all)
    if (!v) return false;
  return true;
}

// a heap's operations end before they return (blocking) or are tracked by
// its communicator's tail event (deferred mode, finish()): that is all the
// device work destroy must wait for
static void heap_quiesce(mx_heap *h) {
  mx_comm *c = h->c;
  if (c->tail_valid && c->tail && hipEventSynchronize(c->tail) != hipSuccess) (void)hipGetLastError();
}

static void heap_unmap(mx_heap *h) {
  for (int p = 0; p < h->c->size && p < MAXR; p++) {
    if (p != h->c->rank && h->peer_flags[p]) release_later((void *)h->peer_flags[p], REL_IPC);
    if (p != h->c->rank) { h->peer_flags[p] = nullptr; h->peer[p] = nullptr; }
  }
}

// One collective attempt at exporting my heap allocation and mapping every
// peer's.  Every PE makes the same sequence of exchanges whatever fails
// locally, so a failure on one PE never strands the others in an exchange.
// The mappings are verified by reading each PE's signature word through
// them: on this image an IPC import has been seen (intermittently, 4
// processes on one GPU) to return a mapping of another PE's buffer, which
// would otherwise surface as a hang or wrong data much later.
static bool heap_map_attempt(mx_heap *h) {
  mx_comm *c = h->c;
  const int dbg = getenv("MX_DEBUG_IPC") != nullptr;
  heap_info mine;
  memset(&mine, 0, sizeof mine);
  int ok = hipIpcGetMemHandle(&mine.h, h->mem) == hipSuccess;
  mine.bytes = ok ? h->bytes : 0;
  std::vector<heap_info> all(c->size);
  if (c->ag(&mine, all.data(), sizeof mine, c->ag_ctx) != 0) return false;
  for (int p = 0; p < c->size; p++) {
    if (p == c->rank || !ok) continue;
    char *m = nullptr;
    if (all[p].bytes != h->bytes) ok = 0;   // shmem heaps are the same size everywhere
    else if (hipIpcOpenMemHandle((void **)&m, all[p].h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
      fprintf(stderr, "mx_heap_create: rank %d cannot map PE %d's heap\n", c->rank, p);
      ok = 0;
    } else {
      h->peer[p] = m + kHeapFlagBytes;
      h->peer_flags[p] = (uint64_t *)m;
    }
  }
  const uint64_t sig = 0x5EED0000ull + (uint64_t)c->rank;
  hipStream_t ls = life_stream();
  if (ok && (hipMemcpyAsync(h->flags + 256, &sig, sizeof sig, hipMemcpyHostToDevice, ls) != hipSuccess ||
             hipStreamSynchronize(ls) != hipSuccess))
    ok = 0;
  if (!heap_agree(c, ok)) return false;   // every PE mapped and signed before anyone checks
  for (int p = 0; p < c->size; p++) {
    uint64_t v = 0;
    hipError_t e = hipMemcpyAsync(&v, h->peer_flags[p] + 256, sizeof v, hipMemcpyDeviceToHost, ls);
    if (e == hipSuccess) e = hipStreamSynchronize(ls);
    if (dbg) fprintf(stderr, "[mx ipc] rank %d: PE %d mapped at %p reads 0x%llx\n", c->rank, p,
                     (void *)h->peer_flags[p], (unsigned long long)v);
    if (e != hipSuccess || v != 0x5EED0000ull + (uint64_t)p) {
      fprintf(stderr, "mx_heap_create: rank %d reads 0x%llx through its mapping of PE %d's heap; remapping\n",
              c->rank, (unsigned long long)v, p);
      ok = 0;
    }
  }
  return heap_agree(c, ok);               // nobody uses the heap before every PE checked its mappings
}
}  // namespace

extern "C" int mx_heap_create(mx_comm_t *c, size_t bytes, mx_heap_t **out) {
  if (!c || !out || !bytes) return MX_ERR_ARG;
  if (c->local && c->size != 1) return MX_ERR_STATE;
  if (!c->local && (!(c->flags & MX_COMM_IPC) || !c->ag)) return MX_ERR_STATE;
  int rc = mx_ensure_init();
  if (rc) return rc;
  mx_heap *h = new (std::nothrow) mx_heap();
  if (!h) return MX_ERR_NOMEM;
  h->c = c;
  h->bytes = (bytes + 255) & ~(size_t)255;
  // preferred: a slice of the heap region mapped (and verified) at
  // communicator creation -- the same sequence on every PE gives the same
  // offset, and no new IPC export is needed
  if (c->hregion && c->hregion_used + kHeapFlagBytes + h->bytes <= c->hregion_bytes) {
    h->carved = 1;
    h->region_off = c->hregion_used;
    c->hregion_used += kHeapFlagBytes + h->bytes;
    for (int p = 0; p < c->size; p++) {
      h->peer_flags[p] = (uint64_t *)(c->peer_hregion[p] + h->region_off);
      h->peer[p] = c->peer_hregion[p] + h->region_off + kHeapFlagBytes;
    }
    h->mem = c->hregion + h->region_off;
    h->flags = (uint64_t *)h->mem;
    h->base = h->mem + kHeapFlagBytes;
    // flag words start at 0 on every PE before anyone signals.  The slice may
    // have served an earlier heap: zero it only once every PE is past that
    // heap's destroy (its device idle, its trailing sequence writes landed),
    // else a late write of the old heap survives the zeroing (as the
    // communicator flags did in round 3)
    hipStream_t ls = life_stream();
    int ok = heap_agree(c, 1) && hipMemsetAsync(h->mem, 0, kHeapFlagBytes, ls) == hipSuccess &&
             hipStreamSynchronize(ls) == hipSuccess;
    if (!heap_agree(c, ok)) {
      c->hregion_used = h->region_off;
      delete h;
      return MX_ERR_HIP;
    }
    *out = h;
    return MX_SUCCESS;
  }
  std::vector<char *> discarded;   // failed attempts' buffers stay allocated until we succeed (fresh VAs)
  bool mapped = false;
  for (int attempt = 0; attempt < 3 && !mapped; attempt++) {
    int ok = hipExtMallocWithFlags((void **)&h->mem, kHeapFlagBytes + h->bytes, hipDeviceMallocUncached) ==
             hipSuccess;
    hipStream_t ls = life_stream();
    if (ok && (hipMemsetAsync(h->mem, 0, kHeapFlagBytes, ls) != hipSuccess ||
               hipStreamSynchronize(ls) != hipSuccess))
      ok = 0;
    if (!ok) h->mem = nullptr;
    if (c->local) {
      mapped = ok;
      if (!ok) break;
    } else if (!heap_agree(c, ok)) {
      if (h->mem) discarded.push_back(h->mem);
      h->mem = nullptr;
      break;                       // an allocation failed somewhere: give up together
    }
    h->base = h->mem + kHeapFlagBytes;
    h->flags = (uint64_t *)h->mem;
    h->peer[c->rank] = h->base;
    h->peer_flags[c->rank] = h->flags;
    if (c->local) break;
    mapped = heap_map_attempt(h);
    if (!mapped) {
      heap_unmap(h);
      discarded.push_back(h->mem);
      h->mem = nullptr;
    }
  }
  for (char *m : discarded) release_later(m, REL_DEV);
  if (!mapped) {
    release_later(h->mem, REL_DEV);
    delete h;
    return MX_ERR_HIP;
  }
  *out = h;
  return MX_SUCCESS;
}

extern "C" int mx_heap_destroy(mx_heap_t *h) {
  if (!h) return MX_SUCCESS;
  // the heap's own operations only (every heap call records its stream's
  // event), never the whole device
  heap_quiesce(h);
  if (h->carved) {   // give the slice back if it is the last one (heaps are destroyed in LIFO order)
    if (h->region_off + kHeapFlagBytes + h->bytes == h->c->hregion_used) h->c->hregion_used = h->region_off;
    delete h;
    return MX_SUCCESS;
  }
  heap_unmap(h);
  release_later(h->mem, REL_DEV);
  delete h;
  release_flush();
  return MX_SUCCESS;
}

extern "C" void *mx_heap_base(const mx_heap_t *h) { return h ? h->base : nullptr; }

// Symmetric allocation: every PE makes the same calls in the same order
// (shmem_malloc is collective), so first-fit over the same free list gives
// the same offset everywhere.
extern "C" void *mx_shmalloc(mx_heap_t *h, size_t bytes) {
  if (!h || !bytes) return nullptr;
  const size_t need = (bytes + 255) & ~(size_t)255;
  for (auto it = h->freed.begin(); it != h->freed.end(); ++it) {
    if (it->second >= need) {
      const size_t off = it->first, rest = it->second - need;
      h->freed.erase(it);
      if (rest) h->freed[off + need] = rest;
      h->live[off] = need;
      return h->base + off;
    }
  }
  if (h->brk + need > h->bytes) return nullptr;
  const size_t off = h->brk;
  h->brk += need;
  h->live[off] = need;
  return h->base + off;
}

extern "C" int mx_shfree(mx_heap_t *h, void *p) {
  if (!h || !p) return MX_ERR_ARG;
  const size_t off = (size_t)((char *)p - h->base);
  auto it = h->live.find(off);
  if (it == h->live.end()) return MX_ERR_ARG;
  size_t start = off, len = it->second;
  h->live.erase(it);
  auto nx = h->freed.lower_bound(start);              // coalesce with neighbours
  if (nx != h->freed.end() && nx->first == start + len) { len += nx->second; h->freed.erase(nx); }
  auto pv = h->freed.lower_bound(start);
  if (pv != h->freed.begin()) {
    --pv;
    if (pv->first + pv->second == start) { start = pv->first; len += pv->second; h->freed.erase(pv); }
  }
  if (start + len == h->brk) h->brk = start;           // give the tail back to the bump pointer
  else h->freed[start] = len;
  return MX_SUCCESS;
}

extern "C" void *mx_shmem_ptr(const mx_heap_t *h, const void *addr, int pe) {
  if (!h || pe < 0 || pe >= h->c->size || !heap_has(h, addr, 1)) return nullptr;
  return h->peer[pe] + ((const char *)addr - h->base);
}

extern "C" int mx_shmem_putmem(mx_heap_t *h, void *dest, const void *src, size_t bytes, int pe, void *stream) {
  if (!h || !dest || !src || !heap_has(h, dest, bytes)) return MX_ERR_ARG;
  void *remote = mx_shmem_ptr(h, dest, pe);
  if (!remote) return MX_ERR_ARG;
  int rc = copy_async(remote, src, bytes, (hipStream_t)stream);
  return rc ? rc : finish(h->c, (hipStream_t)stream);
}

extern "C" int mx_shmem_getmem(mx_heap_t *h, void *dest, const void *src, size_t bytes, int pe, void *stream) {
  if (!h || !dest || !src || !heap_has(h, src, bytes)) return MX_ERR_ARG;
  const void *remote = mx_shmem_ptr(h, src, pe);
  if (!remote) return MX_ERR_ARG;
  int rc = copy_async(dest, remote, bytes, (hipStream_t)stream);
  return rc ? rc : finish(h->c, (hipStream_t)stream);
}

extern "C" int mx_shmem_barrier_all(mx_heap_t *h, void *stream) {
  if (!h) return MX_ERR_ARG;
  const uint32_t all = all_ranks_mask(h->c->size);
  int rc = heap_sync(h, all, (hipStream_t)stream);
  return rc ? rc : finish(h->c, (hipStream_t)stream);
}

// shmem_<type>_<op>_to_all over the active set (PE_start, logPE_stride,
// PE_size) with symmetric target/source (oshmem/shmem/c/shmem_reduce.c:29-65).
// The fold order is the one scoll/mpi would get from coll/tuned on a
// communicator of the active set (mx_allreduce_decision over PE_size ranks,
// virtual rank = position in the active set), so results equal
// mx_shmem_reduce's bit for bit.
extern "C" int mx_shmem_reduce_heap(mx_heap_t *h, int sop, int st, size_t dt_size, void *target,
                                    const void *source, size_t nreduce, int pe_start, int log_pe_stride,
                                    int pe_size, void *stream) {
  if (!h || !target || !source) return MX_ERR_ARG;
  mx_comm *c = h->c;
  int op, type;
  int rc = mx_shmem_to_mpi(sop, st, dt_size, &op, &type);
  if (rc) return rc;
  fold_launch_fn fl = fold_fns(op, type).fold;
  if (!fl || !op_has_kernel(op, type)) return MX_ERR_UNSUPPORTED;
  const size_t es = type_size(type);
  if (pe_size < 1 || pe_size > MAXR || pe_start < 0 || log_pe_stride < 0 || log_pe_stride > 5) return MX_ERR_ARG;
  int members[MAXR], me = -1;
  uint32_t mask = 0;
  for (int i = 0; i < pe_size; i++) {
    members[i] = pe_start + (i << log_pe_stride);
    if (members[i] >= c->size) return MX_ERR_ARG;
    mask |= 1u << members[i];
    if (members[i] == c->rank) me = i;
  }
  if (me < 0) return MX_ERR_ARG;   // only the active set calls (RUNTIME_CHECK_PE semantics)
  if (!heap_has(h, target, nreduce * es) || !heap_has(h, source, nreduce * es)) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (nreduce == 0) return MX_SUCCESS;
  const int n = pe_size;
  if (n == 1) {
    if ((rc = copy_async(target, source, nreduce * es, s))) return rc;
    return finish(c, s);
  }
  // (1) every member's source is final; (2) each member folds its part from
  // all sources into all targets; (3) every target is complete
  if ((rc = heap_sync(h, mask, s))) return rc;
  size_t off[MAXR], len[MAXR];
  blockcount(nreduce, n, off, len);
  if (len[me]) {
    std::vector<Seg> segs;
    if ((rc = allreduce_segments(MX_ALLREDUCE_AUTO, n, nreduce, es, off[me], off[me] + len[me], segs))) return rc;
    const char *sp[MAXR];
    char *dp[MAXR];
    const size_t so = (size_t)((const char *)source - h->base) + off[me] * es;
    const size_t to = (size_t)((char *)target - h->base) + off[me] * es;
    for (int j = 0; j < n; j++) {
      sp[j] = h->peer[members[j]] + so;
      dp[j] = h->peer[members[j]] + to;
    }
    for (const Seg &sg : segs)
      if ((rc = run_fold(c, fl, sg, off[me], sp, n, dp, n, es, s))) return rc;
  }
  if ((rc = heap_sync(h, mask, s))) return rc;
  return finish(c, s);
}

// ---------------------------------------------------------------------------
// One-sided accumulate on symmetric device memory.
//
// MPI_Accumulate / MPI_Get_accumulate / MPI_Fetch_and_op /
// MPI_Compare_and_swap with a target in another GPU's symmetric heap.  The
// reference's osc/rdma, without network atomics, takes the target's
// accumulate lock, reads the target region, applies ompi_op_reduce(op,
// origin, tmp) and writes it back (ompi_osc_rdma_gacc_contig,
// osc_rdma_accumulate.c:188-251; the same process for a local target:
// ompi_osc_rdma_gacc_local :121-168 -> ompi_osc_base_sndrcv_op,
// osc_base_obj_convert.c:160-253).  Here the target region is directly
// addressable over xGMI, so the op kernel itself (k_reduce2, in = origin,
// inout = the mapped target) is the read-modify-write; an exclusive lock
// word in the target heap's flag page (system-scope CAS from a one-thread
// kernel, released after a system fence) serialises it against every other
// accumulate on that PE, which is the MPI per-element atomicity guarantee.
// Non-contiguous datatypes go through the convertor kernels: origin packed
// once, target region gathered, combined element for element in type-map
// order (what ompi_osc_base_sndrcv_op's paired iovec walk does), scattered
// back -- all under the lock.  Every call completes before it returns (the
// flush of osc/rdma folded into the call).
// ---------------------------------------------------------------------------
namespace mx {

constexpr size_t kAccLockWord = 384;   // heap flag page: words 0..15 pair sequences, 256 signature

__global__ void k_acc_lock(uint64_t *lock, uint64_t tag, uint64_t timeout_ticks, int *err, int *poison) {
  if (threadIdx.x == 0 && !poisoned(poison)) {
    const uint64_t t0 = wall_clock64();
    uint64_t expect = 0;
    while (!__hip_atomic_compare_exchange_strong(lock, &expect, tag, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_SYSTEM)) {
      expect = 0;
      __builtin_amdgcn_s_sleep(4);
      if (wall_clock64() - t0 > timeout_ticks) {
        raise_timeout(err, poison);
        break;
      }
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

__global__ void k_acc_unlock(uint64_t *lock) {
  if (threadIdx.x == 0) {
    __threadfence_system();   // the target update is visible before the lock is free
    __hip_atomic_store(lock, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// compare-and-swap of one element (osc_rdma_accumulate.c:170-186 semantics):
// result = target; if (target == compare, bytewise) target = origin
__global__ void k_cas_bytes(char *target, const char *compare, const char *origin, char *result, int es) {
  if (threadIdx.x == 0) {
    bool eq = true;
    for (int i = 0; i < es; i++) {
      const char t = target[i];
      result[i] = t;
      eq = eq && t == compare[i];
    }
    if (eq)
      for (int i = 0; i < es; i++) target[i] = origin[i];
  }
}

}  // namespace mx

namespace {

static uint64_t *acc_lock_word(mx_heap *h, int pe) {
  return (pe == h->c->rank ? h->flags : h->peer_flags[pe]) + kAccLockWord;
}

static int acc_lock(mx_heap *h, int pe, hipStream_t s) {
  hipLaunchKernelGGL(k_acc_lock, dim3(1), dim3(64), 0, s, acc_lock_word(h, pe), (uint64_t)h->c->rank + 1,
                     h->c->timeout_ticks, h->c->err_dev, h->c->poison);
  int rc = mx_check_launch();
  // with a bounded wait the lock may not have been taken: find out before
  // the read-modify-write runs (the element kernels take no poison word)
  if (!rc && h->c->timeout_ticks != ~(uint64_t)0) {
    if (hipStreamSynchronize(s) != hipSuccess) return MX_ERR_HIP;
    if (*(volatile int *)h->c->err_host) rc = finish(h->c, s);
  }
  return rc;
}

static int acc_unlock(mx_heap *h, int pe, hipStream_t s) {
  hipLaunchKernelGGL(k_acc_unlock, dim3(1), dim3(64), 0, s, acc_lock_word(h, pe));
  return mx_check_launch();
}

static bool acc_op_ok(int op, int type) {
  if (!type_size(type)) return false;
  return op == MX_OP_REPLACE || op == MX_OP_NO_OP || op_has_kernel(op, type);
}

// target op= origin on `count` elements at `remote` (lock held)
static int acc_apply(int op, int type, const void *origin, void *remote, size_t count, hipStream_t s) {
  if (op == MX_OP_NO_OP || !count) return MX_SUCCESS;
  if (op == MX_OP_REPLACE) return copy_async(remote, origin, count * type_size(type), s);
  return mx_reduce2(op, type, origin, remote, count, s);
}

static int acc_common(mx_heap *h, const void *origin, void *result, size_t count, int type, int op, int pe,
                      void *target, void *stream) {
  if (!h || pe < 0 || pe >= h->c->size || !target) return MX_ERR_ARG;
  if (!acc_op_ok(op, type)) return MX_ERR_UNSUPPORTED;
  const size_t es = type_size(type);
  if (!heap_has(h, target, count * es) || (!origin && op != MX_OP_NO_OP && count)) return MX_ERR_ARG;
  void *remote = mx_shmem_ptr(h, target, pe);
  if (!remote) return MX_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (!count) return MX_SUCCESS;
  int rc;
  if ((rc = acc_lock(h, pe, s))) return rc;
  if (result && (rc = copy_async(result, remote, count * es, s))) return rc;   // fetch the old value
  if ((rc = acc_apply(op, type, origin, remote, count, s))) return rc;
  if ((rc = acc_unlock(h, pe, s))) return rc;
  return finish(h->c, s);
}

}  // namespace

extern "C" int mx_accumulate(mx_heap_t *h, const void *origin, size_t count, int type, int op, int pe, void *target,
                             void *stream) {
  return acc_common(h, origin, nullptr, count, type, op, pe, target, stream);
}

extern "C" int mx_get_accumulate(mx_heap_t *h, const void *origin, void *result, size_t count, int type, int op,
                                 int pe, void *target, void *stream) {
  if (!result) return MX_ERR_ARG;
  return acc_common(h, origin, result, count, type, op, pe, target, stream);
}

extern "C" int mx_fetch_and_op(mx_heap_t *h, const void *origin, void *result, int type, int op, int pe,
                               void *target, void *stream) {
  if (!result) return MX_ERR_ARG;
  return acc_common(h, origin, result, 1, type, op, pe, target, stream);
}

extern "C" int mx_compare_and_swap(mx_heap_t *h, const void *origin, const void *compare, void *result, int type,
                                   int pe, void *target, void *stream) {
  if (!h || !origin || !compare || !result || pe < 0 || pe >= h->c->size) return MX_ERR_ARG;
  const size_t es = type_size(type);
  if (!es || !heap_has(h, target, es)) return MX_ERR_ARG;
  void *remote = mx_shmem_ptr(h, target, pe);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = acc_lock(h, pe, s))) return rc;
  hipLaunchKernelGGL(k_cas_bytes, dim3(1), dim3(64), 0, s, (char *)remote, (const char *)compare,
                     (const char *)origin, (char *)result, (int)es);
  if ((rc = mx_check_launch())) return rc;
  if ((rc = acc_unlock(h, pe, s))) return rc;
  return finish(h->c, s);
}

// Derived datatypes on either side (NULL = `count` contiguous elements of
// `type`); both sides carry the same number of `type` elements.
extern "C" int mx_accumulate_ddt(mx_heap_t *h, const void *origin, size_t origin_count, const mx_ddt_t *origin_ddt,
                                 int type, int op, int pe, void *target, size_t target_count,
                                 const mx_ddt_t *target_ddt, void *stream) {
  if (!h || pe < 0 || pe >= h->c->size || !target || (!origin && op != MX_OP_NO_OP)) return MX_ERR_ARG;
  if (!acc_op_ok(op, type)) return MX_ERR_UNSUPPORTED;
  const size_t es = type_size(type);
  const size_t obytes = origin_ddt ? origin_count * mx_ddt_size(origin_ddt) : origin_count * es;
  const size_t tbytes = target_ddt ? target_count * mx_ddt_size(target_ddt) : target_count * es;
  if (obytes != tbytes || obytes % es) return MX_ERR_ARG;
  if (!obytes) return MX_SUCCESS;
  int64_t lo = 0, hi = (int64_t)tbytes;
  if (target_ddt && mx_ddt_span(target_ddt, target_count, &lo, &hi)) return MX_ERR_ARG;
  if (!heap_has(h, (const char *)target + lo, (size_t)(hi - lo))) return MX_ERR_ARG;
  char *remote = (char *)mx_shmem_ptr(h, (const char *)target + lo, pe) - lo;
  hipStream_t s = (hipStream_t)stream;
  char *po = nullptr, *pt = nullptr;
  int rc = MX_SUCCESS;
  const size_t nel = obytes / es;
  if (origin_ddt && hipMallocAsync((void **)&po, obytes, s) != hipSuccess) return MX_ERR_NOMEM;
  if (target_ddt && hipMallocAsync((void **)&pt, tbytes, s) != hipSuccess) rc = MX_ERR_NOMEM;
  if (!rc && po) rc = mx_pack(origin_ddt, origin_count, origin, po, 0, obytes, s);
  const void *osrc = po ? (const void *)po : origin;
  if (!rc) rc = acc_lock(h, pe, s);
  if (!rc) {
    if (!pt) {
      rc = acc_apply(op, type, osrc, remote, nel, s);
    } else {
      // gather the target region, combine in type-map order, scatter back
      if (op != MX_OP_REPLACE) rc = mx_pack(target_ddt, target_count, remote, pt, 0, tbytes, s);
      if (!rc) rc = acc_apply(op == MX_OP_REPLACE ? MX_OP_REPLACE : op, type, osrc, pt, nel, s);
      if (!rc && op != MX_OP_NO_OP) rc = mx_unpack(target_ddt, target_count, remote, pt, 0, tbytes, s);
    }
    const int urc = acc_unlock(h, pe, s);
    if (!rc) rc = urc;
  }
  if (po) (void)hipFreeAsync(po, s);
  if (pt) (void)hipFreeAsync(pt, s);
  return rc ? rc : finish(h->c, s);
}
