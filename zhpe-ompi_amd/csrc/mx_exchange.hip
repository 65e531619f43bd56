// mx_exchange.hip -- k_exchange: one launch moves a table of byte jobs
// (alltoall, alltoallv, allgatherv; the reference runs them as n-1 pairwise
// or linear point-to-point steps, coll_base_alltoall.c:132-, 569-,
// coll_base_alltoallv.c:125-, 189-, coll_base_allgatherv.c:93-579).
//
// Work assignment (mx_exchange_plan.hpp): every job is cut into blocks of
// kXBlockBytes in its DESTINATION's 16-byte grid, so a job gets workgroups in
// proportion to its bytes and ragged tables waste none; blocks are dealt
// round-robin over the jobs that still have some, so consecutive workgroups
// write to different destinations, and a workgroup finds its job with a
// binary search of the segment table (uniform: scalar loads).
//
// Body: lane l of a workgroup owns the destination granules l, l + 256, ...
// of its block (a wave stores kXWaveBytes contiguous bytes per step).  The
// source bytes of destination granule g start d = (src - dst) mod 16 bytes
// into source granule g of the source's own 16-byte grid, so the stored
// vector is built from the aligned loads of source granules g and g + 1:
// d == 0 copies, d a multiple of 4 selects dwords, any other d funnel-shifts
// neighbouring dwords (a 64-bit shift, v_lshrrev_b64).  Every access is a global_* 16-byte
// load or store (mx_mem.hpp), non-temporal when the launch streams more than
// the Infinity Cache holds (mx_nt_for).
//
// Edges: a granule the job covers only partly -- the first and the last of
// a job, nowhere else -- is written with byte stores of exactly the covered
// bytes, and a source granule is loaded only if it holds a byte the job
// moves.  Nothing outside [dst, dst + bytes) is written; reads stay inside
// the 16-byte granules the source range touches.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <new>
#include <vector>

#include "mx_exchange.hpp"
#include "mx_fold.hpp"
#include "mx_internal.h"
#include "mx_mem.hpp"

namespace mx {

struct XArgs {
  const XJob *jobs;   // device tables, or null: the inline ones
  const XSeg *seg;
  uint32_t njobs;
  uint64_t block0;    // first block of this launch
  const int *poison;
  XJob ijobs[kXInline];
  XSeg iseg[kXInline + 1];
};

// the four stored dwords from the eight loaded ones (w[0..3] source granule
// g, w[4..7] granule g + 1), DQ whole dwords and db bytes in
template <int DQ>
__device__ __forceinline__ void xshift(const uint32_t (&w)[8], unsigned db, uint32_t (&o)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (db == 0) o[i] = w[i + DQ];
    else o[i] = (uint32_t)((((uint64_t)w[i + DQ + 1] << 32) | w[i + DQ]) >> (8 * db));
  }
}

// DQ < 0: source and destination share their misalignment
template <bool NT, int DQ>
__device__ __forceinline__ void xmove(const char *S, char *A, size_t md, size_t bytes, size_t g0, unsigned d) {
  const size_t span = md + bytes;          // the job in its destination's aligned span: [md, span)
  const size_t G = (span + 15) >> 4;       // granules of the span
  const unsigned db = d & 3;
  uint4 lo[kXVec], hi[kXVec];
  unsigned jlo[kXVec], jhi[kXVec];         // the job's bytes of granule g: [jlo, jhi), 0 / 0 = none
#pragma unroll
  for (unsigned u = 0; u < kXVec; u++) {
    const size_t g = g0 + (size_t)u * kXThreads;
    lo[u] = make_uint4(0, 0, 0, 0);
    hi[u] = make_uint4(0, 0, 0, 0);
    jlo[u] = jhi[u] = 0;
    if (g < G) {
      jlo[u] = g == 0 ? (unsigned)md : 0;
      jhi[u] = span - g * 16 < 16 ? (unsigned)(span - g * 16) : 16;
      // source granule g holds the stored bytes [0, 16 - d), granule g + 1 the rest
      if (jlo[u] < 16 - d) ld16<NT>(lo[u], reinterpret_cast<const uint4 *>(S) + g);
      if (DQ >= 0 && jhi[u] > 16 - d) ld16<NT>(hi[u], reinterpret_cast<const uint4 *>(S) + g + 1);
    }
  }
#pragma unroll
  for (unsigned u = 0; u < kXVec; u++) {
    if (jhi[u] == 0) continue;
    const size_t g = g0 + (size_t)u * kXThreads;
    uint32_t o[4];
    if constexpr (DQ < 0) {
      o[0] = lo[u].x; o[1] = lo[u].y; o[2] = lo[u].z; o[3] = lo[u].w;
    } else {
      const uint32_t w[8] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z, hi[u].w};
      xshift<DQ>(w, db, o);
    }
    if (jlo[u] == 0 && jhi[u] == 16) {
      st16<NT>(reinterpret_cast<uint4 *>(A) + g, make_uint4(o[0], o[1], o[2], o[3]));
    } else {   // a job's first or last granule, partly its own: byte stores of exactly its bytes
      unsigned char *q = reinterpret_cast<unsigned char *>(A) + g * 16;
#pragma unroll
      for (unsigned j = 0; j < 16; j++)
        if (j >= jlo[u] && j < jhi[u]) *gp(q + j) = (unsigned char)(o[j >> 2] >> (8 * (j & 3)));
    }
  }
}

template <bool NT>
__global__ void __launch_bounds__(kXThreads) k_exchange(XArgs a) {
  if (poisoned(a.poison)) return;
  const uint64_t b = a.block0 + blockIdx.x;
  uint32_t j;
  uint64_t k;
  XJob jb;
  if (a.jobs) {
    xplan_lookup(gp(a.seg), a.njobs, b, &j, &k);
    jb.src = gp(a.jobs)[j].src;
    jb.dst = gp(a.jobs)[j].dst;
    jb.bytes = gp(a.jobs)[j].bytes;
  } else {
    xplan_lookup(a.iseg, a.njobs, b, &j, &k);
    jb = a.ijobs[j];
  }
  const size_t md = (uintptr_t)jb.dst & 15;
  const unsigned d = (unsigned)(((uintptr_t)jb.src - (uintptr_t)jb.dst) & 15);
  char *A = jb.dst - md;                 // destination granule g: A + 16 g
  const char *S = jb.src - md - d;       // 16-byte aligned; granule g's bytes start at S + 16 g + d
  const size_t g0 = (size_t)k * (kXThreads * kXVec) + threadIdx.x;
  if (d == 0) xmove<NT, -1>(S, A, md, jb.bytes, g0, 0);
  else
    switch (d >> 2) {   // uniform over the workgroup
      case 0: xmove<NT, 0>(S, A, md, jb.bytes, g0, d); break;
      case 1: xmove<NT, 1>(S, A, md, jb.bytes, g0, d); break;
      case 2: xmove<NT, 2>(S, A, md, jb.bytes, g0, d); break;
      default: xmove<NT, 3>(S, A, md, jb.bytes, g0, d); break;
    }
}

constexpr size_t kXTableBytes = (size_t)kXMaxJobs * sizeof(XJob) + ((size_t)kXMaxJobs + 1) * sizeof(XSeg);

static std::atomic<int> g_xtables{0};   // tables alive (mx_exchange_tables_live)

XTable *xtable_new() {
  XTable *t = new (std::nothrow) XTable();
  if (!t) return nullptr;
  g_xtables.fetch_add(1, std::memory_order_relaxed);
  bool ok = true;
  for (int k = 0; k < 2; k++) {
    t->host[k] = (char *)pool_host_get(kXTableBytes);
    t->dev[k] = (char *)pool_dev_get(kXTableBytes);
    ok = ok && t->host[k] && t->dev[k] && hipEventCreateWithFlags(&t->ev[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) { t->ev[k] = nullptr; break; }
  }
  if (!ok) {
    xtable_free(t);
    return nullptr;
  }
  return t;
}

void xtable_free(XTable *t) {
  if (!t) return;
  for (int k = 0; k < 2; k++) {
    if (t->ev[k]) {
      if (t->used[k]) (void)hipEventSynchronize(t->ev[k]);
      (void)hipEventDestroy(t->ev[k]);
    }
    if (t->host[k]) pool_host_put(t->host[k], kXTableBytes);
    if (t->dev[k]) pool_dev_put(t->dev[k], kXTableBytes);
  }
  delete t;
  g_xtables.fetch_sub(1, std::memory_order_relaxed);
}

int exchange_launch(const XJob *jobs, size_t n, const int *poison, hipStream_t s, XTable *tab) {
  XPlan p;
  if (int rc = xplan_build(jobs, n, p)) return rc;
  const size_t J = p.jobs.size();
  if (!J) return MX_SUCCESS;
  if (J > (size_t)kXInline && !tab) {   // no table memory: kXInline jobs at a time
    for (size_t i = 0; i < J; i += kXInline)
      if (int rc = exchange_launch(p.jobs.data() + i, std::min<size_t>(kXInline, J - i), poison, s)) return rc;
    return MX_SUCCESS;
  }
  XArgs a;
  memset(&a, 0, sizeof a);
  a.njobs = (uint32_t)J;
  a.poison = poison;
  int slot = -1;
  if (J <= (size_t)kXInline) {
    memcpy(a.ijobs, p.jobs.data(), J * sizeof(XJob));
    memcpy(a.iseg, p.seg.data(), (J + 1) * sizeof(XSeg));
  } else {
    const size_t jb = J * sizeof(XJob), sb = (J + 1) * sizeof(XSeg);
    slot = (int)(tab->next++ & 1);
    // the slot's last launch (copy and kernels) is over before it is rewritten
    if (tab->used[slot] && hipEventSynchronize(tab->ev[slot]) != hipSuccess) return MX_ERR_HIP;
    memcpy(tab->host[slot], p.jobs.data(), jb);
    memcpy(tab->host[slot] + jb, p.seg.data(), sb);
    if (hipMemcpyAsync(tab->dev[slot], tab->host[slot], jb + sb, hipMemcpyHostToDevice, s) != hipSuccess)
      return MX_ERR_HIP;
    a.jobs = (const XJob *)tab->dev[slot];
    a.seg = (const XSeg *)(tab->dev[slot] + jb);
  }
  const bool nt = mx_nt_for(2 * p.bytes);
  int rc = MX_SUCCESS;
  for (const XLaunch &l : p.launch) {   // more than one only past 2^32 grid threads
    a.block0 = l.block0;
    if (nt) hipLaunchKernelGGL(k_exchange<true>, dim3(l.nblocks), dim3(kXThreads), 0, s, a);
    else hipLaunchKernelGGL(k_exchange<false>, dim3(l.nblocks), dim3(kXThreads), 0, s, a);
    if ((rc = mx_check_launch())) break;
  }
  if (slot >= 0) {
    tab->used[slot] = hipEventRecord(tab->ev[slot], s) == hipSuccess;
    if (!tab->used[slot]) {   // no event to wait for later: wait now
      (void)hipStreamSynchronize(s);
      if (!rc) rc = MX_ERR_HIP;
    }
  }
  return rc;
}

}  // namespace mx

extern "C" int mx_exchange_tables_live(void) { return mx::g_xtables.load(std::memory_order_relaxed); }

extern "C" int mx_exchange_geometry(size_t *block_bytes, size_t *wave_bytes) {
  if (block_bytes) *block_bytes = mx::kXBlockBytes;
  if (wave_bytes) *wave_bytes = mx::kXWaveBytes;
  return MX_SUCCESS;
}
