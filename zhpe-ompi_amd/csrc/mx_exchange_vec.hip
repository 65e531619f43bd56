// mx_exchange_vec.hip -- k_exchange_vec: one launch moves a table of jobs
// whose sides are one-run strided layouts (alltoall / alltoallv of vector,
// hvector and resized datatypes: transposes, pencil redistributions, halo
// columns).  The sender's layout is read and the receiver's written in ONE
// pass: no packed buffer, no pack and unpack launches around an exchange.
//
// Work assignment (mx_exchange_vec_plan.hpp): a job is cut in its STREAM into
// blocks of xv_block_bytes(W), W the job's word width (4, 8 or 16: the
// largest word both layouts, both addresses and the cut allow); blocks are
// dealt round-robin over the jobs that still have some through the segment
// table of the byte kernel (mx_exchange_plan.hpp), so ragged tables get
// workgroups by bytes.
//
// Body: lane t of a workgroup owns the words t, t + 256, ... of its block's
// stretch of the stream.  A flat side is then one coalesced access per wave
// instruction; a strided side touches only the lines that hold data.  The
// stretch start is mapped once per workgroup and strided side (two 64-bit
// multiply-shift divisions); every word is mapped from it in 32-bit
// arithmetic (float-reciprocal quotient by blen made exact by the remainder
// correction, as k_convert_vec does; xv_start / xv_off in
// mx_exchange_vec_plan.hpp, which the host check runs too).  All of a lane's words are loaded
// before any is stored.  W divides blen, so a word never leaves its block:
// nothing outside the receive layout's own bytes is written.  Every access is
// a global_* word (mx_mem.hpp), non-temporal when the launch streams more
// than the Infinity Cache holds (mx_nt_for).
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <vector>

#include "mx_exchange.hpp"
#include "mx_fold.hpp"
#include "mx_internal.h"
#include "mx_mem.hpp"

namespace mx {

struct XVArgs {
  uint32_t njobs;
  uint64_t block0;    // first block of this launch
  const int *poison;
  XVJob jobs[kXInline];
  XSeg seg[kXInline + 1];
};
static_assert(sizeof(XVArgs) <= 4096, "the tables travel in the kernel's argument block");

// SF / DF: the source / destination side is flat (no division on that side)
template <int W, bool SF, bool DF, bool NT>
__device__ __forceinline__ void xvmove(const XVJob &jb, uint64_t k) {
  using U = typename gword<W>::T;
  constexpr unsigned IT = xv_iters(W);
  const uint64_t b0 = k * xv_block_bytes(W);             // the block's first byte of the job
  const uint64_t left = jb.bytes - b0;
  const uint32_t nw = left / W < (uint64_t)kXThreads * IT ? (uint32_t)(left / W) : kXThreads * IT;
  XVStart ss = {}, ds = {};
  const char *sflat = jb.src + jb.s.l.disp + jb.pos_s + b0;
  char *dflat = jb.dst + jb.d.l.disp + jb.pos_d + b0;
  if constexpr (!SF) ss = xv_start(jb.s, jb.pos_s + b0);
  if constexpr (!DF) ds = xv_start(jb.d, jb.pos_d + b0);
  U v[IT];
  char *da[IT];
#pragma unroll
  for (unsigned u = 0; u < IT; u++) {
    const uint32_t w = u * kXThreads + threadIdx.x;
    if (w < nw) {
      const char *sa = SF ? sflat + (size_t)w * W : jb.src + xv_off(jb.s, ss, w * W);
      da[u] = DF ? dflat + (size_t)w * W : jb.dst + xv_off(jb.d, ds, w * W);
      v[u] = ldw<NT, W>(sa);
    }
  }
#pragma unroll
  for (unsigned u = 0; u < IT; u++) {
    const uint32_t w = u * kXThreads + threadIdx.x;
    if (w < nw) stw<NT, W>(da[u], v[u]);
  }
}

template <int W, bool NT>
__device__ __forceinline__ void xvsides(const XVJob &jb, uint64_t k) {
  const bool sf = xlay_is_flat(jb.s.l), df = xlay_is_flat(jb.d.l);   // uniform over the workgroup
  if (sf && !df) xvmove<W, true, false, NT>(jb, k);
  else if (!sf && df) xvmove<W, false, true, NT>(jb, k);
  else if (!sf && !df) xvmove<W, false, false, NT>(jb, k);
  // flat / flat jobs stay with k_exchange (exchange_vec_launch sends them there)
}

// one instance per word width: the registers a lane needs follow its words
template <int W, bool NT>
__global__ void __launch_bounds__(kXThreads) k_exchange_vec(XVArgs a) {
  if (poisoned(a.poison)) return;
  uint32_t j;
  uint64_t k;
  xplan_lookup(a.seg, a.njobs, a.block0 + blockIdx.x, &j, &k);
  const XVJob &jb = a.jobs[j];
  xvsides<W, NT>(jb, k);
}

template <int W>
static int xv_launch(const XVArgs &a, const XLaunch &l, bool nt, hipStream_t s) {
  if (nt) hipLaunchKernelGGL((k_exchange_vec<W, true>), dim3(l.nblocks), dim3(kXThreads), 0, s, a);
  else hipLaunchKernelGGL((k_exchange_vec<W, false>), dim3(l.nblocks), dim3(kXThreads), 0, s, a);
  return mx_check_launch();
}

static std::atomic<uint64_t> g_xvw[3];   // jobs launched by width (mx_exchange_vec_widths)

int exchange_vec_launch(const XVJob *jobs, size_t n, const int *poison, hipStream_t s) {
  // flat / flat jobs are the byte kernel's
  std::vector<XJob> flat;
  std::vector<XVJob> vec;
  for (size_t i = 0; i < n; i++) {
    if (!jobs[i].bytes) continue;
    if (xlay_is_flat(jobs[i].s.l) && xlay_is_flat(jobs[i].d.l))
      flat.push_back(XJob{jobs[i].src + jobs[i].s.l.disp + jobs[i].pos_s, jobs[i].dst + jobs[i].d.l.disp + jobs[i].pos_d,
                          (size_t)jobs[i].bytes});
    else vec.push_back(jobs[i]);
  }
  if (!flat.empty())
    if (int rc = exchange_launch(flat.data(), flat.size(), poison, s)) return rc;
  // the jobs of one width are one launch (the jobs of a call share their
  // datatypes, so a call is one launch unless its addresses differ in alignment)
  size_t bytes = 0;
  for (const XVJob &jb : vec) bytes += jb.bytes;
  const bool nt = mx_nt_for(2 * bytes);
  for (unsigned W : {16u, 8u, 4u}) {
    std::vector<XVJob> grp;
    for (const XVJob &jb : vec)
      if (jb.W == W) grp.push_back(jb);
    XVPlan p;
    if (int rc = xvplan_build(grp.data(), grp.size(), p)) return rc;
    for (size_t i = 0; i < p.jobs.size(); i += kXInline) {   // kXInline jobs at a time
      const size_t J = std::min<size_t>(kXInline, p.jobs.size() - i);
      XVPlan q;
      if (p.jobs.size() <= (size_t)kXInline) q = p;
      else if (int rc = xvplan_build(p.jobs.data() + i, J, q)) return rc;
      XVArgs a;
      memset(&a, 0, sizeof a);
      a.njobs = (uint32_t)J;
      a.poison = poison;
      memcpy(a.jobs, q.jobs.data(), J * sizeof(XVJob));
      memcpy(a.seg, q.seg.data(), (J + 1) * sizeof(XSeg));
      g_xvw[W == 4 ? 0 : W == 8 ? 1 : 2].fetch_add(J, std::memory_order_relaxed);
      for (const XLaunch &l : q.launch) {   // more than one only past 2^32 grid threads
        a.block0 = l.block0;
        const int rc = W == 4 ? xv_launch<4>(a, l, nt, s) : W == 8 ? xv_launch<8>(a, l, nt, s) : xv_launch<16>(a, l, nt, s);
        if (rc) return rc;
      }
    }
  }
  return MX_SUCCESS;
}

}  // namespace mx

extern "C" int mx_exchange_vec_geometry(unsigned W, size_t *block_bytes, size_t *wave_bytes) {
  if (W != 4 && W != 8 && W != 16) return MX_ERR_ARG;
  if (block_bytes) *block_bytes = mx::xv_block_bytes(W);
  if (wave_bytes) *wave_bytes = mx::xv_wave_bytes(W);
  return MX_SUCCESS;
}

extern "C" int mx_exchange_vec_widths(uint64_t out[3]) {
  if (!out) return MX_ERR_ARG;
  for (int k = 0; k < 3; k++) out[k] = mx::g_xvw[k].load(std::memory_order_relaxed);
  return MX_SUCCESS;
}
