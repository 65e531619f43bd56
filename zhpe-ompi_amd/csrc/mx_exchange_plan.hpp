// mx_exchange_plan.hpp -- host-only planning of the exchange kernel's launches
// (mx_exchange_plan.hip): the job table, the block -> job prefix table, the
// split into launches, the staging rounds and the argument checks of
// alltoall / alltoallv / allgatherv.  No HIP API, no communicator, no
// launch: it compiles with a host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "../../include/mx_kernels.h"
#include "../../include/mx_coll.h"

#ifdef __HIPCC__
#define MX_XHD __host__ __device__
#else
#define MX_XHD
#endif

namespace mx {

// ---- geometry of k_exchange (mx_exchange.hip) ------------------------------
// A workgroup of kXThreads lanes moves kXVec 16-byte vectors per lane: one
// wave covers kXWaveBytes contiguous destination bytes per step, a workgroup
// kXBlockBytes in all.  Blocks are cut in the DESTINATION's 16-byte grid
// (from dst rounded down to 16), so every store of the body is aligned.
constexpr unsigned kXThreads = 256;
constexpr unsigned kXVec = 4;
constexpr size_t kXWaveBytes = 64 * 16;
constexpr size_t kXBlockBytes = (size_t)kXThreads * kXVec * 16;
// HIP: a grid holds fewer than 2^32 threads
constexpr uint64_t kXMaxGridBlocks = (((uint64_t)1 << 32) - 1) / kXThreads;
constexpr int kXMaxJobs = MX_MAX_RANKS * MX_MAX_RANKS;

struct XJob {
  const char *src;
  char *dst;
  size_t bytes;
};

// blocks of a job: the 16-byte-aligned span around [dst, dst + bytes) in
// pieces of kXBlockBytes
MX_XHD inline uint64_t xjob_blocks(uintptr_t dst, size_t bytes) {
  return bytes ? ((uint64_t)(dst & 15) + bytes + kXBlockBytes - 1) / kXBlockBytes : 0;
}
// the bytes [*lo, *hi) of the job (offsets from dst) that its block k moves
MX_XHD inline void xjob_block_range(uintptr_t dst, size_t bytes, uint64_t k, size_t *lo, size_t *hi) {
  const size_t md = dst & 15;
  const uint64_t a = k * kXBlockBytes, b = a + kXBlockBytes;   // in the aligned span
  *lo = a > md ? (size_t)(a - md) : 0;
  *hi = b - md < bytes ? (size_t)(b - md) : bytes;
  if (*lo > *hi) *lo = *hi;
}

// Block -> job map.  Jobs are dealt round by round: round t holds block t of
// every job that has more than t blocks, in table order, so consecutive
// blocks belong to different jobs (different destination ranges -- a push
// loads every peer link from the first wave) for as long as more than one
// job has blocks left, and every job gets blocks in proportion to its bytes.
// With the jobs sorted by block count (stable: callers list jobs so that
// neighbours go to different peers, and equal-sized jobs keep that order)
// the rounds [seg[i].round0, seg[i+1].round0) all hold the jobs i..njobs-1,
// so a block finds its job from the segment that holds it:
//   t = round0 + (b - block0) / (njobs - i),  job = i + (b - block0) % (njobs - i)
struct XSeg {
  uint64_t block0;   // first block of the segment
  uint64_t round0;   // its first round
};
struct XLaunch {
  uint64_t block0;   // first block of the launch
  uint32_t nblocks;  // its grid
};
struct XPlan {
  std::vector<XJob> jobs;     // non-empty jobs, ascending block count
  std::vector<XSeg> seg;      // jobs.size() + 1 entries; seg.back().block0 = all blocks
  std::vector<XLaunch> launch;
  uint64_t nblocks = 0;
  size_t bytes = 0;           // moved in all
};
template <class SegPtr>   // const XSeg * (the kernel: its global-address-space form)
MX_XHD inline void xplan_lookup(SegPtr seg, uint32_t njobs, uint64_t b, uint32_t *job, uint64_t *k) {
  uint32_t lo = 0, hi = njobs;   // the last segment i with seg[i].block0 <= b
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (seg[mid].block0 <= b) lo = mid;
    else hi = mid;
  }
  const uint64_t o = b - seg[lo].block0, alive = njobs - lo;
  if ((o >> 32) == 0) {   // the usual case: a 32-bit division
    *job = lo + (uint32_t)o % (uint32_t)alive;
    *k = seg[lo].round0 + (uint32_t)o / (uint32_t)alive;
  } else {
    *job = lo + (uint32_t)(o % alive);
    *k = seg[lo].round0 + o / alive;
  }
}

// The segment and launch tables of J jobs with ascending block counts nb[0..J);
// returns the blocks in all.
uint64_t xplan_tables(const uint64_t *nb, size_t J, uint64_t max_grid_blocks, std::vector<XSeg> &seg,
                      std::vector<XLaunch> &launch);

// Builds the plan of one launch group from `n` jobs (empty jobs dropped).
// max_grid_blocks: the launch split (kXMaxGridBlocks; tests pass less).
int xplan_build(const XJob *jobs, size_t n, XPlan &out, uint64_t max_grid_blocks = kXMaxGridBlocks);

// ---- staging rounds ----------------------------------------------------------
// A staged call moves every pair through a slot of `cap` bytes: round q
// carries the bytes [q*cap, (q+1)*cap) of each pair that is that long.  The
// round count comes from the largest pair and is the same on every rank.
inline uint64_t xrounds(size_t max_pair, size_t cap) { return cap ? (max_pair + cap - 1) / cap : 0; }
inline void xround_piece(size_t pair_bytes, size_t cap, uint64_t q, size_t *off, size_t *len) {
  const uint64_t a = q * cap;
  *off = a < pair_bytes ? (size_t)a : pair_bytes;
  *len = pair_bytes - *off < cap ? pair_bytes - *off : cap;
}
// slot geometry of a staging of `main_bytes` shared by n senders: the slot
// stride and what a round carries per pair (16 bytes of every slot are kept
// for the source's misalignment).  false: the staging is too small.
bool xstage_slots(size_t main_bytes, int n, size_t *slot, size_t *cap);

// ---- argument checks -----------------------------------------------------------
// sizes / offsets of one rank's row: non-null, off + bytes does not wrap
int xcheck_row(int n, const size_t *bytes, const size_t *offs);
// the receive ranges of one buffer are pairwise disjoint (MPI requires it;
// the in-place forms rely on it)
bool xranges_disjoint(int n, const size_t *bytes, const size_t *offs);

}  // namespace mx
