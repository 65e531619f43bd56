// mx_exchange_vec_plan.hpp -- host-only planning of the strided exchange
// kernel (k_exchange_vec, mx_exchange_vec.hip): which datatypes it takes, the
// description of one side of a job, the word width of a job and the block ->
// job tables of a launch.  No HIP API, no communicator, no launch: it
// compiles with a host compiler (mx_exchange_vec_plan.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "mx_ddt_layout.hpp"
#include "mx_exchange_plan.hpp"

namespace mx {

// One side of a job, all in bytes.  Byte b of the stream of the side's
// instances lives at  user + i*ext + disp + l*stride1 + o  with B = b / blen,
// o = b % blen, i = B / cnt1, l = B % cnt1 -- the map of the convertor's VEC
// kernel (k_convert_vec).  blen == 0 is a FLAT side: byte b lives at
// user + disp + b (a staging slot, bytes, a contiguous datatype).
struct XLay {
  int64_t disp;
  uint64_t blen, cnt1;
  int64_t stride1, ext;
};
inline XLay xlay_flat(int64_t disp = 0) { return XLay{disp, 0, 1, 0, 1}; }
MX_XHD inline bool xlay_is_flat(const XLay &l) { return l.blen == 0; }

// offset from `user` of stream byte b (the brute-force form of the map)
MX_XHD inline int64_t xlay_off(const XLay &l, uint64_t b) {
  if (l.blen == 0) return l.disp + (int64_t)b;
  const uint64_t B = b / l.blen, o = b % l.blen, i = B / l.cnt1, k = B % l.cnt1;
  return (int64_t)i * l.ext + l.disp + (int64_t)k * l.stride1 + (int64_t)o;
}

// floor(n / d) for n < 2^kMagicBits through d's Magic
MX_XHD inline uint64_t xudiv(uint64_t n, const Magic &M) { return (uint64_t)(((unsigned __int128)n * M.m) >> M.k); }

// Qualification: one run of one level (what MPI_Type_vector, hvector and
// resized contiguous types flatten to), blocks of at most kVecMaxBlen bytes,
// and on the receiving side a monotonic layout (no byte written twice).  A
// run of one block per instance whose extent is the block is flat.
bool xlay_from(const DdtLayout &L, bool receive_side, XLay *out);

// Access unit: the largest power of two <= 16 that divides every value given
// (0 divides by all).  A side's unit takes blen, disp, stride1, ext and the
// buffer address; a job's word width W the units of both sides, both stream
// positions and its bytes.
MX_XHD inline unsigned xunit_of(uint64_t v, unsigned u = 16) {
  while (u > 1 && (v & (u - 1))) u >>= 1;
  return u;
}
inline uint64_t xabs(int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; }
unsigned xlay_unit(const XLay &l, uintptr_t addr);

struct XSide {
  XLay l;
  Magic mblen, mcnt1;
};
struct XVJob {
  const char *src;   // the `user` of the source side
  char *dst;
  XSide s, d;
  uint64_t pos_s, pos_d;   // where the job starts in either side's stream
  uint64_t bytes;
  uint32_t W, pad;         // word width: 4, 8 or 16
};

// ---- geometry of k_exchange_vec ----------------------------------------------
// Lane t of a workgroup owns the W-byte words t, t + kXThreads, ... of its
// block's stretch of the job's stream, xv_iters(W) of them (16-byte words
// take four: eight of them with their addresses leave two waves a SIMD): a
// wave covers 64 * W contiguous stream bytes per step, a workgroup
// kXThreads * xv_iters(W) * W -- 8, 16 and 16 KiB for W = 4, 8 and 16.
MX_XHD constexpr unsigned xv_iters(unsigned W) { return W == 16 ? 4 : 8; }
MX_XHD inline size_t xv_wave_bytes(unsigned W) { return (size_t)64 * W; }
MX_XHD inline size_t xv_block_bytes(unsigned W) { return (size_t)kXThreads * xv_iters(W) * W; }
MX_XHD inline uint64_t xvjob_blocks(uint64_t bytes, unsigned W) {
  return (bytes + xv_block_bytes(W) - 1) / xv_block_bytes(W);
}

// ---- the kernel's form of the map (shared with the host check) -----------------
// Where a workgroup's stretch starts in a strided side, found once per
// workgroup with two 64-bit multiply-shift divisions; every word of the
// stretch is then mapped from it in 32-bit arithmetic: a stretch is at most
// 16 KiB of words of 4 bytes and more, so it crosses fewer than 2^14 blocks.
struct XVStart {
  int64_t base0;    // offset from `user` of block 0 of the instance the stretch starts in
  int64_t baseL;    // ... of the block it starts in
  uint32_t o0;      // the stretch's first byte within that block
  uint32_t room;    // blocks from there to the end of the instance (clipped to 2^31)
  uint32_t cnt1;    // blocks per instance (clipped to 2^31)
  float rblen, rcnt1;
};
MX_XHD inline XVStart xv_start(const XSide &S, uint64_t p0) {
  XVStart st;
  const uint64_t B0 = xudiv(p0, S.mblen);
  const uint64_t i0 = xudiv(B0, S.mcnt1), l0 = B0 - i0 * S.l.cnt1;
  const uint64_t clip = (uint64_t)1 << 31;
  st.o0 = (uint32_t)(p0 - B0 * S.l.blen);
  st.base0 = (int64_t)i0 * S.l.ext + S.l.disp;
  st.baseL = st.base0 + (int64_t)l0 * S.l.stride1;
  st.room = (uint32_t)(S.l.cnt1 - l0 < clip ? S.l.cnt1 - l0 : clip);
  st.cnt1 = (uint32_t)(S.l.cnt1 < clip ? S.l.cnt1 : clip);
  st.rblen = 1.0f / (float)S.l.blen;
  st.rcnt1 = 1.0f / (float)st.cnt1;
  return st;
}
// floor(t / d) and the remainder for t < 2^23: the float-reciprocal quotient
// is off by at most two, which the remainder corrects
MX_XHD inline uint32_t xv_divmod(uint32_t t, uint32_t d, float rd, uint32_t *rem) {
  uint32_t q = (uint32_t)((float)t * rd);
  int32_t r = (int32_t)(t - q * d);
  if (r < 0) { q--; r += (int32_t)d; }
  if (r < 0) { q--; r += (int32_t)d; }
  if (r >= (int32_t)d) { q++; r -= (int32_t)d; }
  if (r >= (int32_t)d) { q++; r -= (int32_t)d; }
  *rem = (uint32_t)r;
  return q;
}
// offset from `user` of the byte `rel` bytes into the stretch
MX_XHD inline int64_t xv_off(const XSide &S, const XVStart &st, uint32_t rel) {
  uint32_t r;
  const uint32_t q = xv_divmod(st.o0 + rel, (uint32_t)S.l.blen, st.rblen, &r);   // blocks past the first
  if (q < st.room) return st.baseL + (int64_t)q * S.l.stride1 + (int64_t)r;
  const uint32_t e = q - st.room;   // blocks past the end of the first instance: fewer than 2^14
  uint32_t d = 0, l = e;
  if (e >= st.cnt1) d = xv_divmod(e, st.cnt1, st.rcnt1, &l);
  return st.base0 + (int64_t)(d + 1) * S.l.ext + (int64_t)l * S.l.stride1 + (int64_t)r;
}

// Fills the magics and W of a job.  MX_ERR_UNSUPPORTED: W would be below 4;
// MX_ERR_ARG: a stream position or length past 2^kMagicBits.
int xvjob_make(const char *src, const XLay &sl, uint64_t pos_s, char *dst, const XLay &dl, uint64_t pos_d,
               uint64_t bytes, XVJob *out);

struct XVPlan {
  std::vector<XVJob> jobs;     // non-empty jobs, ascending block count
  std::vector<XSeg> seg;       // jobs.size() + 1 entries (xplan_lookup)
  std::vector<XLaunch> launch;
  uint64_t nblocks = 0;
  size_t bytes = 0;
};
// The round-robin block -> job tables of mx_exchange_plan.hpp over blocks cut
// in the STREAM: block k of a job is its stream bytes [k, k + 1) * xv_block_bytes(W).
int xvplan_build(const XVJob *jobs, size_t n, XVPlan &out, uint64_t max_grid_blocks = kXMaxGridBlocks);

}  // namespace mx
