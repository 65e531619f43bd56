// mx_ddt_layout.hpp -- host-only layout planning of the datatype engine
// (mx_ddt_layout.hip): a committed description becomes the run table, the
// byte map and, on demand, the piece and block tables the convertor's kernels
// (mx_convertor.hip) read, with every tile size they trust.  No HIP API, no
// launch, no environment: it compiles with a host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "../../include/mx_kernels.h"
#include "../../include/mx_convertor.h"

namespace mx {

// ---------------------------------------------------------------------------
// table elements the kernels read, and the limits the planners test against
// ---------------------------------------------------------------------------
// Division by a run-time constant without a 64-bit divide: for numerators
// n < 2^48, floor(n / d) = floor(n * m / 2^k) with k = 48 + ceil(log2 d),
// m = ceil(2^k / d) (Granlund & Montgomery, PLDI'94, thm 4.2).
struct Magic { uint64_t m; uint32_t k; uint32_t pad; };
constexpr int kMagicBits = 48;

struct DRun {
  int64_t disp;
  uint64_t blen;     // bytes per block
  uint64_t cnt1;     // inner block count
  int64_t stride1;
  uint64_t cnt2;     // outer repetition count
  int64_t stride2;
  uint64_t poff;     // packed offset of the run within one instance
  uint64_t bytes;    // blen * cnt1 * cnt2
  Magic mblen, mcnt1;
};

constexpr int kCB = 256;
constexpr size_t kMaxRuns = (size_t)1 << 22;
// VEC kernels (k_convert_vec, k_exchange_vec): keeps t / blen exact in fp32 + 1 correction
constexpr uint64_t kVecMaxBlen = (uint64_t)1 << 22;

constexpr uint32_t kBmapMaxS = 65535;      // packed bytes per instance (piece soff is 16-bit)
constexpr size_t kBmapLds = 20480;         // PACK: map bytes staged in LDS
constexpr int kBmapSpan = 24576;           // PACK: user span staged per tile
constexpr int kBmapSpans[3] = {12288, kBmapSpan, 49152};   // MX_CONV_BMAP_SPAN choices
// PACK: a tile's staged span starts at the 128-byte line holding its first
// user byte (a wave's 1 KiB loads then cover whole lines) and ends on the
// 16-byte granule after its last one, so a tile of w user bytes stages less
// than w + kBmapAlign + 16 bytes; the planner leaves one more granule to spare
constexpr int kBmapAlign = 128;
constexpr int kBmapSlack = kBmapAlign + 32;
constexpr int kPieceStage = 16384;        // UNPACK: packed bytes staged per tile

struct DPiece {
  int32_t uoff;       // user offset from the instance origin
  uint16_t soff;      // stream offset within the instance
  uint8_t lg;         // width = 1 << lg bytes (user address aligned to it)
  uint8_t pad;
};

constexpr uint32_t kBlkCap = 1024;         // staged blocks per tile (16 KiB of LDS)
constexpr uint32_t kBlkG = 256;            // tfirst granularity (instance stream bytes)
constexpr uint32_t kBlkMaxT = 65536;       // largest tile (packed-memory bytes)
constexpr uint32_t kBlkSpan = 24576;       // PACK, span-staged: user span staged per tile

// device block table entry (8 B): user offset from the instance origin and
// stream offset; a block's length is the next entry's soff minus its own
// (the table carries one sentinel entry with soff = the instance size)
struct DBlk { int32_t uoff; uint32_t soff; };
struct HBlk { int64_t uoff; uint32_t soff; uint32_t len; };   // host side of the block table (plan_blocks)

inline Magic make_magic(uint64_t d) {
  Magic M;
  int l = 0;
  while (l < 64 && (((unsigned __int128)1) << l) < d) l++;
  M.k = (uint32_t)(kMagicBits + l);
  const unsigned __int128 two_k = ((unsigned __int128)1) << M.k;
  M.m = (uint64_t)((two_k + d - 1) / d);
  M.pad = 0;
  return M;
}

inline uint64_t gcd64(uint64_t a, uint64_t b) {
  while (b) { uint64_t t = a % b; a = b; b = t; }
  return a;
}

// ---------------------------------------------------------------------------
// the layout of one committed datatype
// ---------------------------------------------------------------------------
struct DdtLayout {
  std::vector<DRun> runs;
  size_t size = 0;
  int64_t lb = 0, ub = 0;
  uint64_t gcd_all = 0;  // gcd of every disp/stride/blen/extent (access unit)
  Magic mS = {0, 0, 0};  // divide by size
  bool monotonic = false;   // user addresses strictly increase along the stream
  // byte map of one instance (size <= kBmapMaxS): bmap[b] = user offset of
  // packed byte b.  PACK kernel k_pack_bmap stages (bmap - umin) as 16-bit
  // (user span < 64 KiB) or 32-bit words when they fit kBmapLds.
  std::vector<int32_t> bmap;
  int map16 = 0;
  int64_t umin = 0, uspan = 0;
  uint64_t bmap_T = 0;             // stream bytes per PACK tile (0: no PACK kernel)
  uint64_t bmap_Ts[3] = {0, 0, 0}; // the same for staged spans kBmapSpans[0..2] (bmap_T = [1])
  bool bmap_quad = false;          // the PACK kernel stages the map as quads (BmapArgs::qsh)
  bool bmap_cw = false;            // >= 90 % of packed dwords are 4 user-contiguous bytes (BmapArgs::cw)
  bool bmap_word = false;          // every dword at a phase 4k is (BmapArgs::word)
  bool piece_pack = false;         // PACK takes the piece kernel (wide word-aligned pieces, build_bmap)
};

// Flattens the description (nrec 32-byte records; basic_sizes as
// mx_ddt_create takes them) into L: runs with their packed offsets and
// magics, the access unit, monotonic, and the byte map with its tiles.
// inst_tiles: byte-map tiles of whole instances for non-monotonic layouts
// (MX_CONV_BMAP_INST).  MX_SUCCESS or an MX_ERR_* code.
int ddt_layout_create(const void *desc, size_t nrec, const uint64_t *basic_sizes, size_t size, int64_t lb, int64_t ub,
                      bool inst_tiles, DdtLayout &L);

// The piece table for a user origin at address `al` mod 16 and its tile of K
// pieces; false: not applicable.  Needs the byte map.
bool plan_pieces(const DdtLayout &L, int al, std::vector<DPiece> &pieces, uint32_t &K);

// index of the piece holding packed byte b of an instance
inline uint32_t piece_of(const std::vector<DPiece> &v, uint64_t b) {
  uint32_t lo = 0, hi = (uint32_t)v.size() - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) / 2;
    if (v[mid].soff <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct BlkPlan {
  std::vector<HBlk> blocks;        // the blocks (the device table adds the sentinel)
  std::vector<DBlk> dev;           // the device table image, sentinel included
  std::vector<uint32_t> tfirst;
  uint64_t T = 0;                  // packed-memory bytes per tile
  uint64_t Tspan = 0;              // PACK through k_pack_blk_span: its tile (0: not applicable)
  uint32_t capspan = 0;            // most blocks one of its tiles overlaps
};

// The block table; false: not applicable.  tmax: the largest tile tried
// (MX_CONV_BLK_T), span_pack: plan the span PACK's tile (MX_CONV_BLK_SPAN).
bool plan_blocks(const DdtLayout &L, uint64_t tmax, bool span_pack, BlkPlan &P);

// Byte range [*lo, *hi) relative to the user pointer that `count` instances
// touch (the true extent; instance i is displaced by i * extent).
void ddt_span(const DdtLayout &L, size_t count, int64_t *lo, int64_t *hi);

}  // namespace mx
