// mx_ddt_layout.hip -- host-only layout planning of the datatype engine
// (mx_ddt_layout.hpp): flattening a committed description into strided runs,
// the byte map and its PACK tiles, the piece tables and the block table.
// Every bound the convertor's kernels trust is computed here.  No HIP API, no
// launch, no environment.
#include <string.h>
#include <algorithm>
#include <climits>

#include "mx_ddt_layout.hpp"

namespace mx {

namespace {

// dt_elem_desc record views (opal_datatype_internal.h:146-196)
struct RecElem { uint16_t flags, type; uint32_t count; uint64_t blocklen; int64_t extent; int64_t disp; };
struct RecLoop { uint16_t flags, type; uint32_t items; uint32_t loops; uint32_t pad; uint64_t unused; int64_t extent; };
static_assert(sizeof(RecElem) == 32 && sizeof(RecLoop) == 32, "dt_elem_desc is 32 bytes");

constexpr uint16_t T_LOOP = 0, T_END_LOOP = 1, T_LB = 2, T_UB = 3;
constexpr uint16_t F_DATA = 0x0100;

const uint64_t kBasicLP64[MX_OPAL_NBASIC] = {
    0, 0, 0, 0,            // LOOP END_LOOP LB UB
    1, 2, 4, 8, 16,        // INT1 INT2 INT4 INT8 INT16
    1, 2, 4, 8, 16,        // UINT1 .. UINT16
    2, 4, 8, 16, 16,       // FLOAT2 FLOAT4 FLOAT8 FLOAT12 (long double: 16 B) FLOAT16
    4, 8, 16, 32,          // SHORT_FLOAT_COMPLEX FLOAT_COMPLEX DOUBLE_COMPLEX LONG_DOUBLE_COMPLEX
    1, 4, 0                // BOOL WCHAR UNAVAILABLE
};

bool contiguous_single(const DRun &r) { return r.cnt1 == 1 && r.cnt2 == 1; }

void push_run(std::vector<DRun> &out, DRun r) {
  if (r.bytes == 0) return;
  // a 1-level run whose blocks touch is one contiguous block
  if (r.cnt2 == 1 && r.cnt1 > 1 && r.stride1 == (int64_t)r.blen) { r.blen *= r.cnt1; r.cnt1 = 1; r.stride1 = 0; }
  if (!out.empty()) {
    DRun &p = out.back();
    if (contiguous_single(p) && contiguous_single(r) && p.disp + (int64_t)p.blen == r.disp) {
      p.blen += r.blen;
      p.bytes += r.bytes;
      return;
    }
  }
  out.push_back(r);
}

int flatten(const uint8_t *recs, size_t lo, size_t hi, int64_t base, const uint64_t *bs, std::vector<DRun> &out) {
  size_t i = lo;
  while (i < hi) {
    RecElem e;
    memcpy(&e, recs + 32 * i, 32);
    if (e.type == T_END_LOOP) return MX_SUCCESS;   // terminator of this level
    if (e.type == T_LOOP) {
      RecLoop L;
      memcpy(&L, recs + 32 * i, 32);
      if (L.items == 0 || i + L.items >= hi + 1) return MX_ERR_ARG;
      std::vector<DRun> body;
      int rc = flatten(recs, i + 1, i + L.items, 0, bs, body);
      if (rc) return rc;
      if (body.size() == 1 && body[0].cnt2 == 1) {
        DRun r = body[0];
        r.disp += base;
        if (contiguous_single(r)) {          // loop of one contiguous block
          r.cnt1 = L.loops;
          r.stride1 = L.extent;
        } else {
          r.cnt2 = L.loops;
          r.stride2 = L.extent;
        }
        r.bytes = r.blen * r.cnt1 * r.cnt2;
        push_run(out, r);
      } else {
        if (out.size() + body.size() * (size_t)L.loops > kMaxRuns) return MX_ERR_UNSUPPORTED;
        for (uint32_t l = 0; l < L.loops; l++)
          for (DRun r : body) {
            r.disp += base + (int64_t)l * L.extent;
            push_run(out, r);
          }
      }
      i += L.items + 1;
      continue;
    }
    if (e.type == T_LB || e.type == T_UB || !(e.flags & F_DATA)) { i++; continue; }
    if (e.type >= MX_OPAL_NBASIC || bs[e.type] == 0) return MX_ERR_ARG;
    DRun r;
    r.disp = base + e.disp;
    r.blen = e.blocklen * bs[e.type];
    r.cnt1 = e.count;
    r.stride1 = e.extent;
    r.cnt2 = 1;
    r.stride2 = 0;
    r.bytes = r.blen * r.cnt1;
    push_run(out, r);
    if (out.size() > kMaxRuns) return MX_ERR_UNSUPPORTED;
    i++;
  }
  return MX_SUCCESS;
}

// Every byte of the stream lies at a higher user address than the one
// before it (runs, blocks and instances in address order, no overlap):
// then a tile's bytes all lie in [addr(first), addr(last)].
bool is_monotonic(const std::vector<DRun> &runs, int64_t ext) {
  if (runs.empty()) return false;
  int64_t prev_end = INT64_MIN;   // one past the last byte so far
  for (const DRun &r : runs) {
    if (r.cnt1 > 1 && r.stride1 < (int64_t)r.blen) return false;
    const int64_t inner = (int64_t)(r.cnt1 - 1) * r.stride1 + (int64_t)r.blen;
    if (r.cnt2 > 1 && r.stride2 < inner) return false;
    if (r.disp < prev_end) return false;
    prev_end = r.disp + (int64_t)(r.cnt2 - 1) * r.stride2 + inner;
  }
  return prev_end <= ext + runs[0].disp;   // next instance starts after
}

uint64_t absg(int64_t v) { return v < 0 ? (uint64_t)(-v) : (uint64_t)v; }

// Pieces of one instance for a user origin at address `al` mod 16: maximal
// contiguous user runs in stream order, cut into naturally aligned
// 1/2/4/8/16-byte pieces (aligned for every instance: the width also
// divides the extent).
void cut_pieces(const DdtLayout *d, int al, std::vector<DPiece> &v) {
  const uint64_t A = gcd64(16, absg(d->ub - d->lb));
  const size_t S = d->bmap.size();
  for (size_t b = 0; b < S;) {
    size_t L = 1;
    while (b + L < S && d->bmap[b + L] == d->bmap[b] + (int32_t)L) L++;
    for (size_t pos = 0; pos < L;) {
      const int64_t x = (int64_t)d->bmap[b] + (int64_t)pos;
      const uint64_t addr = (uint64_t)(((al + x) % 16 + 16) % 16);
      uint64_t w = 16;
      while (w > 1 && (addr % w || w > L - pos || A % w)) w >>= 1;
      DPiece pc;
      pc.uoff = (int32_t)x;
      pc.soff = (uint16_t)(b + pos);
      pc.lg = (uint8_t)__builtin_ctzll(w);
      pc.pad = 0;
      v.push_back(pc);
      pos += w;
    }
    b += L;
  }
}

// Byte map of one instance: bmap[b] = user offset of packed byte b.  Also
// fixes the PACK tile: the largest multiple of 256 stream bytes (<= 16 KiB)
// whose user span, rounded out to 16 bytes, always fits kBmapSpan -- whole
// instances for a non-monotonic layout, [addr(first), addr(last)] for a
// monotonic one.
// inst_tiles false (MX_CONV_BMAP_INST=0): the byte-map PACK's tiles of
// non-monotonic layouts stay multiples of 256 stream bytes instead of whole
// instances (A/B switch; read at datatype creation)
void build_bmap(DdtLayout *d, bool inst_tiles) {
  const int64_t ext = d->ub - d->lb;
  const uint64_t S = d->size;
  if (S == 0 || S > kBmapMaxS || ext <= 0) return;
  std::vector<int32_t> m;
  m.reserve(S);
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  for (const DRun &r : d->runs)
    for (uint64_t l2 = 0; l2 < r.cnt2; l2++)
      for (uint64_t l1 = 0; l1 < r.cnt1; l1++)
        for (uint64_t o = 0; o < r.blen; o++) {
          const int64_t u = r.disp + (int64_t)l2 * r.stride2 + (int64_t)l1 * r.stride1 + (int64_t)o;
          if (u < INT32_MIN || u > INT32_MAX) return;
          m.push_back((int32_t)u);
          lo = std::min(lo, u);
          hi = std::max(hi, u + 1);
        }
  if (m.size() != S) return;
  d->bmap.swap(m);
  d->umin = lo;
  d->uspan = hi - lo;
  // 16-bit map entries when every entry of the kernel's wrapped table
  // (bmap + ext for the three bytes past an instance) fits
  d->map16 = d->uspan + (int64_t)((S + 2) / S) * ext <= 65536;
  // PACK kernel choice: pieces of >= 8 bytes on average that all land on
  // whole packed words move with few wide accesses through the piece kernel;
  // narrow or misaligned pieces go through the byte map, whose cost per
  // byte is flat.  Measured at 1 GiB (profiles/r02/convertor_r2.txt): lower
  // triangle (8-byte pieces) piece 3.58 vs byte map 2.28 TB/s; indexed /
  // BLACS (4-byte) 2.66 / 2.85 vs 3.40 / 3.05; struct (misaligned) 2.46 vs
  // 3.41; 8-byte struct types equal within 2 %.
  {
    std::vector<DPiece> v;
    cut_pieces(d, 0, v);
    bool words = true;
    for (const DPiece &p : v) words = words && p.lg >= 2 && (p.soff & 3) == 0;
    d->piece_pack = words && !v.empty() && S >= 8 * v.size();
  }
  // The byte map is staged only for dense layouts (<= 4 user bytes per
  // packed byte; a sparse one reads mostly gaps -- ref_matrix_borders at 23:
  // 0.83 -> 0.42 TB/s) and maps small enough for >= 3 workgroups per CU
  // (ref_upper_matrix_60's 29 KiB map: 1.32 -> 1.25 TB/s)
  if ((S + 3) * (d->map16 ? 2 : 4) > kBmapLds || ext > 4 * (int64_t)S || d->uspan > 4 * (int64_t)S) return;
  d->bmap_quad = S % 4 != 0 && 4 * S * (d->map16 ? 2 : 4) <= kBmapLds;
  {                                // packed dwords whose 4 bytes are user-contiguous, by instance phase
    auto Ux = [&](uint64_t x) { return (int64_t)(x / S) * ext + d->bmap[x % S]; };
    uint64_t c = 0;
    for (uint64_t b = 0; b < S; b++) c += Ux(b + 3) == Ux(b) + 3 && Ux(b + 1) == Ux(b) + 1 && Ux(b + 2) == Ux(b) + 2;
    d->bmap_cw = c * 10 >= 9 * S;
    uint64_t cwd = 0;                // at the phases a dword of a 16-aligned tile starts at
    for (uint64_t b = 0; b < S; b += 4)
      cwd += Ux(b + 3) == Ux(b) + 3 && Ux(b + 1) == Ux(b) + 1 && Ux(b + 2) == Ux(b) + 2;
    d->bmap_word = S % 4 == 0 && cwd == S / 4;
  }
  // user bytes a tile of T stream bytes starting at instance byte b touches
  auto U = [&](uint64_t x) { return (int64_t)(x / S) * ext + d->bmap[x % S]; };
  auto worst = [&](uint64_t T) {
    if (!d->monotonic) return (int64_t)(((T - 1) / S + 1) * (uint64_t)ext) + d->uspan;
    int64_t w = 0;
    for (uint64_t b = 0; b < S; b++) w = std::max<int64_t>(w, U(b + T - 1) - U(b) + 1);
    return w;
  };
  // the largest T (a multiple of 256, at most 2/3 of the span) whose worst
  // user span + kBmapSlack fits: the span staged from a line start plus its
  // 16-byte rounding up.  worst() grows with T.
  for (int k = 0; k < 3; k++) {
    const int64_t span = kBmapSpans[k];
    uint64_t lo = 0, hi = (uint64_t)span * 2 / 3 / 256;      // in units of 256
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) / 2;
      if (worst(mid * 256) + kBmapSlack <= span) lo = mid;
      else hi = mid - 1;
    }
    d->bmap_Ts[k] = lo * 256;
    // a layout that is not monotonic stages whole instances per tile; when
    // S % 16 == 0 a tile of exactly k instances starts (from offset 0) on an
    // instance boundary and stages k of them, not the k + 1 a tile cut
    // mid-instance does (indexed: 12.9 instead of 19.3 KiB per 10 KiB of stream)
    if (!d->monotonic && S % 16 == 0) {
      const int64_t kk = (span - kBmapSlack - d->uspan) / ext;   // worst(kk * S) + kBmapSlack <= span
      if (kk >= 1 && (uint64_t)kk * S >= 256 && (uint64_t)kk * S <= (uint64_t)span * 2 / 3 &&
          worst((uint64_t)kk * S) + kBmapSlack <= span && inst_tiles)
        d->bmap_Ts[k] = (uint64_t)kk * S;
    }
  }
  d->bmap_T = d->bmap_Ts[1];
}

}  // namespace

int ddt_layout_create(const void *desc, size_t nrec, const uint64_t *basic_sizes, size_t size, int64_t lb, int64_t ub,
                      bool inst_tiles, DdtLayout &L) {
  DdtLayout *d = &L;
  const uint64_t *bs = basic_sizes ? basic_sizes : kBasicLP64;
  int rc = flatten((const uint8_t *)desc, 0, nrec, 0, bs, d->runs);
  if (rc) return rc;
  uint64_t poff = 0, g = 16;
  for (DRun &r : d->runs) {
    r.poff = poff;
    poff += r.bytes;
    g = gcd64(g, absg(r.disp));
    g = gcd64(g, r.blen);
    if (r.cnt1 > 1) g = gcd64(g, absg(r.stride1));
    if (r.cnt2 > 1) g = gcd64(g, absg(r.stride2));
  }
  if (poff != size) return MX_ERR_ARG;   // description / size mismatch
  for (DRun &r : d->runs) {
    r.mblen = make_magic(r.blen);
    r.mcnt1 = make_magic(r.cnt1);
  }
  d->size = size;
  d->lb = lb;
  d->ub = ub;
  d->gcd_all = gcd64(g, absg(ub - lb));
  d->mS = make_magic(size ? size : 1);
  d->monotonic = is_monotonic(d->runs, ub - lb);
  build_bmap(d, inst_tiles);
  return MX_SUCCESS;
}

// The piece table for a user origin at address `al` mod 16 (cut_pieces) with
// its tile size.
bool plan_pieces(const DdtLayout &L, int al, std::vector<DPiece> &pieces, uint32_t &Kout) {
  const DdtLayout *d = &L;
  const size_t S = d->bmap.size();
  std::vector<DPiece> v;
  cut_pieces(d, al, v);
  const uint32_t npi = (uint32_t)v.size();
  // pieces per tile: ~8 KiB of stream, staged bytes (+ alignment slop) <= kPieceStage
  auto window = [&](uint32_t K) {
    uint64_t mx = 0;
    for (uint32_t j = 0; j < npi; j++) {
      const uint64_t e = (uint64_t)j + K - 1;
      const DPiece &pe = v[e % npi];
      const uint64_t end = (e / npi) * S + pe.soff + (1u << pe.lg);
      mx = std::max<uint64_t>(mx, end - v[j].soff);
    }
    return mx;
  };
  uint64_t K = std::max<uint64_t>(kCB, std::min<uint64_t>(4096, (8192ull * npi / S) / kCB * kCB));
  while (K > kCB && window((uint32_t)K) + 32 > (uint64_t)kPieceStage) K -= kCB;
  if (window((uint32_t)K) + 32 > (uint64_t)kPieceStage) return false;
  pieces.swap(v);
  Kout = (uint32_t)K;
  return true;
}

// The block table of k_convert_blk: the instance's contiguous user blocks in
// stream order (touching blocks merged), tfirst[k] = the block holding
// instance stream byte k * kBlkG (one entry past the last stretch, so
// [tfirst[k], tfirst[k + 1]] always brackets the search), and the tile T: the
// largest of tmax (16 KiB) .. 512 B of packed memory whose stream stretch
// never overlaps more than kBlkCap blocks (a T-byte stretch overlaps at most
// the blocks from b to the one holding end(b) - 2 + T, over every block b,
// across instance boundaries).
bool plan_blocks(const DdtLayout &L, uint64_t tmax, bool span_pack, BlkPlan &P) {
  const DdtLayout *d = &L;
  const uint64_t S = d->size;
  const int64_t ext = d->ub - d->lb;
  constexpr uint64_t kMaxBlocks = (uint64_t)1 << 22;
  if (S == 0 || S >= ((uint64_t)1 << 31) || ext <= 0) return false;
  std::vector<HBlk> v;
  uint64_t soff = 0;
  for (const DRun &r : d->runs) {
    if (v.size() + r.cnt1 * r.cnt2 > kMaxBlocks + 1) return false;
    for (uint64_t l2 = 0; l2 < r.cnt2; l2++)
      for (uint64_t l1 = 0; l1 < r.cnt1; l1++) {
        const int64_t u = r.disp + (int64_t)l2 * r.stride2 + (int64_t)l1 * r.stride1;
        if (!v.empty() && v.back().uoff + (int64_t)v.back().len == u && v.back().len + r.blen < ((uint64_t)1 << 31)) {
          v.back().len += (uint32_t)r.blen;
        } else {
          HBlk b;
          b.uoff = u;
          b.soff = (uint32_t)soff;
          b.len = (uint32_t)r.blen;
          v.push_back(b);
        }
        soff += r.blen;
      }
  }
  if (v.empty() || v.size() > kMaxBlocks || soff != S) return false;
  const uint64_t nb = v.size();
  auto max_overlap = [&](uint64_t T) {
    uint64_t mx = 0, j = 0;
    for (uint64_t b = 0; b < nb; b++) {
      const uint64_t last = (uint64_t)v[b].soff + v[b].len - 1 + T - 1;   // end(b) - 2 + T
      if (j < b) j = b;
      // advance j to the block holding `last` (monotonic in b)
      while (true) {
        const uint64_t jn = j + 1, i = jn / nb;
        const uint64_t start = i * S + v[jn - i * nb].soff;
        if (start > last) break;
        j = jn;
      }
      mx = std::max<uint64_t>(mx, j - b + 1);
    }
    return mx;
  };
  uint64_t T = tmax;
  while (T > 512 && max_overlap(T) > kBlkCap) T /= 2;
  if (max_overlap(T) > kBlkCap) return false;
  // span PACK (k_pack_blk_span): monotonic blocks; the user span of a
  // T-byte stretch that starts in block b and ends in block j is
  // T + G(j) - G(b), G = user offset - stream offset (non-decreasing), so
  // its maximum over stretches starting in b is at the last j reachable
  bool mono = true;
  for (uint64_t b = 0; b + 1 < nb && mono; b++) mono = v[b].uoff + (int64_t)v[b].len <= v[b + 1].uoff;
  mono = mono && v[nb - 1].uoff + (int64_t)v[nb - 1].len <= v[0].uoff + ext;
  uint64_t Ts = 0, caps = 0;
  if (mono && span_pack) {
    auto G = [&](uint64_t j) {
      const uint64_t i = j / nb;
      return ((int64_t)i * ext + v[j - i * nb].uoff) - (int64_t)(i * S + v[j - i * nb].soff);
    };
    auto max_span = [&](uint64_t TT) {
      int64_t mx = 0;
      uint64_t j = 0;
      for (uint64_t b = 0; b < nb; b++) {
        const uint64_t last = (uint64_t)v[b].soff + v[b].len - 1 + TT - 1;
        if (j < b) j = b;
        while (true) {
          const uint64_t jn = j + 1, i = jn / nb;
          if (i * S + v[jn - i * nb].soff > last) break;
          j = jn;
        }
        mx = std::max<int64_t>(mx, G(j) - G(b));
      }
      return (int64_t)TT + mx;
    };
    for (uint64_t TT = 16384; TT >= 2048; TT /= 2) {
      if (max_overlap(TT) <= kBlkCap && max_span(TT) + 32 <= (int64_t)kBlkSpan) {
        Ts = TT;
        caps = max_overlap(TT) + 1;
        break;
      }
    }
  }
  const uint64_t nk = (S + kBlkG - 1) / kBlkG;
  std::vector<uint32_t> tf(nk + 1);
  for (uint64_t k = 0, b = 0; k < nk; k++) {
    while (b + 1 < nb && v[b + 1].soff <= k * kBlkG) b++;
    tf[k] = (uint32_t)b;
  }
  tf[nk] = (uint32_t)(nb - 1);
  std::vector<DBlk> dv(nb + 1);
  for (uint64_t b = 0; b < nb; b++) {
    if (v[b].uoff < INT32_MIN || v[b].uoff > INT32_MAX) return false;   // instance offsets beyond +-2 GiB
    dv[b].uoff = (int32_t)v[b].uoff;
    dv[b].soff = v[b].soff;
  }
  dv[nb].uoff = 0;
  dv[nb].soff = (uint32_t)S;
  P.blocks.swap(v);
  P.dev.swap(dv);
  P.tfirst.swap(tf);
  P.T = T;
  P.Tspan = Ts;
  P.capspan = (uint32_t)caps;
  return true;
}

void ddt_span(const DdtLayout &L, size_t count, int64_t *lo, int64_t *hi) {
  const DdtLayout *d = &L;
  *lo = *hi = 0;
  if (!count || d->runs.empty()) return;
  int64_t a = INT64_MAX, b = INT64_MIN;
  for (const DRun &r : d->runs) {
    if (!r.bytes) continue;
    const int64_t s1 = (int64_t)(r.cnt1 - 1) * r.stride1, s2 = (int64_t)(r.cnt2 - 1) * r.stride2;
    const int64_t first = r.disp + std::min<int64_t>(0, s1) + std::min<int64_t>(0, s2);
    const int64_t last = r.disp + std::max<int64_t>(0, s1) + std::max<int64_t>(0, s2) + (int64_t)r.blen;
    a = std::min(a, first);
    b = std::max(b, last);
  }
  if (a > b) return;
  const int64_t ext = d->ub - d->lb, tail = (int64_t)(count - 1) * ext;
  *lo = a + std::min<int64_t>(0, tail);
  *hi = b + std::max<int64_t>(0, tail);
}

}  // namespace mx
