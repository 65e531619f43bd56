// ddt_layout_check.cpp -- host check of the datatype layout planner
// (csrc/mx_ddt_layout.hip): every table and tile size the convertor's kernels
// trust, checked against an independent index map m of one instance
// (m[b] = user offset of packed byte b) that the test hands over with each
// description (tests/test_ddt_layout_host.py).  Built with the host compiler
// under sanitizers; exits non-zero on the first violated invariant, naming
// the case and the invariant.
//
// case file: "MXLAYC01", u32 ncases, then per case
//   char name[64]; u32 nrec; u32 pad; i64 size, lb, ub, true_lb, true_ub;
//   u64 basic[MX_OPAL_NBASIC]; u8 desc[32 * nrec]; i64 map[size]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "mx_ddt_layout.hpp"

using namespace mx;

static const char *g_case = "?";
#define CHECK(cond, ...)                                                        \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "FAIL case %s: %s (%s:%d): ", g_case, #cond, __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                             \
      fprintf(stderr, "\n");                                                    \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

// the kernels' udiv (mx_convertor.hip), restated
static uint64_t udiv(uint64_t n, const Magic &M) { return (uint64_t)(((unsigned __int128)n * M.m) >> M.k); }

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

struct Case {
  char name[65];
  uint32_t nrec, pad;
  int64_t size, lb, ub, true_lb, true_ub;
  uint64_t basic[MX_OPAL_NBASIC];
  std::vector<uint8_t> desc;
  std::vector<int64_t> m;
};

static void rd(FILE *f, void *p, size_t n) {
  if (n && fread(p, 1, n, f) != n) {
    fprintf(stderr, "FAIL: short case file\n");
    exit(2);
  }
}

static void check_magic(uint64_t d, const Magic &M, const char *what) {
  const Magic F = make_magic(d);
  CHECK(F.m == M.m && F.k == M.k, "%s: stored magic differs from make_magic(%llu)", what, (unsigned long long)d);
  const uint64_t top = ((uint64_t)1 << kMagicBits) - 1;
  uint64_t ns[] = {0, d - 1, d, top, rnd() & top, rnd() & top, rnd() % (4 * d + 1), rnd() % (d * 1000 + 1) & top};
  for (uint64_t n : ns) CHECK(udiv(n, M) == n / d, "%s: udiv(%llu, %llu)", what, (unsigned long long)n, (unsigned long long)d);
}

// user offset of stream byte x of the message (instance x / S displaced by ext)
static int64_t U(const Case &c, uint64_t x) {
  const uint64_t S = (uint64_t)c.size;
  return (int64_t)(x / S) * (c.ub - c.lb) + c.m[x % S];
}

static void check_runs(const Case &c, const DdtLayout &L) {
  const uint64_t S = (uint64_t)c.size;
  CHECK(L.size == S && L.lb == c.lb && L.ub == c.ub, "size / lb / ub");
  uint64_t b = 0, poff = 0;
  for (const DRun &r : L.runs) {
    CHECK(r.poff == poff, "poff is not the running sum at run %zu", (size_t)(&r - L.runs.data()));
    CHECK(r.bytes == r.blen * r.cnt1 * r.cnt2 && r.bytes > 0, "run bytes");
    poff += r.bytes;
    for (uint64_t l2 = 0; l2 < r.cnt2; l2++)
      for (uint64_t l1 = 0; l1 < r.cnt1; l1++)
        for (uint64_t o = 0; o < r.blen; o++, b++) {
          CHECK(b < S, "the runs hold more than size bytes");
          const int64_t u = r.disp + (int64_t)l2 * r.stride2 + (int64_t)l1 * r.stride1 + (int64_t)o;
          CHECK(u == c.m[b], "run walk: stream byte %llu at %lld, map says %lld", (unsigned long long)b, (long long)u,
                (long long)c.m[b]);
        }
    check_magic(r.blen, r.mblen, "blen");
    check_magic(r.cnt1, r.mcnt1, "cnt1");
  }
  CHECK(b == S && poff == S, "the runs hold %llu of %llu bytes", (unsigned long long)b, (unsigned long long)S);
  check_magic(S, L.mS, "size");
  if (L.monotonic)
    for (uint64_t x = 0; x + 1 < 2 * S; x++)
      CHECK(U(c, x) < U(c, x + 1), "monotonic set, but stream byte %llu does not lie below the next", (unsigned long long)x);
}

static void check_bmap(const Case &c, const DdtLayout &L) {
  const uint64_t S = (uint64_t)c.size;
  const int64_t ext = c.ub - c.lb;
  if (L.bmap.empty()) {
    CHECK(!L.bmap_T && !L.bmap_Ts[0] && !L.bmap_Ts[1] && !L.bmap_Ts[2] && !L.piece_pack, "tiles without a byte map");
    return;
  }
  CHECK(L.bmap.size() == S && S <= kBmapMaxS && ext > 0, "byte map of %zu entries", L.bmap.size());
  int64_t lo = c.m[0], hi = c.m[0];
  for (uint64_t b = 0; b < S; b++) {
    CHECK(L.bmap[b] == c.m[b], "bmap[%llu]", (unsigned long long)b);
    lo = std::min(lo, c.m[b]);
    hi = std::max(hi, c.m[b]);
  }
  CHECK(L.umin == lo && L.uspan == hi - lo + 1, "umin / uspan");
  CHECK(lo == c.true_lb && hi + 1 == c.true_ub, "the case's own true bounds");
  if (L.map16)   // the kernel's wrapped table: the map and, displaced by ext, its first three entries again
    for (uint64_t x = 0; x < S + 3; x++) CHECK(U(c, x) - lo >= 0 && U(c, x) - lo < 65536, "map16: entry %llu", (unsigned long long)x);
  // the byte-map PACK: staged only for dense layouts whose map fits kBmapLds
  const bool staged = !((S + 3) * (L.map16 ? 2 : 4) > kBmapLds || ext > 4 * (int64_t)S || L.uspan > 4 * (int64_t)S);
  if (!staged) {
    CHECK(!L.bmap_T && !L.bmap_Ts[0] && !L.bmap_Ts[1] && !L.bmap_Ts[2], "tiles of a map that is not staged");
    CHECK(!L.bmap_quad && !L.bmap_cw && !L.bmap_word, "shapes of a map that is not staged");
    return;
  }
  CHECK(L.bmap_T == L.bmap_Ts[1], "bmap_T");
  for (int k = 0; k < 3; k++) {
    const uint64_t T = L.bmap_Ts[k];
    if (!T) continue;
    CHECK(T % 16 == 0, "bmap_Ts[%d] = %llu is no multiple of 16", k, (unsigned long long)T);
    for (uint64_t b = 0; b < S; b++) {
      int64_t span;
      if (L.monotonic) span = U(c, b + T - 1) - U(c, b) + 1;
      else span = (int64_t)((b + T - 1) / S) * ext + L.uspan;   // the whole instances 0 .. (b + T - 1) / S
      CHECK(span + 160 <= kBmapSpans[k], "bmap_Ts[%d] = %llu: a tile at phase %llu spans %lld user bytes", k,
            (unsigned long long)T, (unsigned long long)b, (long long)span);
    }
  }
  auto cont4 = [&](uint64_t b) { return U(c, b + 1) == U(c, b) + 1 && U(c, b + 2) == U(c, b) + 2 && U(c, b + 3) == U(c, b) + 3; };
  uint64_t cw = 0, cwd = 0;
  for (uint64_t b = 0; b < S; b++) cw += cont4(b);
  for (uint64_t b = 0; b < S; b += 4) cwd += cont4(b);
  CHECK(L.bmap_cw == (cw * 10 >= 9 * S), "bmap_cw: %llu of %llu dwords are contiguous", (unsigned long long)cw, (unsigned long long)S);
  CHECK(L.bmap_word == (S % 4 == 0 && cwd == S / 4), "bmap_word");
  CHECK(L.bmap_quad == (S % 4 != 0 && 4 * S * (L.map16 ? 2 : 4) <= kBmapLds), "bmap_quad");
}

static void check_pieces(const Case &c, const DdtLayout &L, int al) {
  const uint64_t S = (uint64_t)c.size;
  const int64_t ext = c.ub - c.lb;
  std::vector<DPiece> v;
  uint32_t K = 0;
  if (!plan_pieces(L, al, v, K)) return;
  const uint64_t A = gcd64(16, (uint64_t)(ext < 0 ? -ext : ext));
  const uint64_t npi = v.size();
  CHECK(npi > 0 && K >= (uint32_t)kCB, "al %d: %llu pieces, K %u", al, (unsigned long long)npi, K);
  uint64_t at = 0;
  for (uint64_t p = 0; p < npi; p++) {
    const uint64_t w = (uint64_t)1 << v[p].lg;
    CHECK(v[p].soff == at && at + w <= S, "al %d: piece %llu at stream %u after %llu", al, (unsigned long long)p, v[p].soff,
          (unsigned long long)at);
    for (uint64_t i = 0; i < w; i++)
      CHECK(c.m[at + i] == (int64_t)v[p].uoff + (int64_t)i, "al %d: piece %llu byte %llu", al, (unsigned long long)p, (unsigned long long)i);
    CHECK(w <= 16 && ((al + (int64_t)v[p].uoff) % (int64_t)w + (int64_t)w) % (int64_t)w == 0, "al %d: piece %llu of %llu bytes at user %d is misaligned",
          al, (unsigned long long)p, (unsigned long long)w, v[p].uoff);
    CHECK(A % w == 0, "al %d: piece width %llu does not divide gcd(16, extent) = %llu", al, (unsigned long long)w, (unsigned long long)A);
    at += w;
  }
  CHECK(at == S, "al %d: the pieces cover %llu of %llu bytes", al, (unsigned long long)at, (unsigned long long)S);
  for (uint64_t j = 0; j < npi; j++) {
    const uint64_t e = j + K - 1;
    const uint64_t end = (e / npi) * S + v[e % npi].soff + ((uint64_t)1 << v[e % npi].lg);
    CHECK(end - v[j].soff + 32 <= (uint64_t)kPieceStage, "al %d: %u pieces from %llu stage %llu bytes", al, K,
          (unsigned long long)j, (unsigned long long)(end - v[j].soff));
  }
  for (uint64_t b = 0; b < S; b++) {
    const uint32_t p = piece_of(v, b);
    CHECK(p < npi && v[p].soff <= b && b < v[p].soff + ((uint64_t)1 << v[p].lg), "al %d: piece_of(%llu) = %u", al, (unsigned long long)b, p);
  }
}

static void check_blocks(const Case &c, const DdtLayout &L, uint64_t tmax, bool span_pack) {
  const uint64_t S = (uint64_t)c.size;
  BlkPlan P;
  if (!plan_blocks(L, tmax, span_pack, P)) return;
  const uint64_t nb = P.blocks.size();
  CHECK(nb > 0 && P.dev.size() == nb + 1, "%llu blocks, device table of %zu", (unsigned long long)nb, P.dev.size());
  std::vector<uint32_t> idx(S);   // block of every stream byte
  uint64_t at = 0;
  for (uint64_t b = 0; b < nb; b++) {
    const HBlk &h = P.blocks[b];
    CHECK(h.soff == at && h.len > 0 && at + h.len <= S, "block %llu at stream %u after %llu", (unsigned long long)b, h.soff, (unsigned long long)at);
    CHECK(P.dev[b].soff == h.soff && (int64_t)P.dev[b].uoff == h.uoff, "device entry %llu", (unsigned long long)b);
    for (uint64_t i = 0; i < h.len; i++) {
      CHECK(c.m[at + i] == h.uoff + (int64_t)i, "block %llu byte %llu", (unsigned long long)b, (unsigned long long)i);
      idx[at + i] = (uint32_t)b;
    }
    at += h.len;
  }
  CHECK(at == S, "the blocks cover %llu of %llu bytes", (unsigned long long)at, (unsigned long long)S);
  CHECK(P.dev[nb].uoff == 0 && P.dev[nb].soff == S, "sentinel {%d, %u}", P.dev[nb].uoff, P.dev[nb].soff);
  const uint64_t nk = (S + kBlkG - 1) / kBlkG;
  CHECK(P.tfirst.size() == nk + 1, "tfirst of %zu entries for %llu stretches", P.tfirst.size(), (unsigned long long)nk);
  for (uint64_t k = 0; k < nk; k++)
    CHECK(P.tfirst[k] <= idx[k * kBlkG] && idx[k * kBlkG] <= P.tfirst[k + 1] && P.tfirst[k + 1] < nb, "tfirst[%llu]", (unsigned long long)k);
  // stream stretches [s, s + T): every start for a small instance; else the
  // starts at a block's last byte and those that end on a block's first byte,
  // where the block count and the user span of a stretch peak
  std::vector<uint64_t> starts;
  auto starts_for = [&](uint64_t T) {
    starts.clear();
    if (S <= 4096) {
      for (uint64_t s = 0; s < S; s++) starts.push_back(s);
      return;
    }
    for (uint64_t b = 0; b < nb; b++) {
      starts.push_back(P.blocks[b].soff + P.blocks[b].len - 1);
      const uint64_t first = ((T - 1) / S + 1) * S + P.blocks[b].soff;   // a copy of the block's first byte at or past T - 1
      starts.push_back((first - (T - 1)) % S);
    }
  };
  auto blk_at = [&](uint64_t x) { return (x / S) * nb + idx[x % S]; };
  CHECK(P.T >= 512 && P.T <= tmax && (P.T & (P.T - 1)) == 0, "T = %llu", (unsigned long long)P.T);
  starts_for(P.T);
  for (uint64_t s : starts)
    CHECK(blk_at(s + P.T - 1) - blk_at(s) + 1 <= kBlkCap, "T = %llu: the stretch at %llu overlaps %llu blocks", (unsigned long long)P.T,
          (unsigned long long)s, (unsigned long long)(blk_at(s + P.T - 1) - blk_at(s) + 1));
  if (P.Tspan) {
    CHECK(span_pack && P.Tspan % 64 == 0, "Tspan = %llu", (unsigned long long)P.Tspan);
    starts_for(P.Tspan);
    for (uint64_t s : starts) {
      const uint64_t n = blk_at(s + P.Tspan - 1) - blk_at(s) + 1;
      CHECK(n + 1 <= P.capspan, "Tspan = %llu: the stretch at %llu overlaps %llu blocks, capspan %u", (unsigned long long)P.Tspan,
            (unsigned long long)s, (unsigned long long)n, P.capspan);
      const int64_t lo = U(c, s), hi = U(c, s + P.Tspan - 1);
      CHECK(hi >= lo && hi - lo + 1 + 32 <= (int64_t)kBlkSpan, "Tspan = %llu: the stretch at %llu spans user [%lld, %lld]",
            (unsigned long long)P.Tspan, (unsigned long long)s, (long long)lo, (long long)hi);
    }
    // the span kernel reads a stretch as [addr(first), addr(last)]: the blocks ascend, instance after instance
    for (uint64_t x = 0; x + 1 < 2 * S; x++) CHECK(U(c, x) < U(c, x + 1), "Tspan set for a layout that does not ascend at %llu", (unsigned long long)x);
  } else {
    CHECK(P.capspan == 0, "capspan without Tspan");
  }
}

static void check_span(const Case &c, const DdtLayout &L) {
  for (size_t count : {(size_t)1, (size_t)3}) {
    int64_t lo = 1, hi = -1;
    ddt_span(L, count, &lo, &hi);
    const int64_t tail = (int64_t)(count - 1) * (c.ub - c.lb);
    CHECK(lo == c.true_lb + std::min<int64_t>(0, tail) && hi == c.true_ub + std::max<int64_t>(0, tail),
          "span of %zu instances [%lld, %lld)", count, (long long)lo, (long long)hi);
  }
}

// a description cut short, or with the wrong size, is refused; the copy ends
// with the description so that a read past it is the sanitizer's to report
static void check_rejection(const Case &c) {
  for (uint32_t k = 1; k < c.nrec; k++) {
    bool data = false;   // the cut takes data records along
    for (uint32_t i = k; i < c.nrec; i++) {
      uint16_t flags, type;
      memcpy(&flags, &c.desc[32 * i], 2);
      memcpy(&type, &c.desc[32 * i + 2], 2);
      data = data || (type > 3 && (flags & 0x0100));
    }
    uint8_t *cut = (uint8_t *)malloc(32 * (size_t)k);
    memcpy(cut, c.desc.data(), 32 * (size_t)k);
    DdtLayout T;
    const int rc = ddt_layout_create(cut, k, c.basic, (size_t)c.size, c.lb, c.ub, true, T);
    free(cut);
    // (a cut that drops only END_LOOP / bound markers still describes every byte)
    CHECK(rc != MX_SUCCESS || !data, "the description cut to %u of %u records is accepted", k, c.nrec);
  }
  for (int64_t off : {(int64_t)-1, (int64_t)1}) {
    DdtLayout T;
    CHECK(ddt_layout_create(c.desc.data(), c.nrec, c.basic, (size_t)(c.size + off), c.lb, c.ub, true, T) != MX_SUCCESS,
          "size %lld accepted for a description of %lld bytes", (long long)(c.size + off), (long long)c.size);
  }
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s CASEFILE\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  char magic[8];
  uint32_t ncases = 0;
  rd(f, magic, 8);
  rd(f, &ncases, 4);
  if (memcmp(magic, "MXLAYC01", 8) != 0) {
    fprintf(stderr, "FAIL: bad case file magic\n");
    return 2;
  }
  size_t bmaps = 0;
  for (uint32_t i = 0; i < ncases; i++) {
    Case c;
    memset(c.name, 0, sizeof(c.name));
    rd(f, c.name, 64);
    rd(f, &c.nrec, 4);
    rd(f, &c.pad, 4);
    rd(f, &c.size, 8);
    rd(f, &c.lb, 8);
    rd(f, &c.ub, 8);
    rd(f, &c.true_lb, 8);
    rd(f, &c.true_ub, 8);
    rd(f, c.basic, sizeof(c.basic));
    c.desc.resize(32 * (size_t)c.nrec);
    rd(f, c.desc.data(), c.desc.size());
    c.m.resize((size_t)c.size);
    rd(f, c.m.data(), 8 * c.m.size());
    g_case = c.name;
    CHECK(c.size > 0 && c.nrec > 0, "empty case");
    DdtLayout L;
    const int rc = ddt_layout_create(c.desc.data(), c.nrec, c.basic, (size_t)c.size, c.lb, c.ub, true, L);
    CHECK(rc == MX_SUCCESS, "ddt_layout_create: %d", rc);
    check_runs(c, L);
    check_bmap(c, L);
    check_span(c, L);
    if (!L.bmap.empty()) {
      bmaps++;
      for (int al = 0; al < 16; al++) check_pieces(c, L, al);
      // MX_CONV_BMAP_INST=0: tiles of 256-byte multiples only
      DdtLayout L2;
      CHECK(ddt_layout_create(c.desc.data(), c.nrec, c.basic, (size_t)c.size, c.lb, c.ub, false, L2) == MX_SUCCESS, "inst_tiles off");
      check_bmap(c, L2);
    }
    // the default plan, and the other tiles MX_CONV_BLK_T / MX_CONV_BLK_SPAN can ask for
    check_blocks(c, L, 16384, true);
    check_blocks(c, L, 16384, false);
    check_blocks(c, L, 4096, true);
    check_blocks(c, L, kBlkMaxT, true);
    check_rejection(c);
  }
  fclose(f);
  printf("ddt_layout_check: %u cases (%zu with a byte map) keep every invariant\n", ncases, bmaps);
  return 0;
}
