// exchange_vec_check.cpp -- host check of the strided exchange planner
// (csrc/mx_exchange_vec_plan.hip): the XLay map and its magic-division form
// against a brute-force walk of random layouts, unit and word-width
// selection, plans whose blocks tile every job's stream exactly once (job
// starts in the middle of a block and of an instance included), and every
// qualification rule, on descriptions flattened by the layout planner
// (csrc/mx_ddt_layout.hip).  No pointer of a job is ever dereferenced.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <random>
#include <vector>

#include "mx_exchange_vec_plan.hpp"

using namespace mx;

static int fails = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      if (fails++ < 20) {                               \
        printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
        printf(__VA_ARGS__);                            \
        printf("\n");                                   \
      }                                                 \
    }                                                   \
  } while (0)

static std::mt19937_64 rng(20251);
static uint64_t rnd(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); }

// the largest power of two <= 16 dividing every value
static unsigned brute_unit(std::vector<uint64_t> v) {
  unsigned u = 16;
  for (uint64_t x : v)
    while (u > 1 && x % u) u /= 2;
  return u;
}

// ---- the map -------------------------------------------------------------------
// brute force: walk instances, blocks and bytes in stream order
static std::vector<int64_t> walk(const XLay &l, uint64_t count) {
  std::vector<int64_t> m;
  for (uint64_t i = 0; i < count; i++)
    for (uint64_t k = 0; k < l.cnt1; k++)
      for (uint64_t o = 0; o < l.blen; o++) m.push_back((int64_t)i * l.ext + l.disp + (int64_t)k * l.stride1 + (int64_t)o);
  return m;
}

// the kernel's form (xv_start / xv_off, the functions k_exchange_vec calls):
// the stretch start by magic division, then every word from it in 32 bits
static int64_t kernel_off(const XSide &S, uint64_t p0, uint32_t rel) { return xv_off(S, xv_start(S, p0), rel); }

static XLay random_lay(unsigned unit) {
  XLay l;
  l.blen = unit * rnd(1, 40);
  l.cnt1 = rnd(1, 7);
  l.stride1 = (int64_t)(l.blen + unit * rnd(0, 30)) * (rnd(0, 3) ? 1 : -1);
  l.disp = (int64_t)(unit * rnd(0, 8)) - (int64_t)(unit * 4);
  l.ext = (int64_t)(l.blen * l.cnt1 + unit * rnd(0, 50));
  if (l.cnt1 == 1) l.stride1 = 0;
  return l;
}

static void check_map() {
  for (int it = 0; it < 300; it++) {
    const unsigned unit = 1u << rnd(0, 4);
    const XLay l = random_lay(unit);
    const uint64_t count = rnd(1, 9);
    const std::vector<int64_t> m = walk(l, count);
    XVJob j;
    const int rc = xvjob_make((const char *)(uintptr_t)4096, l, 0, (char *)(uintptr_t)8192, xlay_flat(), 0, m.size(), &j);
    const unsigned W = brute_unit({l.blen, xabs(l.disp), xabs(l.stride1), xabs(l.ext), (uint64_t)m.size()});
    CHECK(j.W == W && rc == (W >= 4 ? MX_SUCCESS : MX_ERR_UNSUPPORTED), "W %u (%u expected) gives rc %d", j.W, W, rc);
    for (uint64_t b = 0; b < m.size(); b++) CHECK(xlay_off(l, b) == m[b], "xlay_off at %llu", (unsigned long long)b);
    for (int k = 0; k < 20; k++) {
      const uint64_t p0 = rnd(0, m.size() - 1);
      const uint32_t rel = (uint32_t)rnd(0, m.size() - 1 - p0);
      CHECK(kernel_off(j.s, p0, rel) == m[p0 + rel], "kernel map at %llu + %u", (unsigned long long)p0, rel);
    }
  }
  // the largest block and the longest stretch a workgroup maps from one start
  XLay l{0, kVecMaxBlen, 3, (int64_t)kVecMaxBlen + 64, 4 * (int64_t)kVecMaxBlen};
  XVJob j;
  CHECK(xvjob_make((const char *)(uintptr_t)4096, l, 0, (char *)(uintptr_t)8192, xlay_flat(), 0, 6 * kVecMaxBlen, &j) == MX_SUCCESS, "big blen");
  for (int k = 0; k < 20000; k++) {
    const uint64_t p0 = rnd(0, 6 * kVecMaxBlen - xv_block_bytes(16) - 1) & ~(uint64_t)15;
    const uint32_t rel = (uint32_t)rnd(0, xv_block_bytes(16) - 1);
    CHECK(kernel_off(j.s, p0, rel) == xlay_off(l, p0 + rel), "big blen at %llu + %u", (unsigned long long)p0, rel);
  }
  // small blocks: a stretch crosses thousands of blocks and hundreds of instances
  for (uint64_t cnt1 : {(uint64_t)1, (uint64_t)2, (uint64_t)7, (uint64_t)5000, (uint64_t)1 << 33}) {
    const XLay s4{8, 4, cnt1, cnt1 > 1 ? 12 : 0, cnt1 < 10000 ? (int64_t)(12 * cnt1 + 4) : (int64_t)1 << 37};
    const uint64_t total = (uint64_t)1 << 22;
    CHECK(xvjob_make((const char *)(uintptr_t)4096, s4, 0, (char *)(uintptr_t)8192, xlay_flat(), 0, total, &j) == MX_SUCCESS, "small blocks");
    for (int k = 0; k < 20000; k++) {
      const uint64_t p0 = rnd(0, total - xv_block_bytes(16) - 1) & ~(uint64_t)3;
      const uint32_t rel = (uint32_t)rnd(0, xv_block_bytes(16) - 1);
      CHECK(kernel_off(j.s, p0, rel) == xlay_off(s4, p0 + rel), "cnt1 %llu at %llu + %u", (unsigned long long)cnt1, (unsigned long long)p0, rel);
    }
  }
  // a flat side
  const XLay f = xlay_flat(-24);
  CHECK(xlay_is_flat(f) && xlay_off(f, 100) == 76, "flat map");
}

// ---- units and widths ------------------------------------------------------------
static void check_units() {
  for (int it = 0; it < 2000; it++) {
    const unsigned unit = 1u << rnd(0, 4);
    const XLay s = random_lay(unit), d = random_lay(1u << rnd(0, 4));
    const uintptr_t sa = 4096 + rnd(0, 64), da = 8192 + 16 * rnd(0, 4);
    CHECK(xlay_unit(s, sa) == brute_unit({s.blen, xabs(s.disp), xabs(s.stride1), xabs(s.ext), sa}), "send unit");
    const uint64_t ps = 4 * rnd(0, 100), pd = 8 * rnd(0, 100), bytes = 4 * rnd(1, 1000);
    XVJob j;
    const int rc = xvjob_make((const char *)sa, s, ps, (char *)da, d, pd, bytes, &j);
    const unsigned W = brute_unit({s.blen, xabs(s.disp), xabs(s.stride1), xabs(s.ext), sa, d.blen, xabs(d.disp),
                                   xabs(d.stride1), xabs(d.ext), da, ps, pd, bytes});
    CHECK(j.W == W, "W %u, expected %u", j.W, W);
    CHECK(rc == (W >= 4 ? MX_SUCCESS : MX_ERR_UNSUPPORTED), "W %u gives rc %d", W, rc);
  }
  // a flat side: the address and its displacement only
  CHECK(xlay_unit(xlay_flat(), 4096) == 16 && xlay_unit(xlay_flat(8), 4096) == 8 && xlay_unit(xlay_flat(), 4100) == 4, "flat units");
  XVJob j;
  const XLay b2{0, 2, 4, 4, 16};   // 2-byte blocks
  CHECK(xvjob_make((const char *)(uintptr_t)4096, b2, 0, (char *)(uintptr_t)8192, xlay_flat(), 0, 64, &j) == MX_ERR_UNSUPPORTED, "2-byte blocks");
  CHECK(xvjob_make((const char *)(uintptr_t)4096, xlay_flat(), 0, (char *)(uintptr_t)8192, xlay_flat(), 0, (uint64_t)1 << 48, &j) == MX_ERR_ARG,
        "a stream past the magic range");
}

// ---- plans -------------------------------------------------------------------------
static void check_plans() {
  for (int it = 0; it < 200; it++) {
    const size_t n = rnd(0, kXMaxJobs);
    std::vector<XVJob> in(n);
    for (XVJob &j : in) {
      const unsigned unit = 4u << rnd(0, 2);
      const XLay s = random_lay(unit), d = rnd(0, 2) ? random_lay(4u << rnd(0, 2)) : xlay_flat();
      const uint64_t kind = rnd(0, 9);
      uint64_t bytes = kind == 0 ? 0 : kind == 1 ? rnd(1, 40) * xv_block_bytes(unit) : 4 * rnd(1, 30000);
      // a job starts anywhere its word allows: inside a block, inside an instance
      const uint64_t ps = 16 * rnd(0, 5000), pd = 16 * rnd(0, 5000);
      const int rc = xvjob_make((const char *)(uintptr_t)(1 << 20), s, ps, (char *)(uintptr_t)(1 << 24), d, pd, bytes, &j);
      CHECK(rc == MX_SUCCESS, "job");
    }
    XVPlan p;
    const uint64_t max_grid = it % 3 == 0 ? rnd(1, 50) : kXMaxGridBlocks;
    CHECK(xvplan_build(in.data(), in.size(), p, max_grid) == MX_SUCCESS, "plan");
    size_t nonempty = 0, bytes = 0;
    for (const XVJob &j : in) { nonempty += j.bytes != 0; bytes += j.bytes; }
    CHECK(p.jobs.size() == nonempty && p.bytes == bytes && p.seg.size() == nonempty + 1, "jobs kept");
    uint64_t sum = 0;
    for (size_t i = 0; i < p.jobs.size(); i++) {
      const uint64_t nb = xvjob_blocks(p.jobs[i].bytes, p.jobs[i].W);
      CHECK(i == 0 || xvjob_blocks(p.jobs[i - 1].bytes, p.jobs[i - 1].W) <= nb, "block order");
      CHECK(p.jobs[i].bytes % p.jobs[i].W == 0 && p.jobs[i].pos_s % p.jobs[i].W == 0 && p.jobs[i].pos_d % p.jobs[i].W == 0, "whole words");
      sum += nb;
    }
    CHECK(sum == p.nblocks && p.seg.back().block0 == sum, "block count");
    uint64_t at = 0;
    for (const XLaunch &l : p.launch) {
      CHECK(l.block0 == at && l.nblocks > 0 && l.nblocks <= max_grid, "launches");
      CHECK((uint64_t)l.nblocks * kXThreads < ((uint64_t)1 << 32), "grid");
      at += l.nblocks;
    }
    CHECK(at == sum, "launches cover the blocks");
    // every stream byte of every job belongs to exactly one block: block k of
    // a job is its bytes [k, k + 1) * xv_block_bytes(W), as the kernel takes them
    std::vector<std::vector<uint8_t>> seen(p.jobs.size());
    for (size_t i = 0; i < p.jobs.size(); i++) seen[i].assign(xvjob_blocks(p.jobs[i].bytes, p.jobs[i].W), 0);
    uint32_t last = ~0u;
    for (uint64_t b = 0; b < p.nblocks; b++) {
      uint32_t j;
      uint64_t k;
      xplan_lookup(p.seg.data(), (uint32_t)p.jobs.size(), b, &j, &k);
      CHECK(j < p.jobs.size() && k < seen[j].size(), "block %llu maps outside", (unsigned long long)b);
      if (j >= p.jobs.size() || k >= seen[j].size()) break;
      CHECK(!seen[j][k], "block twice");
      seen[j][k] = 1;
      const uint64_t b0 = k * xv_block_bytes(p.jobs[j].W);
      CHECK(b0 < p.jobs[j].bytes, "an empty block");
      size_t sg = 0;   // the last segment that starts at or before b
      for (size_t i = 0; i < p.jobs.size(); i++)
        if (p.seg[i].block0 <= b) sg = i;
      const uint64_t alive = p.jobs.size() - sg;
      if (alive > 1 && b) CHECK(j != last, "neighbouring blocks of one job");
      last = j;
    }
    for (size_t i = 0; i < p.jobs.size(); i++)
      for (uint8_t v : seen[i]) CHECK(v == 1, "a block never dealt");
  }
  XVPlan p;
  XVJob bad;
  memset(&bad, 0, sizeof bad);
  bad.src = (const char *)(uintptr_t)64;
  bad.dst = (char *)(uintptr_t)128;
  bad.bytes = 64;
  bad.W = 2;
  CHECK(xvplan_build(&bad, 1, p) == MX_ERR_ARG, "a 2-byte word is planned");
  bad.W = 8;
  bad.bytes = 60;
  CHECK(xvplan_build(&bad, 1, p) == MX_ERR_ARG, "a job of half a word is planned");
}

// ---- qualification -----------------------------------------------------------------
struct RecElem { uint16_t flags, type; uint32_t count; uint64_t blocklen; int64_t extent; int64_t disp; };
struct RecLoop { uint16_t flags, type; uint32_t items; uint32_t loops; uint32_t pad; uint64_t unused; int64_t extent; };
static void elem(std::vector<uint8_t> &d, uint16_t type, uint32_t count, uint64_t blocklen, int64_t extent, int64_t disp) {
  RecElem e{0x0100, type, count, blocklen, extent, disp};
  d.insert(d.end(), (uint8_t *)&e, (uint8_t *)&e + 32);
}
static void end_loop(std::vector<uint8_t> &d, uint32_t items) {
  RecElem e{0, 1, items, 0, 0, 0};
  d.insert(d.end(), (uint8_t *)&e, (uint8_t *)&e + 32);
}
static bool qualifies(const std::vector<uint8_t> &body, size_t size, int64_t lb, int64_t ub, bool recv, XLay *out, DdtLayout *keep = nullptr) {
  std::vector<uint8_t> d = body;
  end_loop(d, (uint32_t)(d.size() / 32));
  DdtLayout L;
  const int rc = ddt_layout_create(d.data(), d.size() / 32, nullptr, size, lb, ub, false, L);
  CHECK(rc == MX_SUCCESS, "layout rc %d", rc);
  if (keep) *keep = L;
  return rc == MX_SUCCESS && xlay_from(L, recv, out);
}

static void check_qualification() {
  const uint16_t I4 = 6, I8 = 7, I2 = 5, I16 = 8;
  XLay l;
  std::vector<uint8_t> d;
  // MPI_Type_vector(3, 2, 5, MPI_INT): blen 8, stride 20, extent 48
  elem(d, I4, 3, 2, 20, 0);
  CHECK(qualifies(d, 24, 0, 48, true, &l) && l.blen == 8 && l.cnt1 == 3 && l.stride1 == 20 && l.ext == 48 && l.disp == 0, "vector");
  CHECK(xlay_unit(l, 4096) == 4, "vector unit");
  // resized contiguous: one block of 8 bytes, extent 24
  d.clear();
  elem(d, I8, 1, 1, 8, 0);
  CHECK(qualifies(d, 8, 0, 24, true, &l) && l.blen == 8 && l.cnt1 == 1 && l.ext == 24 && !xlay_is_flat(l), "resized");
  // contiguous: flat
  CHECK(qualifies(d, 8, 0, 8, true, &l) && xlay_is_flat(l), "contiguous is flat");
  // a negative displacement
  d.clear();
  elem(d, I8, 3, 1, 24, -8);
  CHECK(qualifies(d, 24, -8, 64, true, &l) && l.disp == -8 && xlay_unit(l, 4096) == 8, "disp -8");
  // a negative stride: the send side only
  d.clear();
  elem(d, I8, 3, 2, -32, 64);
  CHECK(qualifies(d, 48, 0, 96, false, &l) && l.stride1 == -32, "negative stride sends");
  CHECK(!qualifies(d, 48, 0, 96, true, &l), "a non-monotonic layout receives");
  // overlapping instances (extent below the span): not monotonic
  d.clear();
  elem(d, I4, 3, 1, 8, 0);
  CHECK(qualifies(d, 12, 0, 8, false, &l) && !qualifies(d, 12, 0, 8, true, &l), "overlapping instances");
  // two runs (a struct)
  d.clear();
  elem(d, I4, 2, 1, 8, 0);
  elem(d, I8, 1, 1, 8, 32);
  CHECK(!qualifies(d, 16, 0, 40, false, &l), "a two-run struct");
  // two levels: a loop over a strided element
  d.clear();
  {
    RecLoop L{0, 0, 2, 3, 0, 0, 64};
    d.insert(d.end(), (uint8_t *)&L, (uint8_t *)&L + 32);
    elem(d, I4, 2, 1, 8, 0);
    end_loop(d, 2);
  }
  DdtLayout K;
  CHECK(!qualifies(d, 24, 0, 192, false, &l, &K) && K.runs.size() == 1 && K.runs[0].cnt2 == 3, "cnt2 > 1");
  // 2-byte blocks qualify as a layout; their unit makes the call unsupported
  d.clear();
  elem(d, I2, 4, 1, 4, 0);
  CHECK(qualifies(d, 8, 0, 16, true, &l) && xlay_unit(l, 4096) == 2, "2-byte blocks");
  // the block length limit
  d.clear();
  elem(d, I16, 2, kVecMaxBlen / 16, 2 * (int64_t)kVecMaxBlen, 0);
  CHECK(qualifies(d, 2 * kVecMaxBlen, 0, 4 * (int64_t)kVecMaxBlen, true, &l), "blen at the limit");
  d.clear();
  elem(d, I16, 2, kVecMaxBlen / 16 + 1, 2 * (int64_t)kVecMaxBlen, 0);
  CHECK(!qualifies(d, 2 * kVecMaxBlen + 32, 0, 4 * (int64_t)kVecMaxBlen, true, &l), "blen above the limit");
}

int main() {
  check_map();
  check_units();
  check_plans();
  check_qualification();
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("exchange_vec_check: ok\n");
  return 0;
}
