// rooted_check.cpp -- host check of the rooted exchange planner
// (csrc/mx_rooted_plan.hip).  It simulates n = 1, 2, 3, 5 and 16 ranks on host
// byte arrays: every rank's planned jobs run through xlay_off round by round
// (staged, zero-copy and local plans), and the result is compared with a
// brute-force walk of the layouts.  Every destination byte of a layout is
// written exactly once; no gap byte, no byte past a cut and no byte of a
// non-significant buffer is written; no two jobs of a round overlap in a
// staging area and none leaves it; a staging byte is read only after the rank
// the reader waits for wrote it; the round counts equal the formula of
// mx_comm_rooted_rounds; the verdict is the same whichever rank evaluates it.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>

#include "mx_rooted_plan.hpp"

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

static std::mt19937_64 rng(90210);
static uint64_t rnd(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); }

constexpr uint8_t FILL = 0xA5;
constexpr int64_t ORG = 4096;      // where offset 0 of a simulated buffer sits in its array
constexpr size_t kRoom = 16384;    // what one block spans at the most (3456 + 480 stream bytes, a third of the extent)

// brute force: the offsets of the first `bytes` stream bytes, instance by instance
static std::vector<int64_t> walk(const XLay &l, uint64_t bytes) {
  std::vector<int64_t> m;
  if (l.blen == 0) {
    for (uint64_t b = 0; b < bytes; b++) m.push_back(l.disp + (int64_t)b);
    return m;
  }
  for (uint64_t i = 0; m.size() < bytes; i++)
    for (uint64_t k = 0; k < l.cnt1 && m.size() < bytes; k++)
      for (uint64_t o = 0; o < l.blen && m.size() < bytes; o++)
        m.push_back((int64_t)i * l.ext + l.disp + (int64_t)k * l.stride1 + (int64_t)o);
  return m;
}

// the layouts of tests/test_rooted_gpu.py (send-only ones last)
struct Shape { const char *name; XLay l; uint64_t size; bool recv_ok; };
static const Shape kShapes[] = {
    {"flat", {0, 0, 1, 0, 1}, 1, true},
    {"b4s8", {0, 4, 6, 8, 48}, 24, true},
    {"vec", {0, 8, 3, 20, 48}, 24, true},
    {"b24s40", {0, 24, 3, 40, 120}, 72, true},
    {"b16s48", {0, 16, 3, 48, 144}, 48, true},
    {"b48s64", {0, 48, 2, 64, 128}, 96, true},
    {"resized", {0, 8, 1, 0, 24}, 8, true},
    {"dispm8", {-8, 8, 3, 24, 72}, 24, true},
    {"negstride", {64, 16, 3, -32, 96}, 48, false},
};
constexpr int kNShapes = sizeof kShapes / sizeof kShapes[0];

struct Sim {
  int n, kind, root;
  bool inplace;
  Shape single[MX_MAX_RANKS], multi;
  uint64_t scount[MX_MAX_RANKS];             // instances (bytes for flat) of each single side
  uint64_t mcount[MX_MAX_RANKS];             // ... of each block of the multi side
  int64_t mdispl[MX_MAX_RANKS];              // in extents (bytes for flat)
  uintptr_t saddr[MX_MAX_RANKS], maddr;      // the simulated addresses (alignment only)
  size_t main_bytes;
  RRow rows[MX_MAX_RANKS];
  std::vector<uint8_t> sbuf[MX_MAX_RANKS], mbuf, stage[MX_MAX_RANKS];
  std::vector<uint8_t> swr[MX_MAX_RANKS], mwr;   // writes per byte
  std::vector<int> stage_writer[MX_MAX_RANKS];   // who wrote a staging byte this round (-1: nobody)
};

static void make_rows(Sim &S) {
  for (int p = 0; p < S.n; p++) {
    RRow &r = S.rows[p];
    memset(&r, 0, sizeof r);
    r.h.root = S.root;
    r.h.kind = S.kind;
    r.h.verdict = 1;
    r.h.lay = r.h.mlay = xlay_flat();
    r.h.unit = r.h.munit = 16;
    r.h.inplace = p == S.root && S.inplace;
    if (!r.h.inplace) {
      r.h.lay = S.single[p].l;
      r.h.bytes = S.scount[p] * S.single[p].size;
      if (r.h.bytes) r.h.unit = xlay_unit(r.h.lay, S.saddr[p]);
      r.h.mis = (uint32_t)((S.saddr[p] + (uint64_t)r.h.lay.disp) & 15);
    }
    if (p != S.root) continue;
    r.h.mlay = S.multi.l;
    const int64_t ext = xlay_is_flat(S.multi.l) ? 1 : S.multi.l.ext;
    for (int q = 0; q < S.n; q++) {
      r.mbytes[q] = S.mcount[q] * S.multi.size;
      r.moffs[q] = S.mdispl[q] * ext;
    }
    r.h.munit = xlay_unit(r.h.mlay, S.maddr);
    r.h.mmis = (uint32_t)((S.maddr + (uint64_t)r.h.mlay.disp) & 15);
  }
}

static uint8_t *end_byte(Sim &S, const REnd &e, uint64_t b, bool write, int by) {
  const int64_t off = e.off + xlay_off(e.lay, e.pos + b);
  if (e.buf == RB_STAGE) {
    CHECK(off >= 0 && (size_t)off < S.main_bytes, "a job leaves the staging of rank %d: offset %lld", e.rank, (long long)off);
    if (off < 0 || (size_t)off >= S.main_bytes) return nullptr;
    if (write) {
      CHECK(S.stage_writer[e.rank][(size_t)off] < 0, "two jobs of a round overlap in the staging of rank %d", e.rank);
      S.stage_writer[e.rank][(size_t)off] = by;
    }
    return &S.stage[e.rank][(size_t)off];
  }
  std::vector<uint8_t> &buf = e.buf == RB_MULTI ? S.mbuf : S.sbuf[e.rank];
  const int64_t at = ORG + off;
  CHECK(at >= 0 && (size_t)at < buf.size(), "offset %lld outside the simulated buffer", (long long)off);
  if (at < 0 || (size_t)at >= buf.size()) return nullptr;
  if (write) (e.buf == RB_MULTI ? S.mwr : S.swr[e.rank])[(size_t)at]++;
  return &buf[(size_t)at];
}

// the simulated address of an end's user pointer, for the word rule
static uintptr_t end_addr(const Sim &S, const REnd &e) {
  const uintptr_t base = e.buf == RB_STAGE ? (uintptr_t)0x7000000 : e.buf == RB_MULTI ? S.maddr : S.saddr[e.rank];
  return base + (uintptr_t)e.off;
}

// runs the jobs `rank` launches; wait: the ranks its wait before them names
// (staging reads must come from those); owners: the stagings it may write
static void run_jobs(Sim &S, const RHead &h, int rank, const std::vector<RJob> &jobs, uint32_t ready, uint32_t done,
                     bool mp) {
  CHECK(jobs.size() <= (size_t)MX_MAX_RANKS, "%zu jobs in one launch", jobs.size());
  for (const RJob &j : jobs) {
    CHECK(j.len > 0, "an empty job");
    if (j.bytes) {
      CHECK(xlay_is_flat(j.s.lay) && xlay_is_flat(j.d.lay), "a byte job with a strided side");
    } else {
      XVJob v;
      const int rc = xvjob_make((const char *)end_addr(S, j.s), j.s.lay, j.s.pos, (char *)end_addr(S, j.d), j.d.lay,
                                j.d.pos, j.len, &v);
      CHECK(rc == MX_SUCCESS, "a planned job misses the word rule (rc %d)", rc);
    }
    if (mp) {
      // what a rank writes: its own single side, the root its multi side, a staging whose owner it waited for
      if (j.d.buf == RB_SINGLE) CHECK(j.d.rank == rank, "rank %d writes rank %d's buffer", rank, j.d.rank);
      if (j.d.buf == RB_MULTI) CHECK(rank == h.root && h.kind == RK_GATHER, "rank %d writes the root's buffer", rank);
      if (j.d.buf == RB_STAGE && j.d.rank != rank)
        CHECK((done >> j.d.rank) & 1, "rank %d writes the staging of %d without its DONE", rank, j.d.rank);
      if (j.s.buf == RB_SINGLE && j.s.rank != rank)
        CHECK((ready >> j.s.rank) & 1, "rank %d reads rank %d's buffer without its READY", rank, j.s.rank);
      if (j.s.buf == RB_MULTI && rank != h.root)
        CHECK((ready >> h.root) & 1, "rank %d reads the root's buffer without its READY", rank);
      if (j.s.buf == RB_MULTI) CHECK(h.kind == RK_SCATTER, "a gather reads the receive side");
    }
    for (uint64_t b = 0; b < j.len; b++) {
      if (j.s.buf == RB_STAGE) {
        CHECK(j.s.rank == rank, "rank %d reads the staging of %d", rank, j.s.rank);
        const int64_t off = j.s.off + xlay_off(j.s.lay, j.s.pos + b);
        if (off >= 0 && (size_t)off < S.main_bytes) {
          const int w = S.stage_writer[j.s.rank][(size_t)off];
          CHECK(w >= 0 && ((ready >> w) & 1), "rank %d reads a staging byte rank %d wrote without waiting for it", rank, w);
        }
      }
      const uint8_t *sp = end_byte(S, j.s, b, false, rank);
      uint8_t *dp = end_byte(S, j.d, b, true, rank);
      if (sp && dp) *dp = *sp;
    }
  }
}

enum { MODE_LOCAL, MODE_STAGED, MODE_ZC };

static void simulate(Sim &S, int mode, const char *what) {
  const int n = S.n;
  make_rows(S);
  // every rank evaluates its own copy of the rows
  RHead h;
  int rc0 = 0;
  for (int r = 0; r < n; r++) {
    std::vector<RRow> copy(S.rows, S.rows + n);
    RHead hr;
    memset(&hr, 0, sizeof hr);
    const int rc = rooted_verdict(copy.data(), n, 0, &hr);
    if (r == 0) { rc0 = rc; h = hr; }
    CHECK(rc == rc0, "%s: rank %d's verdict %d, rank 0's %d", what, r, rc, rc0);
    if (!rc && !rc0) {
      CHECK(hr.max_block == h.max_block && hr.inplace == h.inplace && hr.root == h.root && hr.kind == h.kind,
            "%s: rank %d derives another head", what, r);
      for (int p = 0; p < n; p++)
        CHECK(hr.len[p] == h.len[p] && hr.bytepair[p] == h.bytepair[p], "%s: rank %d derives another block %d", what, r, p);
    }
  }
  CHECK(rc0 == MX_SUCCESS, "%s: verdict %d", what, rc0);
  if (rc0) return;
  // buffers: sources random, destinations the fill
  const bool gather = S.kind == RK_GATHER;
  const size_t sbig = (size_t)ORG + kRoom, big = (size_t)ORG + (size_t)(n + 1) * kRoom;
  for (int p = 0; p < n; p++) {
    S.sbuf[p].assign(sbig, FILL);
    S.swr[p].assign(sbig, 0);
    if (gather)
      for (auto &v : S.sbuf[p]) v = (uint8_t)rng();
    S.stage[p].assign(S.main_bytes, 0);
    S.stage_writer[p].assign(S.main_bytes, -1);
  }
  S.mbuf.assign(big, FILL);
  S.mwr.assign(big, 0);
  if (!gather)
    for (auto &v : S.mbuf) v = (uint8_t)rng();
  // the brute-force result
  std::vector<uint8_t> exp_m = S.mbuf, exp_wr_m(big, 0);
  std::vector<std::vector<uint8_t>> exp_s(n), exp_wr_s(n);
  const RRow &T = S.rows[S.root];
  for (int p = 0; p < n; p++) {
    exp_s[p] = S.sbuf[p];
    exp_wr_s[p].assign(sbig, 0);
    uint64_t len = std::min(S.scount[p] * S.single[p].size, S.mcount[p] * S.multi.size);
    if (p == S.root && S.inplace) len = 0;
    CHECK(len == h.len[p], "%s: block %d moves %llu bytes, brute force %llu", what, p, (unsigned long long)h.len[p],
          (unsigned long long)len);
    const std::vector<int64_t> ws = walk(S.single[p].l, len), wm = walk(S.multi.l, len);
    for (uint64_t b = 0; b < len; b++) {
      const size_t a = (size_t)(ORG + ws[b]), m = (size_t)(ORG + T.moffs[p] + wm[b]);
      if (gather) { exp_m[m] = S.sbuf[p][a]; exp_wr_m[m]++; }
      else { exp_s[p][a] = S.mbuf[m]; exp_wr_s[p][a]++; }
    }
  }
  std::vector<RJob> jobs;
  if (mode == MODE_LOCAL) {
    rooted_local_jobs(h, S.rows, jobs);
    run_jobs(S, h, 0, jobs, 0, 0, false);
  } else if (mode == MODE_ZC) {
    for (int r = 0; r < n; r++) {
      rooted_zc_jobs(h, S.rows, r, jobs);
      run_jobs(S, h, r, jobs, rooted_zc_ready_mask(h, r), 0, true);
      // the owner of a buffer that is read waits for its readers
      for (const RJob &j : jobs) {
        const int owner = j.s.buf == RB_MULTI ? h.root : j.s.rank;
        if (owner != r)
          CHECK((rooted_zc_pushed_mask(h, owner) >> r) & 1, "%s: rank %d does not wait for its reader %d", what, owner, r);
      }
    }
  } else {
    RGeom g;
    const bool ok = rooted_geom(S.main_bytes, n, S.kind, h.max_block, &g);
    CHECK(ok, "%s: no staging geometry", what);
    if (!ok) return;
    const size_t cap = gather ? ((S.main_bytes / (size_t)n) & ~(size_t)255) - 256 : (S.main_bytes & ~(size_t)255) - 256;
    CHECK(g.cap == cap && g.rounds == (h.max_block + cap - 1) / cap, "%s: %llu rounds of %zu bytes, formula %llu of %zu",
          what, (unsigned long long)g.rounds, g.cap, (unsigned long long)((h.max_block + cap - 1) / cap), cap);
    for (uint64_t q = 0; q < g.rounds; q++) {
      for (int p = 0; p < n; p++) std::fill(S.stage_writer[p].begin(), S.stage_writer[p].end(), -1);
      for (int phase = 0; phase < 2; phase++)
        for (int r = 0; r < n; r++) {
          rooted_staged_jobs(h, S.rows, g, r, q, phase, jobs);
          run_jobs(S, h, r, jobs, phase ? rooted_staged_ready_mask(h, g, r, q) : 0,
                   phase ? 0 : rooted_staged_done_mask(h, g, r, q), true);
        }
    }
  }
  CHECK(S.mbuf == exp_m, "%s: the multi side differs from the brute-force walk", what);
  CHECK(S.mwr == exp_wr_m, "%s: a multi-side byte was not written exactly once (or a gap byte was)", what);
  for (int p = 0; p < n; p++) {
    CHECK(S.sbuf[p] == exp_s[p], "%s: rank %d's single side differs from the brute-force walk", what, p);
    CHECK(S.swr[p] == exp_wr_s[p], "%s: a byte of rank %d's single side was not written exactly once", what, p);
  }
}

// a random call: the single sides may differ rank by rank (the asymmetric case)
static void random_sim(Sim &S, int n, int kind, int root, bool v, bool inplace, bool bytes_only, size_t main_bytes) {
  S.n = n;
  S.kind = kind;
  S.root = root;
  S.inplace = inplace;
  S.main_bytes = main_bytes;
  const bool gather = kind == RK_GATHER;
  auto pick = [&](bool receive) {
    for (;;) {
      const Shape &s = kShapes[bytes_only ? 0 : rnd(0, kNShapes - 1)];
      if (!receive || s.recv_ok) return s;
    }
  };
  S.multi = pick(gather);
  const bool mflat = xlay_is_flat(S.multi.l);
  const uint64_t block = bytes_only ? rnd(1, 5000) : 288 * rnd(1, 12);   // lcm of the instance sizes
  int64_t at = 0;
  S.maddr = 0x1000000 + (bytes_only ? rnd(0, 15) : 0);
  std::vector<int> order(n);
  for (int p = 0; p < n; p++) order[p] = p;
  if (v) std::shuffle(order.begin(), order.end(), rng);   // displacements in non-rank order
  const uint64_t grain = mflat && !bytes_only ? 4 : 1;   // a flat side against a strided one: whole words
  for (int p = 0; p < n; p++) {
    S.single[p] = pick(!gather);
    S.saddr[p] = 0x2000000 + (uintptr_t)p * 0x100000 + (bytes_only ? rnd(0, 15) : 0);
    uint64_t bytes = block;
    if (v) bytes = rnd(0, 3) ? 288 * rnd(0, 10) : 0;
    if (v && bytes_only) bytes = rnd(0, 4000);
    S.scount[p] = bytes / S.single[p].size;
    S.mcount[p] = bytes / S.multi.size;
    if (v && rnd(0, 4) == 0 && S.mcount[p] > 3 * grain) S.mcount[p] -= 3 * grain;   // less room / a shorter announcement
    if (v && rnd(0, 4) == 0) S.mcount[p] += 5 * grain;
  }
  for (int k = 0; k < n; k++) {
    const int p = order[k];
    if (v) at += (int64_t)(rnd(0, 3) * grain);   // gaps
    S.mdispl[p] = at;
    at += (int64_t)S.mcount[p];
  }
}

static void verdict_cases() {
  Sim S;
  random_sim(S, 3, RK_GATHER, 1, false, false, false, 1 << 20);
  S.multi = kShapes[2];
  for (int p = 0; p < 3; p++) { S.single[p] = kShapes[0]; S.scount[p] = 288; S.mcount[p] = 12; S.mdispl[p] = 12 * p; }
  make_rows(S);
  RHead h;
  auto every_rank = [&](int want, const char *what) {
    for (int r = 0; r < S.n; r++) {
      std::vector<RRow> copy(S.rows, S.rows + S.n);
      CHECK(rooted_verdict(copy.data(), S.n, 0, &h) == want, "%s as rank %d sees it", what, r);
    }
  };
  every_rank(MX_SUCCESS, "flat into vec");
  CHECK(rooted_verdict(S.rows, 3, 3 * 288, &h) == MX_ERR_UNSUPPORTED, "at the exchange minimum");
  CHECK(rooted_verdict(S.rows, 3, 3 * 288 - 1, &h) == MX_SUCCESS, "above the exchange minimum");
  S.rows[2].h.verdict = 0;                        // MX_DDT_NONE on a non-root
  every_rank(MX_ERR_UNSUPPORTED, "a rank that cannot take part");
  S.rows[2].h.verdict = 1;
  S.rows[0].h.root = 2;                           // a mismatched root
  every_rank(MX_ERR_ARG, "a mismatched root");
  S.rows[0].h.root = 1;
  S.rows[0].h.kind = RK_SCATTER;
  every_rank(MX_ERR_ARG, "gather against scatter");
  S.rows[0].h.kind = RK_GATHER;
  const XLay b2s4{0, 2, 4, 4, 16};                // 2-byte blocks: the word would be 2
  S.rows[0].h.lay = b2s4;
  S.rows[0].h.unit = xlay_unit(b2s4, 0x1000);
  every_rank(MX_ERR_UNSUPPORTED, "b2s4 against a strided partner");
  S.rows[1].h.mlay = xlay_flat();
  every_rank(MX_ERR_UNSUPPORTED, "b2s4 against a flat partner");
  S.rows[0].h.lay = xlay_flat();
  S.rows[0].h.unit = 1;                           // an odd address: flat to flat has no word rule
  every_rank(MX_SUCCESS, "odd bytes into bytes");
  for (int p = 0; p < 3; p++) S.rows[p].h.root = 3;
  every_rank(MX_ERR_ARG, "root out of range");
}

int main() {
  static Sim S;
  const int sizes[] = {1, 2, 3, 5, 16};
  int sims = 0;
  for (int n : sizes)
    for (int kind = 0; kind < 2; kind++)
      for (int rep = 0; rep < (n == 16 ? 4 : 10); rep++) {
        const int root = rep % n;
        const bool v = rep & 1, inplace = rep % 5 == 3, bytes_only = rep % 4 == 2;
        char what[128];
        // stagings of one round, and small ones that cut blocks into three and more rounds
        const size_t stagings[] = {(size_t)1 << 20, (size_t)n * 1280, (size_t)n * 768 + 256};
        for (int mode = 0; mode < (n == 1 ? 1 : 3); mode++)
          for (size_t st = 0; st < (mode == MODE_STAGED ? 3 : 1); st++) {
            random_sim(S, n, kind, root, v, inplace && mode != MODE_ZC, bytes_only, stagings[st]);
            snprintf(what, sizeof what, "n=%d %s root=%d %s%s%s mode=%d staging=%zu", n, kind ? "scatter" : "gather", root,
                     v ? "v " : "", inplace ? "inplace " : "", bytes_only ? "bytes" : "", mode, stagings[st]);
            simulate(S, mode, what);
            sims++;
          }
      }
  verdict_cases();
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("rooted_check: %d simulated calls ok\n", sims);
  return 0;
}
