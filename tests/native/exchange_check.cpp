// exchange_check.cpp -- host check of the exchange planner
// (csrc/mx_exchange_plan.hip): for 1..MX_MAX_RANKS ranks and random ragged
// n x n size matrices (zeros included) the plan's block counts sum to its
// grids, every byte of every job is moved by exactly one block, consecutive
// blocks go to different jobs while more than one job has blocks left, the
// staging rounds tile every pair, and no grid reaches 2^32 threads.  No
// pointer of a job is ever dereferenced.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>

#include "mx_exchange_plan.hpp"

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

static void check_plan(const std::vector<XJob> &in, uint64_t max_grid, bool cover, const char *what) {
  XPlan p;
  CHECK(xplan_build(in.data(), in.size(), p, max_grid) == MX_SUCCESS, "%s", what);
  size_t nonempty = 0, bytes = 0;
  for (const XJob &j : in) { nonempty += j.bytes != 0; bytes += j.bytes; }
  CHECK(p.jobs.size() == nonempty, "%s: %zu jobs kept of %zu non-empty", what, p.jobs.size(), nonempty);
  CHECK(p.bytes == bytes, "%s: bytes", what);
  CHECK(p.seg.size() == p.jobs.size() + 1, "%s: segments", what);
  // block counts sum to the grid, launches tile the blocks, grids fit HIP
  uint64_t sum = 0;
  std::vector<uint64_t> nb(p.jobs.size());
  for (size_t i = 0; i < p.jobs.size(); i++) {
    CHECK(p.jobs[i].bytes != 0, "%s: empty job kept", what);
    nb[i] = xjob_blocks((uintptr_t)p.jobs[i].dst, p.jobs[i].bytes);
    CHECK(i == 0 || nb[i - 1] <= nb[i], "%s: jobs not in block order", what);
    sum += nb[i];
  }
  CHECK(sum == p.nblocks && p.seg.back().block0 == sum, "%s: %llu blocks planned, %llu in the jobs", what,
        (unsigned long long)p.nblocks, (unsigned long long)sum);
  uint64_t at = 0;
  for (const XLaunch &l : p.launch) {
    CHECK(l.block0 == at && l.nblocks > 0, "%s: launch does not continue the last", what);
    CHECK((uint64_t)l.nblocks * kXThreads < ((uint64_t)1 << 32), "%s: grid of %u blocks", what, l.nblocks);
    CHECK(l.nblocks <= max_grid, "%s: grid above the split", what);
    at += l.nblocks;
  }
  CHECK(at == sum, "%s: launches cover %llu of %llu blocks", what, (unsigned long long)at, (unsigned long long)sum);
  if (!cover) return;
  // every byte once; neighbours differ while more than one job is alive
  std::vector<std::vector<uint8_t>> seen(p.jobs.size());
  for (size_t i = 0; i < p.jobs.size(); i++) seen[i].assign(p.jobs[i].bytes, 0);
  std::vector<uint64_t> got(p.jobs.size(), 0);
  uint32_t pj = 0;
  for (uint64_t b = 0; b < sum; b++) {
    uint32_t j = 0;
    uint64_t k = 0;
    xplan_lookup(p.seg.data(), (uint32_t)p.jobs.size(), b, &j, &k);
    CHECK(j < p.jobs.size() && k < nb[j], "%s: block %llu -> job %u block %llu", what, (unsigned long long)b, j,
          (unsigned long long)k);
    if (j >= p.jobs.size() || k >= nb[j]) return;
    CHECK(k == got[j], "%s: job %u gets block %llu after %llu", what, j, (unsigned long long)k,
          (unsigned long long)got[j]);
    got[j]++;
    if (b > 0 && j == pj) {
      size_t alive = 0;   // jobs that still have a block when this one is dealt
      for (size_t i = 0; i < p.jobs.size(); i++) alive += nb[i] > k;
      CHECK(alive == 1, "%s: blocks %llu and %llu both go to job %u, %zu jobs alive", what,
            (unsigned long long)(b - 1), (unsigned long long)b, j, alive);
    }
    pj = j;
    size_t lo, hi;
    xjob_block_range((uintptr_t)p.jobs[j].dst, p.jobs[j].bytes, k, &lo, &hi);
    CHECK(lo < hi && hi <= p.jobs[j].bytes, "%s: empty or wild block", what);
    CHECK(hi - lo <= kXBlockBytes, "%s: block longer than a workgroup moves", what);
    // inner block edges lie on the destination's 16-byte grid
    CHECK(lo == 0 || (((uintptr_t)p.jobs[j].dst + lo) & 15) == 0, "%s: block start off the grid", what);
    for (size_t o = lo; o < hi && o < seen[j].size(); o++) seen[j][o]++;
  }
  for (size_t i = 0; i < p.jobs.size(); i++) {
    CHECK(got[i] == nb[i], "%s: job %zu got %llu of %llu blocks", what, i, (unsigned long long)got[i],
          (unsigned long long)nb[i]);
    for (size_t o = 0; o < seen[i].size(); o++)
      if (seen[i][o] != 1) {
        CHECK(false, "%s: job %zu byte %zu moved %d times", what, i, o, (int)seen[i][o]);
        break;
      }
  }
}

int main() {
  std::mt19937_64 rng(20260107);
  char label[96];
  for (int n = 1; n <= MX_MAX_RANKS; n++)
    for (int rep = 0; rep < 6; rep++) {
      std::vector<XJob> jobs;
      const int zero_row = (int)(rng() % n);
      for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
          size_t bytes;
          switch (rng() % 6) {
            case 0: bytes = 0; break;
            case 1: bytes = 1 + rng() % 40; break;
            case 2: bytes = kXBlockBytes - 20 + rng() % 40; break;       // around one workgroup
            case 3: bytes = kXWaveBytes - 20 + rng() % 40; break;        // around one wave step
            case 4: bytes = rng() % (5 * kXBlockBytes); break;
            default: bytes = rng() % 5000; break;
          }
          if (i == zero_row && rep % 2) bytes = 0;
          // made-up addresses with every misalignment; never dereferenced
          const uintptr_t src = 0x100000000ull + (uintptr_t)(i * n + j) * 0x1000000ull + rng() % 16;
          const uintptr_t dst = 0x900000000ull + (uintptr_t)(j * n + i) * 0x1000000ull + rng() % 16;
          jobs.push_back(XJob{(const char *)src, (char *)dst, bytes});
        }
      snprintf(label, sizeof label, "n=%d rep=%d", n, rep);
      check_plan(jobs, kXMaxGridBlocks, true, label);
      snprintf(label, sizeof label, "n=%d rep=%d split at 7 blocks", n, rep);
      check_plan(jobs, 7, true, label);
    }
  {   // all jobs empty: nothing to launch
    std::vector<XJob> jobs(9, XJob{(const char *)16, (char *)32, 0});
    XPlan p;
    CHECK(xplan_build(jobs.data(), jobs.size(), p) == MX_SUCCESS && p.launch.empty() && p.nblocks == 0, "empty plan");
  }
  {   // tables past 2^32 grid threads are split (sizes only: nothing is touched)
    std::vector<XJob> jobs;
    for (int i = 0; i < 3; i++)
      jobs.push_back(XJob{(const char *)0x1000 + i, (char *)((uintptr_t)(i + 1) << 44) + 5, ((size_t)1 << 40) + 12345 * i});
    jobs.push_back(XJob{(const char *)0x77, (char *)0x99, 3});
    check_plan(jobs, kXMaxGridBlocks, false, "2^40-byte jobs");
    XPlan p;
    xplan_build(jobs.data(), jobs.size(), p);
    CHECK(p.launch.size() > 1, "2^40-byte jobs fit one grid?");
    // spot-check the map at the launch edges
    for (const XLaunch &l : p.launch)
      for (uint64_t b : {l.block0, l.block0 + l.nblocks - 1}) {
        uint32_t j;
        uint64_t k;
        xplan_lookup(p.seg.data(), (uint32_t)p.jobs.size(), b, &j, &k);
        CHECK(j < p.jobs.size() && k < xjob_blocks((uintptr_t)p.jobs[j].dst, p.jobs[j].bytes), "edge block");
      }
  }
  // staging rounds tile every pair without overlap
  for (int rep = 0; rep < 2000; rep++) {
    const size_t cap = 1 + rng() % 70000;
    size_t pair[8], maxp = 0;
    for (size_t &v : pair) {
      v = rng() % 3 == 0 ? 0 : rng() % 300000;
      if (v > maxp) maxp = v;
    }
    const uint64_t R = xrounds(maxp, cap);
    CHECK(R * cap >= maxp && (R == 0 || (R - 1) * cap < maxp), "round count %llu for %zu by %zu",
          (unsigned long long)R, maxp, cap);
    for (size_t v : pair) {
      size_t next = 0;
      for (uint64_t q = 0; q < R; q++) {
        size_t off, len;
        xround_piece(v, cap, q, &off, &len);
        CHECK(len <= cap && off + len <= v, "piece outside its pair");
        CHECK(len == 0 || off == next, "piece %llu of a %zu-byte pair starts at %zu, expected %zu",
              (unsigned long long)q, v, off, next);
        next += len;
      }
      CHECK(next == v, "rounds moved %zu of %zu bytes", next, v);
    }
  }
  {
    size_t slot = 0, cap = 0;
    CHECK(!xstage_slots(1000, 4, &slot, &cap), "tiny staging accepted");
    for (int n = 1; n <= MX_MAX_RANKS; n++) {
      CHECK(xstage_slots(256 << 10, n, &slot, &cap), "256 KiB staging refused");
      CHECK(slot % 256 == 0 && slot * n <= (256 << 10) && cap + 16 <= slot && cap > 0, "slot geometry n=%d", n);
    }
    const size_t b[3] = {4, 0, 8}, o[3] = {0, 2, 4}, bad[3] = {0, 2, 3}, wrap[3] = {0, 0, (size_t)-4};
    CHECK(xcheck_row(3, b, o) == MX_SUCCESS && xcheck_row(3, b, wrap) != MX_SUCCESS, "row check");
    CHECK(xcheck_row(0, b, o) != MX_SUCCESS && xcheck_row(3, nullptr, o) != MX_SUCCESS, "row check arguments");
    CHECK(xranges_disjoint(3, b, o) && !xranges_disjoint(3, b, bad), "disjoint check");
  }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("exchange planner: ok\n");
  return 0;
}
