// mx_exchange_plan.hip -- host-only planning for the exchange kernel
// (mx_exchange_plan.hpp): job and prefix tables, launch split, staging
// rounds, argument checks.  No HIP API, no communicator, no launch.
#include <algorithm>

#include "mx_exchange_plan.hpp"

namespace mx {

uint64_t xplan_tables(const uint64_t *nb, size_t J, uint64_t max_grid_blocks, std::vector<XSeg> &seg,
                      std::vector<XLaunch> &launch) {
  seg.resize(J + 1);
  launch.clear();
  uint64_t blocks = 0, round = 0;
  for (size_t i = 0; i < J; i++) {
    seg[i] = XSeg{blocks, round};
    blocks += (nb[i] - round) * (uint64_t)(J - i);   // rounds [round, nb[i]) hold the jobs i..J-1
    round = nb[i];
  }
  seg[J] = XSeg{blocks, round};
  for (uint64_t b = 0; b < blocks; b += max_grid_blocks)
    launch.push_back(XLaunch{b, (uint32_t)std::min<uint64_t>(max_grid_blocks, blocks - b)});
  return blocks;
}

int xplan_build(const XJob *jobs, size_t n, XPlan &out, uint64_t max_grid_blocks) {
  out = XPlan();
  if (n > (size_t)kXMaxJobs || (n && !jobs) || !max_grid_blocks) return MX_ERR_ARG;
  if (max_grid_blocks > kXMaxGridBlocks) max_grid_blocks = kXMaxGridBlocks;
  for (size_t i = 0; i < n; i++) {
    if (!jobs[i].bytes) continue;   // zero-byte jobs never reach the device
    if (!jobs[i].src || !jobs[i].dst) return MX_ERR_ARG;
    out.jobs.push_back(jobs[i]);
    out.bytes += jobs[i].bytes;
  }
  std::stable_sort(out.jobs.begin(), out.jobs.end(), [](const XJob &a, const XJob &b) {
    return xjob_blocks((uintptr_t)a.dst, a.bytes) < xjob_blocks((uintptr_t)b.dst, b.bytes);
  });
  std::vector<uint64_t> nb(out.jobs.size());
  for (size_t i = 0; i < nb.size(); i++) nb[i] = xjob_blocks((uintptr_t)out.jobs[i].dst, out.jobs[i].bytes);
  out.nblocks = xplan_tables(nb.data(), nb.size(), max_grid_blocks, out.seg, out.launch);
  return MX_SUCCESS;
}

bool xstage_slots(size_t main_bytes, int n, size_t *slot, size_t *cap) {
  if (n < 1) return false;
  *slot = (main_bytes / (size_t)n) & ~(size_t)255;
  if (*slot < 512) return false;
  *cap = *slot - 256;
  return true;
}

int xcheck_row(int n, const size_t *bytes, const size_t *offs) {
  if (n < 1 || n > MX_MAX_RANKS || !bytes || !offs) return MX_ERR_ARG;
  for (int p = 0; p < n; p++)
    if (offs[p] + bytes[p] < offs[p]) return MX_ERR_ARG;
  return MX_SUCCESS;
}

bool xranges_disjoint(int n, const size_t *bytes, const size_t *offs) {
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++)
      if (bytes[a] && bytes[b] && offs[a] < offs[b] + bytes[b] && offs[b] < offs[a] + bytes[a]) return false;
  return true;
}

}  // namespace mx
