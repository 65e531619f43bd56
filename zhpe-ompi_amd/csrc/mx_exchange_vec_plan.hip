// mx_exchange_vec_plan.hip -- host-only planning for the strided exchange
// kernel (mx_exchange_vec_plan.hpp): qualification of a datatype, access
// units, job widths and the block -> job tables.  No HIP API, no launch.
#include <algorithm>

#include "mx_exchange_vec_plan.hpp"

namespace mx {

bool xlay_from(const DdtLayout &L, bool receive_side, XLay *out) {
  if (L.runs.size() != 1 || L.runs[0].cnt2 != 1) return false;
  const DRun &r = L.runs[0];
  if (!r.blen || !r.cnt1 || r.blen > kVecMaxBlen) return false;
  if (receive_side && !L.monotonic) return false;
  const int64_t ext = L.ub - L.lb;
  if (r.cnt1 == 1 && ext == (int64_t)r.blen) *out = xlay_flat(r.disp);
  else *out = XLay{r.disp, r.blen, r.cnt1, r.cnt1 > 1 ? r.stride1 : 0, ext};
  return true;
}

unsigned xlay_unit(const XLay &l, uintptr_t addr) {
  unsigned u = xunit_of(addr);
  u = xunit_of(xabs(l.disp), u);
  if (!xlay_is_flat(l)) {
    u = xunit_of(l.blen, u);
    u = xunit_of(xabs(l.stride1), u);
    u = xunit_of(xabs(l.ext), u);
  }
  return u;
}

int xvjob_make(const char *src, const XLay &sl, uint64_t pos_s, char *dst, const XLay &dl, uint64_t pos_d,
               uint64_t bytes, XVJob *out) {
  const uint64_t lim = (uint64_t)1 << kMagicBits;
  if (pos_s >= lim || pos_d >= lim || bytes >= lim || pos_s + bytes >= lim || pos_d + bytes >= lim) return MX_ERR_ARG;
  XVJob j;
  j.src = src;
  j.dst = dst;
  j.s.l = sl;
  j.d.l = dl;
  for (XSide *sd : {&j.s, &j.d}) {
    const bool flat = xlay_is_flat(sd->l);
    sd->mblen = make_magic(flat ? 1 : sd->l.blen);
    sd->mcnt1 = make_magic(flat ? 1 : sd->l.cnt1);
  }
  j.pos_s = pos_s;
  j.pos_d = pos_d;
  j.bytes = bytes;
  unsigned W = std::min(xlay_unit(sl, (uintptr_t)src), xlay_unit(dl, (uintptr_t)dst));
  W = xunit_of(pos_s, W);
  W = xunit_of(pos_d, W);
  W = xunit_of(bytes, W);
  j.W = W;
  j.pad = 0;
  *out = j;
  return W >= 4 ? MX_SUCCESS : MX_ERR_UNSUPPORTED;
}

int xvplan_build(const XVJob *jobs, size_t n, XVPlan &out, uint64_t max_grid_blocks) {
  out = XVPlan();
  if (n > (size_t)kXMaxJobs || (n && !jobs) || !max_grid_blocks) return MX_ERR_ARG;
  if (max_grid_blocks > kXMaxGridBlocks) max_grid_blocks = kXMaxGridBlocks;
  for (size_t i = 0; i < n; i++) {
    if (!jobs[i].bytes) continue;   // zero-byte jobs never reach the device
    if (!jobs[i].src || !jobs[i].dst) return MX_ERR_ARG;
    const unsigned W = jobs[i].W;
    if ((W != 4 && W != 8 && W != 16) || jobs[i].bytes % W) return MX_ERR_ARG;
    out.jobs.push_back(jobs[i]);
    out.bytes += jobs[i].bytes;
  }
  std::stable_sort(out.jobs.begin(), out.jobs.end(), [](const XVJob &a, const XVJob &b) {
    return xvjob_blocks(a.bytes, a.W) < xvjob_blocks(b.bytes, b.W);
  });
  std::vector<uint64_t> nb(out.jobs.size());
  for (size_t i = 0; i < nb.size(); i++) nb[i] = xvjob_blocks(out.jobs[i].bytes, out.jobs[i].W);
  out.nblocks = xplan_tables(nb.data(), nb.size(), max_grid_blocks, out.seg, out.launch);
  return MX_SUCCESS;
}

}  // namespace mx
