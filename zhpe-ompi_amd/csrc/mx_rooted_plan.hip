// mx_rooted_plan.hip -- host-only planning of the rooted exchanges
// (mx_rooted_plan.hpp): the verdict over the published rows, the staging
// geometry, the job lists and the wait masks.  No HIP API, no launch.
#include <algorithm>

#include "mx_rooted_plan.hpp"

namespace mx {

int rooted_verdict(const RRow *rows, int n, size_t xmin, RHead *h) {
  if (!rows || !h || n < 1 || n > MX_MAX_RANKS) return MX_ERR_ARG;
  const int root = rows[0].h.root, kind = rows[0].h.kind;
  for (int p = 1; p < n; p++)
    if (rows[p].h.root != root || rows[p].h.kind != kind) return MX_ERR_ARG;
  if (root < 0 || root >= n || (kind != RK_GATHER && kind != RK_SCATTER)) return MX_ERR_ARG;
  for (int p = 0; p < n; p++)
    if (!rows[p].h.verdict) return MX_ERR_UNSUPPORTED;
  const RRow &T = rows[root];
  *h = RHead();
  h->n = n;
  h->root = root;
  h->kind = kind;
  h->inplace = T.h.inplace != 0;
  bool ok = true;
  for (int p = 0; p < n; p++) {
    // the sender announces, the receiver has room: the block is cut at the room
    uint64_t len = std::min(rows[p].h.bytes, T.mbytes[p]);
    if (p == root && h->inplace) len = 0;
    h->len[p] = len;
    h->bytepair[p] = xlay_is_flat(rows[p].h.lay) && xlay_is_flat(T.h.mlay);
    h->max_block = std::max(h->max_block, len);
    if (!len || h->bytepair[p]) continue;
    if (len >= ((uint64_t)1 << (kMagicBits - 1))) return MX_ERR_UNSUPPORTED;
    unsigned W = std::min(rows[p].h.unit, T.h.munit);
    W = xunit_of(xabs(T.moffs[p]), W);
    W = xunit_of(len, W);
    ok = ok && W >= 4;
  }
  if (!ok) return MX_ERR_UNSUPPORTED;
  if (xmin && (uint64_t)n * h->max_block <= xmin) return MX_ERR_UNSUPPORTED;
  return MX_SUCCESS;
}

bool rooted_geom(size_t main_bytes, int n, int kind, uint64_t max_block, RGeom *g) {
  if (!xstage_slots(main_bytes, kind == RK_GATHER ? n : 1, &g->slot, &g->cap)) return false;
  g->rounds = xrounds((size_t)max_block, g->cap);
  return true;
}

namespace {

REnd single_end(const RRow *rows, int p, uint64_t pos) { return REnd{RB_SINGLE, p, 0, rows[p].h.lay, pos}; }
REnd multi_end(const RHead &h, const RRow *rows, int p, uint64_t pos) {
  return REnd{RB_MULTI, h.root, rows[h.root].moffs[p], rows[h.root].h.mlay, pos};
}
REnd stage_end(int owner, size_t off) { return REnd{RB_STAGE, owner, (int64_t)off, xlay_flat(), 0}; }

// A byte pair keeps its source's address mod 16 in the slot, so an aligned
// push stays off the kernel's shift path (a round starts at a multiple of
// 256 of the block); the other pairs start at the slot.
size_t slot_shift(const RHead &h, const RRow *rows, int p) {
  if (!h.bytepair[p]) return 0;
  const RRow &T = rows[h.root];
  if (h.kind == RK_GATHER) return rows[p].h.mis & 15;
  return (size_t)(((uint64_t)T.h.mmis + (uint64_t)T.moffs[p]) & 15);
}

// rank p's block between its single side and its place in the multi side
RJob direct_job(const RHead &h, const RRow *rows, int p) {
  const REnd s = single_end(rows, p, 0), m = multi_end(h, rows, p, 0);
  return h.kind == RK_GATHER ? RJob{s, m, h.len[p], h.bytepair[p]} : RJob{m, s, h.len[p], h.bytepair[p]};
}

size_t piece(const RHead &h, const RGeom &g, int p, uint64_t q, size_t *off) {
  size_t len;
  xround_piece((size_t)h.len[p], g.cap, q, off, &len);
  return len;
}

uint32_t peers_with_piece(const RHead &h, const RGeom &g, uint64_t q) {
  uint32_t m = 0;
  size_t o;
  for (int p = 0; p < h.n; p++)
    if (p != h.root && piece(h, g, p, q, &o)) m |= 1u << p;
  return m;
}

uint32_t peers_with_block(const RHead &h) {
  uint32_t m = 0;
  for (int p = 0; p < h.n; p++)
    if (p != h.root && h.len[p]) m |= 1u << p;
  return m;
}

}  // namespace

void rooted_staged_jobs(const RHead &h, const RRow *rows, const RGeom &g, int rank, uint64_t q, int phase,
                        std::vector<RJob> &out) {
  out.clear();
  const bool root = rank == h.root, gather = h.kind == RK_GATHER;
  size_t o, l;
  if (phase == 0) {
    if (root) {
      if (!gather)   // one launch: every peer's piece into that peer's staging
        for (int p = 0; p < h.n; p++)
          if (p != h.root && (l = piece(h, g, p, q, &o)))
            out.push_back(RJob{multi_end(h, rows, p, o), stage_end(p, slot_shift(h, rows, p)), l, h.bytepair[p]});
      if (q == 0 && h.len[h.root]) out.push_back(direct_job(h, rows, h.root));   // the root's own block moves directly
    } else if (gather && (l = piece(h, g, rank, q, &o))) {
      out.push_back(RJob{single_end(rows, rank, o), stage_end(h.root, (size_t)rank * g.slot + slot_shift(h, rows, rank)),
                         l, h.bytepair[rank]});
    }
    return;
  }
  if (root && gather) {   // one launch for all slots of the round
    for (int p = 0; p < h.n; p++)
      if (p != h.root && (l = piece(h, g, p, q, &o)))
        out.push_back(RJob{stage_end(h.root, (size_t)p * g.slot + slot_shift(h, rows, p)), multi_end(h, rows, p, o), l,
                           h.bytepair[p]});
  } else if (!root && !gather && (l = piece(h, g, rank, q, &o))) {
    out.push_back(RJob{stage_end(rank, slot_shift(h, rows, rank)), single_end(rows, rank, o), l, h.bytepair[rank]});
  }
}

uint32_t rooted_staged_done_mask(const RHead &h, const RGeom &g, int rank, uint64_t q) {
  size_t o;
  if (h.kind == RK_GATHER) return rank != h.root && piece(h, g, rank, q, &o) ? 1u << h.root : 0;
  return rank == h.root ? peers_with_piece(h, g, q) : 0;
}

uint32_t rooted_staged_ready_mask(const RHead &h, const RGeom &g, int rank, uint64_t q) {
  size_t o;
  if (h.kind == RK_GATHER) return rank == h.root ? peers_with_piece(h, g, q) : 0;
  return rank != h.root && piece(h, g, rank, q, &o) ? 1u << h.root : 0;
}

void rooted_zc_jobs(const RHead &h, const RRow *rows, int rank, std::vector<RJob> &out) {
  out.clear();
  if (rank == h.root) {
    if (h.kind == RK_GATHER)
      for (int p = 0; p < h.n; p++)
        if (p != h.root && h.len[p]) out.push_back(direct_job(h, rows, p));
    if (h.len[h.root]) out.push_back(direct_job(h, rows, h.root));
  } else if (h.kind == RK_SCATTER && h.len[rank]) {
    out.push_back(direct_job(h, rows, rank));
  }
}

uint32_t rooted_zc_ready_mask(const RHead &h, int rank) {
  if (h.kind == RK_GATHER) return rank == h.root ? peers_with_block(h) : 0;
  return rank != h.root && h.len[rank] ? 1u << h.root : 0;
}

uint32_t rooted_zc_pushed_mask(const RHead &h, int rank) {
  if (h.kind == RK_GATHER) return rank != h.root && h.len[rank] ? 1u << h.root : 0;
  return rank == h.root ? peers_with_block(h) : 0;
}

void rooted_local_jobs(const RHead &h, const RRow *rows, std::vector<RJob> &out) {
  out.clear();
  for (int p = 0; p < h.n; p++)
    if (h.len[p]) out.push_back(direct_job(h, rows, p));
}

}  // namespace mx
