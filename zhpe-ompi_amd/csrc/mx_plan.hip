// mx_plan.hip -- host-only planning of reduction orders (mx_plan.hpp): the
// fold partitions, topologies and expression DAGs that restate the
// reference's algorithms, the DAG compiler, and the decision functions.  No
// HIP API, no communicator, no launch.
#include <string.h>
#include <algorithm>

#include "mx_plan.hpp"

namespace mx {

// ---------------------------------------------------------------------------
// fold partitions: which tree each element gets (restating the reference)
// ---------------------------------------------------------------------------
// COLL_BASE_COMPUTE_BLOCKCOUNT (coll_base_functions.h:428-435)
void blockcount(size_t count, int nblocks, size_t *off, size_t *len) {
  const size_t late = count / nblocks, split = count % nblocks, early = late + (split ? 1 : 0);
  for (int b = 0; b < nblocks; b++) {
    off[b] = (size_t)b < split ? b * early : b * late + split;
    len[b] = (size_t)b < split ? early : late;
  }
}

static int ilog2(int v) { int d = 0; while ((1 << (d + 1)) <= v) d++; return d; }

static uint32_t bitrev(uint32_t v, int D) {
  uint32_t r = 0;
  for (int i = 0; i < D; i++) if (v & (1u << i)) r |= 1u << (D - 1 - i);
  return r;
}

static FoldProg chain(int n, int start, int step, bool acc_first) {
  FoldProg p;
  memset(&p, 0, sizeof p);
  p.kind = PROG_CHAIN;
  p.n = n;
  p.acc_first = acc_first;
  for (int j = 0; j < n; j++) p.ord[j] = (int8_t)(((start + step * j) % n + n) % n);
  return p;
}

// Butterfly over p' = 2^D virtual ranks.  asc: level s combines on bit s
// (recursive doubling / Rabenseifner: mask = 1, 2, 4, ...); !asc: level s
// combines on bit D-1-s (recursive halving: mask = p'/2, ..., 1).  pref: bit
// b set -> the side with bit b = 1 is the target at the level splitting b.
// Leaves: v < extra -> pair (2v, 2v+1) with the odd one first iff first_odd,
// else real rank v + extra.
static FoldProg butterfly(int n, bool asc, uint32_t pref, bool first_odd) {
  FoldProg p;
  memset(&p, 0, sizeof p);
  const int D = ilog2(n), P = 1 << D, extra = n - P;
  p.kind = PROG_BFLY;
  p.n = P;
  p.D = D;
  p.pref = asc ? pref : bitrev(pref, D);
  for (int i = 0; i < P; i++) {
    const int v = asc ? i : (int)bitrev(i, D);  // slot i holds leaf v
    if (v < extra) {
      p.la[i] = (int8_t)(first_odd ? 2 * v + 1 : 2 * v);
      p.lb[i] = (int8_t)(first_odd ? 2 * v : 2 * v + 1);
    } else {
      p.la[i] = (int8_t)(v + extra);
      p.lb[i] = -1;
    }
  }
  return p;
}

static void push_clip(std::vector<Seg> &out, size_t lo, size_t hi, size_t rlo, size_t rhi, const FoldProg &p) {
  const size_t a = std::max(lo, rlo), b = std::min(hi, rhi);
  if (a < b) out.push_back(Seg{a, b, p});
}

// Allreduce fold segments restricted to [rlo, rhi).
int allreduce_segments(int alg, int n, size_t count, size_t es, size_t rlo, size_t rhi,
                       std::vector<Seg> &out) {
  if (alg == kArNbcRing) {
    // segments of ceil(count/p) elements (the last ones short or empty,
    // :648-661); segment b is first sent by rank b-1 from its sendbuf
    // (round 0: element r+1 goes to r+1), then every rank reduces
    // recvbuf = own OP recvbuf (:796-799) -> acc is the target
    const size_t seg = (count + n - 1) / n;
    for (int b = 0; b < n; b++) {
      const size_t lo = std::min(count, (size_t)b * seg), hi = std::min(count, lo + seg);
      push_clip(out, lo, hi, rlo, rhi, chain(n, b - 1, +1, true));
    }
    return MX_SUCCESS;
  }
  if (alg == MX_ALLREDUCE_AUTO) alg = mx_allreduce_decision(n, count, -(int)es);
  if (alg == MX_ALLREDUCE_RING || alg == MX_ALLREDUCE_SEGMENTED_RING) {
    if (count < (size_t)n) alg = MX_ALLREDUCE_RECURSIVE_DOUBLING;  // :371-377 (segmented -> ring -> RD)
  }
  if (alg == MX_ALLREDUCE_RABENSEIFNER) {
    const int P = 1 << ilog2(n);
    if (count < (size_t)P) alg = MX_ALLREDUCE_BASIC_LINEAR;       // :988-995
  }
  switch (alg) {
    case MX_ALLREDUCE_RING:
    case MX_ALLREDUCE_SEGMENTED_RING: {
      // block b folds x_b, then OP(x_{b+1}, acc), ... (:407-482); segmenting
      // into phases (:702-811) only subdivides the blocks.
      size_t off[MAXR], len[MAXR];
      blockcount(count, n, off, len);
      for (int b = 0; b < n; b++) push_clip(out, off[b], off[b] + len[b], rlo, rhi, chain(n, b, +1, false));
      return MX_SUCCESS;
    }
    case MX_ALLREDUCE_RECURSIVE_DOUBLING:
      // every level computes OP(high, low) (:227-236); odd leaves of the
      // non-power-of-two fold compute OP(x_odd, x_even) (:191-193)
      push_clip(out, 0, count, rlo, rhi, butterfly(n, true, 0xffffffffu, true));
      return MX_SUCCESS;
    case MX_ALLREDUCE_BASIC_LINEAR:
      // reduce_intra_basic_linear: rbuf = x_{n-1}; rbuf = OP(rbuf, x_i), i = n-2..0
      push_clip(out, 0, count, rlo, rhi, chain(n, n - 1, -1, true));
      return MX_SUCCESS;
    case MX_ALLREDUCE_RABENSEIFNER: {
      // final window of each virtual rank from recursive halving
      // (:1110-1160): at mask m the lower rank keeps floor(w/2) on the left
      const int D = ilog2(n), P = 1 << D, rem = n - P;
      const size_t lhalf = count / 2;
      for (int v = 0; v < P; v++) {
        size_t lo = 0, w = count;
        for (int s = 0; s < D; s++) {
          const size_t left = w / 2;
          if (v & (1 << s)) { lo += left; w -= left; } else { w = left; }
        }
        // leaves of the non-power-of-two fold: left half OP(x_even, x_odd),
        // right half OP(x_odd, x_even) (:1050-1092)
        if (rem > 0) {
          push_clip(out, lo, std::min(lo + w, lhalf), rlo, rhi, butterfly(n, true, (uint32_t)v, false));
          push_clip(out, std::max(lo, lhalf), lo + w, rlo, rhi, butterfly(n, true, (uint32_t)v, true));
        } else {
          push_clip(out, lo, lo + w, rlo, rhi, butterfly(n, true, (uint32_t)v, false));
        }
      }
      std::sort(out.begin(), out.end(), [](const Seg &a, const Seg &b) { return a.lo < b.lo; });
      return MX_SUCCESS;
    }
    default:
      return MX_ERR_UNSUPPORTED;
  }
}

// Reduce-scatter fold segments for output block `blk` (elements relative to
// the full vector).
int reduce_scatter_segments(int alg, int n, const size_t *rcounts, size_t es, int blk,
                            std::vector<Seg> &out) {
  size_t total = 0, disp[MAXR];
  for (int i = 0; i < n; i++) { disp[i] = total; total += rcounts[i]; }
  if (alg == MX_RS_AUTO) alg = mx_reduce_scatter_decision(n, total, -(int)es);
  const size_t lo = disp[blk], hi = disp[blk] + rcounts[blk];
  if (alg == MX_RS_RING) {
    // block b starts at rank b+1 and ends at rank b (:520-604)
    push_clip(out, lo, hi, lo, hi, chain(n, blk + 1, +1, false));
    return MX_SUCCESS;
  }
  if (alg == MX_RS_RECURSIVE_HALVING) {
    // owner virtual rank of block blk (tmp_rcounts, :205-216); every level
    // computes OP(own, received) with masks p'/2 .. 1 (:218-290); leaves
    // of the non-power-of-two fold: odd rank computes OP(x_odd, x_even)
    const int D = ilog2(n), P = 1 << D, rem = n - P;
    int v = blk < 2 * rem ? blk / 2 : blk - rem;
    (void)P;
    push_clip(out, lo, hi, lo, hi, butterfly(n, false, (uint32_t)v, true));
    return MX_SUCCESS;
  }
  if (alg == MX_RS_BUTTERFLY) {
    // coll_base_reduce_scatter.c:691-880: masks 1, 2, 4, ... (ascending);
    // at every level the lower virtual rank's partial is the source and the
    // higher one's the target (vrank < vpeer: precv = psend OP precv, else
    // psend = precv OP psend, :833-845), whichever rank keeps the block;
    // the non-power-of-two leaves fold the even rank's vector into the odd
    // one's (:772-776).  Per element that is the recursive-doubling tree.
    push_clip(out, lo, hi, lo, hi, butterfly(n, true, 0xffffffffu, true));
    return MX_SUCCESS;
  }
  return MX_ERR_UNSUPPORTED;
}

// Program: EMITs of bare contributions first, then each needed node in
// creation order (children precede parents) followed by its EMITs.
// Registers: contribution j starts in r_j; a register is released after its
// last use and reused by the next definition.
int dag_compile(const Dag &g, int owner, VmProg &p) {
  const int n = g.n, m = (int)g.node.size(), tot = n + m;
  // need[i]: bit 0 = needed when the info bit is set, bit 1 = when clear
  std::vector<int> need(tot, 0);
  for (const auto &o : g.out) need[o.e] |= o.guard == VM_IF_SET ? 1 : o.guard == VM_IF_CLEAR ? 2 : 3;
  for (int i = tot - 1; i >= n; i--)
    if (need[i]) {
      need[g.node[i - n].first] |= need[i];
      need[g.node[i - n].second] |= need[i];
    }
  auto guard_of = [](int nd) { return nd == 1 ? (int)VM_IF_SET : nd == 2 ? (int)VM_IF_CLEAR : 0; };
  struct Ins { int op, d, a, b, guard; };
  std::vector<Ins> seq;
  for (const auto &o : g.out)
    if (o.e < n) seq.push_back({VM_EMIT, o.dst < 0 ? owner : o.dst, o.e, -1, o.guard});
  for (int i = n; i < tot; i++) {
    if (!need[i]) continue;
    seq.push_back({VM_COMB, i, g.node[i - n].first, g.node[i - n].second, guard_of(need[i])});
    for (const auto &o : g.out)
      if (o.e == i) seq.push_back({VM_EMIT, o.dst < 0 ? owner : o.dst, i, -1, o.guard});
  }
  if ((int)seq.size() > VM_MAXI) return MX_ERR_UNSUPPORTED;
  std::vector<int> last(tot, -1);
  for (int k = 0; k < (int)seq.size(); k++) {
    last[seq[k].a] = k;
    if (seq[k].op == VM_COMB) last[seq[k].b] = k;
  }
  // registers: contribution j starts in r_j; a register is released after
  // its last use (in program order -- guarded-out instructions only skip
  // values nothing live depends on) and reused by the next definition
  std::vector<int> reg(tot, -1), free_regs;
  int nregs = n;
  for (int j = 0; j < n; j++) reg[j] = j;
  memset(&p, 0, sizeof p);
  p.nsrc = n;
  for (int k = 0; k < (int)seq.size(); k++) {
    const Ins &q = seq[k];
    VmIns &o = p.ins[p.nins++];
    o.op = (int8_t)(q.op | q.guard);
    o.a = (int8_t)reg[q.a];
    if (q.op == VM_EMIT) {
      o.d = (int8_t)q.d;
      o.b = 0;
      if (last[q.a] == k) free_regs.push_back(reg[q.a]);
      continue;
    }
    o.b = (int8_t)reg[q.b];
    if (last[q.a] == k) free_regs.push_back(reg[q.a]);   // operands are read before the result is written
    if (last[q.b] == k && q.b != q.a) free_regs.push_back(reg[q.b]);
    int r;
    if (!free_regs.empty()) {
      r = free_regs.back();
      free_regs.pop_back();
    } else {
      r = nregs++;
    }
    reg[q.d] = r;
    o.d = (int8_t)r;
  }
  p.nregs = nregs;
  return nregs > VM_MAXREG ? MX_ERR_UNSUPPORTED : MX_SUCCESS;
}

// ---- topology builders (ompi/mca/coll/base/coll_base_topo.c) -------------
static int t_pown(int fanout, int num) {           // pown (:34-46)
  if (num < 0) return 0;
  if (num == 1) return fanout;
  int p = 1;
  for (int j = 0; j < num; j++) p *= fanout;
  return p;
}
static int t_level(int fanout, int rank) {         // calculate_level (:48-56)
  int level, num;
  if (rank < 0) return -1;
  for (level = 0, num = 0; num <= rank; level++) num += t_pown(fanout, level);
  return level - 1;
}
// ompi_coll_base_topo_build_tree (:78-175): children of `rank`, in order
static std::vector<int> topo_tree(int fanout, int n, int root, int rank) {
  std::vector<int> ch;
  if (n < 2) return ch;
  int sr = rank - root;
  if (sr < 0) sr += n;
  const int level = t_level(fanout, sr), delta = t_pown(fanout, level);
  for (int i = 0; i < fanout; i++) {
    const int sc = sr + delta * (i + 1);
    if (sc < n) ch.push_back((sc + root) % n);
    else break;
  }
  return ch;
}
// ompi_coll_base_topo_build_in_order_bmtree (:403-458)
static std::vector<int> topo_in_order_bmtree(int n, int root, int rank) {
  std::vector<int> ch;
  const int vrank = (rank - root + n) % n;
  for (int mask = 1; mask < n; mask <<= 1) {
    const int remote = vrank ^ mask;
    if (remote < vrank) break;
    if (remote < n) ch.push_back((remote + root) % n);
  }
  return ch;
}
// ompi_coll_base_topo_build_chain (:531-673)
static std::vector<int> topo_chain(int fanout, int n, int root, int rank) {
  std::vector<int> ch;
  if (fanout < 1) fanout = 1;
  if (fanout > 32) fanout = 32;                    // MAXTREEFANOUT
  if (n - 1 < fanout) fanout = n - 1;
  const int srank = (rank - root + n) % n;
  if (fanout == 1) {
    if (srank + 1 < n) ch.push_back((srank + 1 + root) % n);
    return ch;
  }
  if (n == 1 || fanout < 1) return ch;
  int maxchainlen = (n - 1) / fanout, mark;
  if ((n - 1) % fanout != 0) {
    maxchainlen++;
    mark = (n - 1) % fanout;
  } else {
    mark = fanout + 1;
  }
  if (srank != 0) {
    int head, len;
    if (srank - 1 < mark * maxchainlen) {
      const int column = (srank - 1) / maxchainlen;
      head = 1 + column * maxchainlen;
      len = maxchainlen;
    } else {
      const int column = mark + (srank - 1 - mark * maxchainlen) / (maxchainlen - 1);
      head = mark * maxchainlen + 1 + (column - mark) * (maxchainlen - 1);
      len = maxchainlen - 1;
    }
    if (srank != head + len - 1 && srank + 1 < n) ch.push_back((srank + 1 + root) % n);
  } else {
    int prev = (root + 1) % n;
    ch.push_back(prev);
    for (int i = 1; i < fanout; i++) {
      int nx = prev + maxchainlen;
      if (i > mark) nx--;
      nx %= n;
      ch.push_back(nx);
      prev = nx;
    }
  }
  return ch;
}
// ompi_coll_base_topo_build_in_order_bintree (:192-295); root is n - 1
static std::vector<int> topo_in_order_bintree(int n, int rank) {
  int size = n, myrank = rank, parent = n - 1, delta = 0, next0 = -1, next1 = -1;
  while (true) {
    const int rightsize = size >> 1;
    int lchild = -1, rchild = -1;
    if (size - 1 > 0) {
      lchild = parent - 1;
      if (lchild > 0) rchild = rightsize - 1;
    }
    if (myrank == parent) {
      if (lchild >= 0) next0 = lchild + delta;
      if (rchild >= 0) next1 = rchild + delta;
      break;
    }
    if (myrank > rchild) {
      size = size - rightsize - 1;
      delta = delta + rightsize;
      myrank = myrank - rightsize;
      parent = size - 1;
    } else {
      size = rightsize;
      parent = rchild;
    }
  }
  std::vector<int> ch;
  if (next0 >= 0) ch.push_back(next0);
  if (next1 >= 0) ch.push_back(next1);
  return ch;
}

// ompi_coll_base_reduce_generic (coll_base_reduce.c:143-240), commutative
// op: a node folds its first child's partial result with its own data
// (child = target, :159-172 + :196-205), then every further child onto that
// accumulator; the root with MPI_IN_PLACE keeps its own data as the target.
template <class CH>
static int reduce_generic_expr(Dag &g, int v, int root, bool root_inplace, const CH &children, int depth) {
  if (depth > g.n) return -1;   // malformed tree
  const std::vector<int> ch = children(v);
  if (ch.empty()) return v;
  int acc;
  size_t i0;
  if (v == root && root_inplace) { acc = v; i0 = 0; }
  else {
    const int c0 = reduce_generic_expr(g, ch[0], root, root_inplace, children, depth + 1);
    if (c0 < 0) return -1;
    acc = g.comb(c0, v);
    i0 = 1;
  }
  for (size_t i = i0; i < ch.size(); i++) {
    const int ci = reduce_generic_expr(g, ch[i], root, root_inplace, children, depth + 1);
    if (ci < 0) return -1;
    acc = g.comb(acc, ci);
  }
  return acc;
}

// The fold expression of MPI_Reduce(root) under algorithm `alg`
// (coll_tuned_reduce_decision.c:36-45 numbering).
static int reduce_expr(Dag &g, int alg, int root, bool root_inplace, int fanout = MX_REDUCE_CHAIN_FANOUT) {
  const int n = g.n;
  switch (alg) {
    case MX_REDUCE_LINEAR: {           // basic_linear (:699-722): rbuf = x_{n-1}; rbuf op= x_i
      int acc = n - 1;
      for (int i = n - 2; i >= 0; i--) acc = g.comb(acc, i);
      return acc;
    }
    case MX_REDUCE_CHAIN:
      return reduce_generic_expr(g, root, root, root_inplace,
                                 [&](int v) { return topo_chain(fanout, n, root, v); }, 0);
    case MX_REDUCE_PIPELINE:
      return reduce_generic_expr(g, root, root, root_inplace, [&](int v) { return topo_chain(1, n, root, v); }, 0);
    case MX_REDUCE_BINARY:
      return reduce_generic_expr(g, root, root, root_inplace, [&](int v) { return topo_tree(2, n, root, v); }, 0);
    case MX_REDUCE_BINOMIAL:
      return reduce_generic_expr(g, root, root, root_inplace,
                                 [&](int v) { return topo_in_order_bmtree(n, root, v); }, 0);
    case MX_REDUCE_IN_ORDER_BINARY: {
      // reduce_intra_in_order_binary (:509-605): generic over the in-order
      // binary tree rooted at n-1; the real root's MPI_IN_PLACE data is
      // copied to a temporary unless n-1 is the root
      const int io_root = n - 1;
      return reduce_generic_expr(g, io_root, io_root, root_inplace && io_root == root,
                                 [&](int v) { return topo_in_order_bintree(n, v); }, 0);
    }
    default:
      return -2;
  }
}

// root_inplace: 0 no, 1 yes, 2 unknown here (multi-process part owners):
// both variants, guarded by the root's info bit, sharing every subtree
// `word`: MX_REDUCE_* in the low byte, the chain fanout in bits 16-23
// (MX_ALG_WORD; 0 = MX_REDUCE_CHAIN_FANOUT)
int reduce_dag(Dag &g, int word, size_t count, size_t es, int root, int root_inplace) {
  int alg = word & 0xff;
  const int fanout = ((word >> 16) & 0xff) ? ((word >> 16) & 0xff) : MX_REDUCE_CHAIN_FANOUT;
  if (alg == MX_REDUCE_AUTO) alg = mx_reduce_decision(g.n, count, -(int)es);
  if (g.n == 1) {
    g.emit(0, root);
    return MX_SUCCESS;
  }
  const int e1 = root_inplace != 0 ? reduce_expr(g, alg, root, true, fanout) : -3;
  const int e0 = root_inplace != 1 ? reduce_expr(g, alg, root, false, fanout) : -3;
  if (e1 == -2 || e0 == -2) return MX_ERR_UNSUPPORTED;
  if (e1 == -1 || e0 == -1) return MX_ERR_ARG;
  if (root_inplace == 1) g.emit(e1, root);
  else if (root_inplace == 0 || e0 == e1) g.emit(e0, root);
  else {
    g.emit(e1, root, VM_IF_SET);
    g.emit(e0, root, VM_IF_CLEAR);
  }
  return MX_SUCCESS;
}

// MPI_Scan: linear (coll_base_scan.c:35-122; coll/basic's scan) and
// recursive doubling (:157-230, commutative branch).
int scan_dag(Dag &g, int alg, bool exclusive) {
  const int n = g.n;
  if (alg == MX_SCAN_AUTO) alg = MX_SCAN_LINEAR;   // tuned has no fixed scan/exscan: coll/basic (linear)
  if (alg == MX_SCAN_LINEAR) {
    if (!exclusive) {                 // rbuf_r = x_r; rbuf_r op= rbuf_{r-1} (target = own data)
      int acc = 0;
      g.emit(0, 0);
      for (int r = 1; r < n; r++) {
        acc = g.comb(r, acc);
        g.emit(acc, r);
      }
    } else if (n > 1) {               // exscan linear (coll_base_exscan.c:35-107)
      int acc = 0;                    // rank 1 receives x_0
      g.emit(0, 1);
      for (int r = 2; r < n; r++) {   // rank r-1 sends reduce_buffer = x_{r-1} op rbuf_{r-1}
        acc = g.comb(r - 1, acc);
        g.emit(acc, r);
      }
    }
    return MX_SUCCESS;
  }
  if (alg != MX_SCAN_RECURSIVE_DOUBLING) return MX_ERR_UNSUPPORTED;
  std::vector<int> rbuf(n), psend(n), prev(n);
  std::vector<char> first(n, 1);
  for (int r = 0; r < n; r++) rbuf[r] = psend[r] = r;
  for (int mask = 1; mask < n; mask <<= 1) {
    prev = psend;                     // sendrecv: every rank sends its psend before reducing
    for (int r = 0; r < n; r++) {
      const int remote = r ^ mask;
      if (remote >= n) continue;
      const int precv = prev[remote];
      if (r > remote) {
        if (exclusive && first[r]) { rbuf[r] = precv; first[r] = 0; }   // exscan :191-195
        else rbuf[r] = g.comb(rbuf[r], precv);                          // recvbuf = precv op recvbuf
      }
      psend[r] = g.comb(psend[r], precv);                               // psend = precv op psend
    }
  }
  for (int r = exclusive ? 1 : 0; r < n; r++) g.emit(rbuf[r], r);
  return MX_SUCCESS;
}

// OpenSHMEM scoll/basic reduce, its default algorithm (recursive doubling,
// mca_scoll_basic_param_reduce_algorithm, scoll_basic_component.c:35;
// _algorithm_recursive_doubling, scoll_basic_reduce.c:374-542): floor2 = the
// largest power of two <= n; PE r + floor2 (an "extra") puts its source to
// PE r, which folds it first; then floor2 - 1 pairwise rounds, PE r with
// r ^ (1 << round), each PE folding the partner's current value into its
// own; every PE keeps its own result and hands it to its extra.  Every fold
// is op->o_func.c_fn(in = received, out = target_cur) = *out = calc(*out,
// *in) (oshmem/op/op.c:165-178): COMB(target = own, source = received),
// the MPI op functions' operand roles, so the op kernels evaluate it.  For
// MAX / MIN with NaNs or signed zeros the two PEs of a pair can end with
// different values (each is the target of its own fold), so every PE gets
// its own tree.
int shmem_basic_rd_dag(Dag &g) {
  const int n = g.n;
  int floor2 = 1;
  for (int i = n >> 1; i; i >>= 1) floor2 <<= 1;
  std::vector<int> cur(n);
  for (int r = 0; r < n; r++) cur[r] = r;
  for (int r = 0; r + floor2 < n; r++) cur[r] = g.comb(cur[r], r + floor2);
  for (int round = 0, exit_flag = floor2 - 1; exit_flag; exit_flag >>= 1, round++) {
    std::vector<int> next(cur);
    for (int r = 0; r < floor2; r++) next[r] = g.comb(cur[r], cur[r ^ (1 << round)]);
    cur.swap(next);
  }
  for (int r = 0; r < n; r++) g.emit(cur[r < floor2 ? r : r - floor2], r);
  return MX_SUCCESS;
}

uint32_t dest_mask_of(const Dag &g, int owner_rank) {
  uint32_t m = 0;
  for (const auto &o : g.out) m |= 1u << (o.dst < 0 ? owner_rank : o.dst);
  return m;
}

// libnbc's binomial reduction in virtual ranks (0 <-> vroot swapped,
// RANK2VRANK nbc_iallreduce.c:353-364): round r = 1..ceil(log2 p), v with
// v % 2^r == 0 receives the partial result of v + 2^(r-1) and computes
// recv = own OP recv (NBC_Sched_op(sendbuf|lbuf, rbuf), :401-409).
int nbc_binomial_expr(Dag &g, int vroot) {
  const int n = g.n;
  auto real = [&](int v) { return v == 0 ? vroot : v == vroot ? 0 : v; };
  std::vector<int> acc(n);
  for (int v = 0; v < n; v++) acc[v] = real(v);
  int maxr = 0;
  while ((1 << maxr) < n) maxr++;
  for (int r = 1; r <= maxr; r++)
    for (int v = 0; v < n; v += 1 << r) {
      const int vp = v + (1 << (r - 1));
      if (vp < n) acc[v] = g.comb(acc[vp], acc[v]);
    }
  return acc[0];
}

// red_sched_chain (nbc_ireduce.c:461-536): virtual ranks (0 <-> root); v = p-1
// sends its data down the chain, every v computes acc = own OP acc (:500-503);
// the root with MPI_IN_PLACE reduces recvbuf = acc OP own (:497-499).
int nbc_chain_expr(Dag &g, int root, bool root_inplace) {
  const int n = g.n;
  auto real = [&](int v) { return v == 0 ? root : v == root ? 0 : v; };
  int acc = real(n - 1);
  for (int v = n - 2; v >= 1; v--) acc = g.comb(acc, real(v));
  return root_inplace ? g.comb(root, acc) : g.comb(acc, root);
}

// The expression a fold program evaluates (eval_prog, mx_fold.hpp).
int fold_expr(Dag &g, const FoldProg &p) {
  if (p.kind == PROG_CHAIN) {
    int acc = p.ord[0];
    for (int j = 1; j < p.n; j++) acc = p.acc_first ? g.comb(acc, p.ord[j]) : g.comb(p.ord[j], acc);
    return acc;
  }
  std::vector<int> R(p.n);
  for (int i = 0; i < p.n; i++) R[i] = p.lb[i] >= 0 ? g.comb(p.la[i], p.lb[i]) : p.la[i];
  for (int s = 0; s < p.D; s++) {
    const int h = 1 << s;
    const bool hi_first = (p.pref >> s) & 1;
    for (int u = 0; u < p.n; u += 2 << s) R[u] = hi_first ? g.comb(R[u + h], R[u]) : g.comb(R[u], R[u + h]);
  }
  return R[0];
}

int pof2_le(int n) { return 1 << ilog2(n); }

}  // namespace mx

using namespace mx;

extern "C" int mx_allreduce_decision(int n, size_t count, int type) {
  // ompi_coll_tuned_allreduce_intra_dec_fixed (coll_tuned_decision_fixed.c:44-95);
  // every predefined op is commutative.  type < 0 passes -element_size.
  const size_t es = type < 0 ? (size_t)(-type) : type_size(type);
  const size_t block_dsize = es * count;
  if (n <= 1) return MX_ALLREDUCE_RING;
  if (block_dsize < 10000) return MX_ALLREDUCE_RECURSIVE_DOUBLING;
  if (count > (size_t)n) {
    const size_t segment_size = 1 << 20;
    return (size_t)n * segment_size >= block_dsize ? MX_ALLREDUCE_RING : MX_ALLREDUCE_SEGMENTED_RING;
  }
  return MX_ALLREDUCE_NONOVERLAPPING;
}

extern "C" int mx_reduce_scatter_decision(int n, size_t total_count, int type) {
  // ompi_coll_tuned_reduce_scatter_intra_dec_fixed (:466-512)
  const size_t es = type < 0 ? (size_t)(-type) : type_size(type);
  const double a = 0.0012, b = 8.0;
  const size_t small_message_size = 12 * 1024, large_message_size = 256 * 1024;
  const size_t total = total_count * es;
  int pow2 = 1;
  while (pow2 < n) pow2 <<= 1;
  if (total <= small_message_size || (total <= large_message_size && pow2 == n) ||
      (double)n >= a * (double)total + b)
    return MX_RS_RECURSIVE_HALVING;
  return MX_RS_RING;
}

extern "C" int mx_reduce_decision(int n, size_t count, int type) {
  // ompi_coll_tuned_reduce_intra_dec_fixed (coll_tuned_decision_fixed.c:354-429),
  // commutative ops (every predefined MPI_Op)
  const size_t es = type < 0 ? (size_t)(-type) : type_size(type);
  const double a1 = 0.6016 / 1024.0, b1 = 1.3496, a2 = 0.0410 / 1024.0, b2 = 9.7128;
  const double a3 = 0.0422 / 1024.0, b3 = 1.1614;
  const size_t message_size = es * count;
  const double ms = (double)message_size, cs = (double)n;
  if (n < 8 && message_size < 512) return MX_REDUCE_LINEAR;
  if ((n < 8 && message_size < 20480) || message_size < 2048 || count <= 1) return MX_REDUCE_BINOMIAL;
  if (cs > a1 * ms + b1) return MX_REDUCE_BINOMIAL;
  if (cs > a2 * ms + b2) return MX_REDUCE_PIPELINE;
  if (cs > a3 * ms + b3) return MX_REDUCE_BINARY;
  return MX_REDUCE_PIPELINE;
}

extern "C" int mx_iallreduce_decision(int n, size_t count, int type, int inplace) {
  // nbc_allreduce_init (nbc_iallreduce.c:113-121), commutative ops
  const size_t es = type < 0 ? (size_t)(-type) : type_size(type);
  if (n < 4 || es * count < 65536 || inplace) return MX_IALLREDUCE_BINOMIAL;
  if (count >= (size_t)pof2_le(n)) return MX_IALLREDUCE_RABENSEIFNER;
  return MX_IALLREDUCE_RING;
}

extern "C" int mx_ireduce_decision(int n, size_t count, int type) {
  // nbc_reduce_init (nbc_ireduce.c:107-116), commutative ops
  const size_t es = type < 0 ? (size_t)(-type) : type_size(type);
  if (n > 2 && count >= (size_t)pof2_le(n)) return MX_IREDUCE_RABENSEIFNER;
  if (n > 4 || es * count < 65536) return MX_IREDUCE_BINOMIAL;
  return MX_IREDUCE_CHAIN;
}
