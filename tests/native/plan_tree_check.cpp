// plan_tree_check.cpp -- host check that the planning unit (csrc/mx_plan.hip)
// plans the oracle's trees.  plan_check.cpp proves the shape of every plan;
// this program proves the order: for 2..MX_MAX_RANKS ranks, every root, in
// place and not, every element of every rank's result must carry, tree for
// tree, the reduction the collective oracle (oracle/mx_oracle_coll.c, symbolic
// mode) performs.  A tree is (target source), the roles of Dag::comb.  Every
// DAG is also compiled for every owner and the VM program interpreted as
// k_vm / vm_run (csrc/mx_fold.hpp) run it, with the info bit clear and set.
// Built with the host compiler under sanitizers and linked with the oracle's
// C files (tests/test_plan_tree_host.py); prints the first mismatches and
// exits non-zero.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "mx_plan.hpp"

using namespace mx;

extern "C" {
// the planner is always given -element_size (plan_check.cpp)
size_t mx_type_size(int type) {
  fprintf(stderr, "FAIL: the planner asked for the size of type id %d\n", type);
  abort();
}
void mxo_sym_reset(int on);
int mxo_sym_node(int64_t id, int64_t *target, int64_t *source);
typedef const void *const *cbufs;
typedef void *const *bufs;
int mxo_allreduce(int alg, int op, int type, int n, size_t count, cbufs sb, bufs rb);
int mxo_allreduce_segring(int op, int type, int n, size_t count, bufs rb, size_t segsize);
int mxo_reduce_scatter(int alg, int op, int type, int n, const size_t *rcounts, cbufs sb, bufs rb);
int mxo_reduce(int alg, int op, int type, int n, size_t count, int root, cbufs sb, void *rbuf);
int mxo_scan(int alg, int op, int type, int n, size_t count, cbufs sb, bufs rb);
int mxo_exscan(int alg, int op, int type, int n, size_t count, cbufs sb, bufs rb);
int mxo_reduce_scatter_block(int alg, int op, int type, int n, size_t rcount, cbufs sb, bufs rb);
int mxo_iallreduce(int alg, int op, int type, int n, size_t count, cbufs sb, bufs rb);
int mxo_ireduce(int alg, int op, int type, int n, size_t count, int root, cbufs sb, void *rbuf);
int mxo_ireduce_scatter(int op, int type, int n, const size_t *rcounts, cbufs sb, bufs rb);
int mxo_shmem_basic_reduce(int op, int type, int n, size_t count, cbufs sb, bufs rb);
int mxo_allreduce_decision(int n, size_t count, size_t es);
int mxo_reduce_scatter_decision(int n, size_t total_count, size_t es);
int mxo_reduce_decision(int n, size_t count, size_t es, int *segsize);
int mxo_iallreduce_decision(int n, size_t count, size_t es, int inplace);
int mxo_ireduce_decision(int n, size_t count, size_t es);
}

static const int SUM = MX_OP_SUM, I64 = MX_TYPE_INT64_T;
static const size_t ES = 8;                  // the symbolic element: an int64 expression id
// leaf of (rank, element): -(rank * STRIDE + element + 1); the stride leaves
// room for reduce_scatter_block's rcount * n elements
static const int64_t STRIDE = 1 << 20;
static const int64_t UNSET = INT64_MIN / 2;  // prefill of result buffers: decodes to no rank

static long g_cmp = 0, g_vm = 0, g_dec = 0;
static int g_fail = 0;

static void fail(const char *fmt, ...) {
  if (g_fail++ >= 12) return;
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "MISMATCH ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
}

// ---- canonical trees: ids 0..MAXR-1 are the ranks' contributions ----------
static const int BAD = -1;
static std::vector<std::pair<int, int>> t_node;
static std::map<std::pair<int, int>, int> t_memo;

static int t_comb(int target, int source) {
  if (target < 0 || source < 0) return BAD;
  const auto k = std::make_pair(target, source);
  const auto it = t_memo.find(k);
  if (it != t_memo.end()) return it->second;
  t_node.push_back(k);
  return t_memo[k] = MAXR + (int)t_node.size() - 1;
}
static std::string t_str(int id) {
  if (id < 0) return "?";
  if (id < MAXR) return std::to_string(id);
  return "(" + t_str(t_node[id - MAXR].first) + " " + t_str(t_node[id - MAXR].second) + ")";
}

// the oracle's expression `v` as a canonical tree; BAD if it holds a leaf of
// another element, an unwritten value or an unknown node
static std::unordered_map<int64_t, int> o_memo;
static int o_tree(int64_t v, size_t elem) {
  if (v < 0) {
    const int64_t k = -(v + 1);
    return (k / STRIDE < MAXR && (size_t)(k % STRIDE) == elem) ? (int)(k / STRIDE) : BAD;
  }
  const auto it = o_memo.find(v);
  if (it != o_memo.end()) return it->second;
  int64_t t, s;
  const int id = mxo_sym_node(v, &t, &s) ? BAD : t_comb(o_tree(t, elem), o_tree(s, elem));
  return o_memo[v] = id;
}

// a planner expression as a canonical tree
static int d_tree(const Dag &g, int e) {
  if (e < g.n) return e;
  return t_comb(d_tree(g, g.node[e - g.n].first), d_tree(g, g.node[e - g.n].second));
}

// ---- the n simulated ranks' buffers ----------------------------------------
struct Ranks {
  int n;
  std::vector<std::vector<int64_t>> x, r;   // contributions, results
  const void *sp[MAXR];
  void *rp[MAXR];
  // inplace: the results start as the contributions and sbufs is null
  Ranks(int n_, size_t count, bool inplace, size_t rcount = (size_t)-1) : n(n_), x(n_), r(n_) {
    for (int q = 0; q < n; q++) {
      x[q].resize(count + 1);
      for (size_t e = 0; e < count; e++) x[q][e] = -((int64_t)q * STRIDE + (int64_t)e + 1);
      r[q] = inplace ? x[q] : std::vector<int64_t>((rcount == (size_t)-1 ? count : rcount) + 1, UNSET);
      sp[q] = x[q].data();
      rp[q] = r[q].data();
    }
    o_memo.clear();
    mxo_sym_reset(1);
  }
  ~Ranks() { mxo_sym_reset(0); }
  cbufs sbufs(bool inplace) const { return inplace ? nullptr : sp; }
};

// rank `rank`'s result element at `at` (element `elem` of the vector) against the planned tree
static void expect(const Ranks &R, int rank, size_t at, size_t elem, int want, const char *what, int alg, size_t count,
                   int root, int inplace) {
  g_cmp++;
  const int got = o_tree(R.r[rank][at], elem);
  if (got != want || got == BAD)
    fail("%s alg %d n %d root %d count %zu in-place %d: rank %d element %zu\n  oracle  %s\n  planner %s", what, alg,
         R.n, root, count, inplace, rank, elem, t_str(got).c_str(), t_str(want).c_str());
}

// ---- VM programs, interpreted as vm_run does --------------------------------
// registers 0..nsrc-1 start as the contributions; an instruction whose guard
// the info bit rules out is skipped; COMB r[d] = (r[a] r[b]); EMIT r[a] -> d
static void vm_outputs(const VmProg &p, int info, std::vector<std::pair<int, int>> &out) {
  std::vector<int> R(VM_MAXREG, BAD);
  for (int j = 0; j < p.nsrc; j++) R[j] = j;
  const int skip = info ? VM_IF_CLEAR : VM_IF_SET;
  for (int i = 0; i < p.nins; i++) {
    const VmIns in = p.ins[i];
    if (in.op & skip) continue;
    if ((in.op & 3) == VM_COMB) {
      const int x = R[in.a], y = R[in.b];
      R[in.d] = t_comb(x, y);
    } else {
      out.push_back({in.d, R[in.a]});
    }
  }
}

// for every owner and both info bits: the program emits exactly the DAG's
// outputs that are live under that bit, each with its tree
static void check_vm(const Dag &g, const char *what, int alg, int root) {
  for (int owner = 0; owner < g.n; owner++) {
    VmProg p;
    const int rc = dag_compile(g, owner, p);
    if (rc != MX_SUCCESS) { fail("%s alg %d n %d owner %d: dag_compile %d", what, alg, g.n, owner, rc); continue; }
    for (int info = 0; info < 2; info++) {
      std::vector<std::pair<int, int>> want, got;
      for (const DagOut &o : g.out)
        if (o.guard == 0 || o.guard == (info ? VM_IF_SET : VM_IF_CLEAR))
          want.push_back({o.dst < 0 ? owner : o.dst, d_tree(g, o.e)});
      vm_outputs(p, info, got);
      std::sort(want.begin(), want.end());
      std::sort(got.begin(), got.end());
      g_vm += (long)want.size();
      if (want == got) continue;
      std::string w, q;
      for (const auto &o : want) w += " " + std::to_string(o.first) + ":" + t_str(o.second);
      for (const auto &o : got) q += " " + std::to_string(o.first) + ":" + t_str(o.second);
      fail("VM program of %s alg %d n %d root %d owner %d info %d\n  DAG outputs %s\n  program    %s", what, alg, g.n,
           root, owner, info, w.c_str(), q.c_str());
    }
  }
}

// the per-element trees of fold segments that must tile [lo, hi)
static bool seg_trees(const std::vector<Seg> &segs, int n, size_t lo, size_t hi, std::vector<int> &tree,
                      const char *what, int alg, bool vm) {
  size_t at = lo;
  for (const Seg &s : segs) {
    if (s.lo != at || s.hi <= s.lo || s.hi > hi) break;
    Dag g(n);
    g.emit(fold_expr(g, s.p), n - 1);
    const int t = d_tree(g, g.out[0].e);
    for (size_t e = s.lo; e < s.hi; e++) tree[e] = t;
    if (vm) check_vm(g, what, alg, n - 1);
    at = s.hi;
  }
  if (at != hi && !(lo >= hi && segs.empty())) {
    fail("%s alg %d n %d: segments do not tile [%zu,%zu)", what, alg, n, lo, hi);
    return false;
  }
  return true;
}

// an allreduce-shaped oracle call against per-element trees, on every rank
typedef std::function<int(Ranks &, bool)> oracle_fn;
static void check_all_ranks(const char *what, int alg, int n, size_t count, const std::vector<int> &tree,
                            const oracle_fn &call) {
  for (int inplace = 0; inplace < 2; inplace++) {
    Ranks R(n, count, inplace);
    if (call(R, inplace)) { fail("%s alg %d n %d count %zu: the oracle refused", what, alg, n, count); continue; }
    for (int q = 0; q < n; q++)
      for (size_t e = 0; e < count; e++) expect(R, q, e, e, tree[e], what, alg, count, -1, inplace);
  }
}

// allreduce_segments(alg) over the whole range and over every rank's part
static bool planned_allreduce(int alg, int n, size_t count, std::vector<int> &tree, const char *what, bool vm) {
  tree.assign(count, BAD);
  std::vector<Seg> all;
  if (allreduce_segments(alg, n, count, ES, 0, count, all) != MX_SUCCESS) {
    fail("%s alg %d n %d count %zu: allreduce_segments failed", what, alg, n, count);
    return false;
  }
  if (!seg_trees(all, n, 0, count, tree, what, alg, vm)) return false;
  size_t off[MAXR], len[MAXR];
  blockcount(count, n, off, len);
  for (int p = 0; p < n; p++) {
    std::vector<Seg> part;
    std::vector<int> pt(count, BAD);
    if (allreduce_segments(alg, n, count, ES, off[p], off[p] + len[p], part) != MX_SUCCESS ||
        !seg_trees(part, n, off[p], off[p] + len[p], pt, what, alg, false))
      return false;
    for (size_t e = off[p]; e < off[p] + len[p]; e++) {
      g_cmp++;
      if (pt[e] != tree[e])
        fail("%s alg %d n %d count %zu: part %d element %zu\n  part  %s\n  whole %s", what, alg, n, count, p, e,
             t_str(pt[e]).c_str(), t_str(tree[e]).c_str());
    }
  }
  return true;
}

static void check_decisions(int n) {
  const size_t sizes[] = {1, 4, 8, 16};
  for (size_t es : sizes) {
    std::vector<size_t> counts = {1, (size_t)n - 1, (size_t)n, (size_t)n + 1, 4 * (size_t)n + 3,
                                  (size_t)pof2_le(n) - 1, (size_t)pof2_le(n)};
    // the two sides of every byte threshold of the five rules
    for (size_t bytes : {512u, 2048u, 10000u, 12u * 1024, 20480u, 65536u, 256u * 1024, 1u << 20})
      for (size_t mul : {(size_t)1, (size_t)n})
        for (long d = -1; d <= 1; d++) counts.push_back((size_t)((long)(bytes * mul / es) + d));
    for (size_t c : counts) {
      if (c == 0) continue;
      const int t = -(int)es;
      for (int inplace = 0; inplace < 2; inplace++) {
        g_dec++;
        if (mx_iallreduce_decision(n, c, t, inplace) != mxo_iallreduce_decision(n, c, es, inplace))
          fail("iallreduce decision n %d count %zu es %zu in-place %d: %d, oracle %d", n, c, es, inplace,
               mx_iallreduce_decision(n, c, t, inplace), mxo_iallreduce_decision(n, c, es, inplace));
      }
      g_dec += 4;
      if (mx_ireduce_decision(n, c, t) != mxo_ireduce_decision(n, c, es))
        fail("ireduce decision n %d count %zu es %zu: %d, oracle %d", n, c, es, mx_ireduce_decision(n, c, t),
             mxo_ireduce_decision(n, c, es));
      if (mx_allreduce_decision(n, c, t) != mxo_allreduce_decision(n, c, es))
        fail("allreduce decision n %d count %zu es %zu: %d, oracle %d", n, c, es, mx_allreduce_decision(n, c, t),
             mxo_allreduce_decision(n, c, es));
      if (mx_reduce_decision(n, c, t) != mxo_reduce_decision(n, c, es, nullptr))
        fail("reduce decision n %d count %zu es %zu: %d, oracle %d", n, c, es, mx_reduce_decision(n, c, t),
             mxo_reduce_decision(n, c, es, nullptr));
      if (mx_reduce_scatter_decision(n, c, t) != mxo_reduce_scatter_decision(n, c, es))
        fail("reduce_scatter decision n %d total %zu es %zu: %d, oracle %d", n, c, es,
             mx_reduce_scatter_decision(n, c, t), mxo_reduce_scatter_decision(n, c, es));
    }
  }
}

// a rooted oracle call (mxo_reduce / mxo_ireduce) against one tree for every element
typedef int (*rooted_fn)(int, int, int, int, size_t, int, cbufs, void *);
static void check_rooted(const char *what, rooted_fn fn, int alg, int n, size_t count, int root, int inplace,
                         const std::vector<int> &tree) {
  Ranks R(n, count, false);
  if (inplace) { R.r[root] = R.x[root]; R.rp[root] = R.r[root].data(); R.sp[root] = nullptr; }
  if (fn(alg, SUM, I64, n, count, root, R.sp, R.rp[root])) { fail("%s alg %d n %d: the oracle refused", what, alg, n); return; }
  for (size_t e = 0; e < count; e++) expect(R, root, e, e, tree[e], what, alg, count, root, inplace);
}

int main() {
  size_t split_phases = 0;
  for (int n = 2; n <= MX_MAX_RANKS; n++) {
    check_decisions(n);
    const size_t counts[5] = {1, (size_t)n - 1, (size_t)n, (size_t)n + 1, 4 * (size_t)n + 3};
    for (size_t count : counts) {
      // VM programs are interpreted at the two ends of the counts: at 1 the
      // ring and Rabenseifner plans are their small-count fallbacks (recursive
      // doubling, basic linear), at 4n + 3 they are the ring chains and the
      // Rabenseifner butterflies themselves; the DAGs in between repeat these
      const bool vm = count == counts[0] || count == counts[4];
      std::vector<int> tree;
      // ---- allreduce: tuned 1, 3-6 and AUTO ---------------------------------
      for (int alg : {(int)MX_ALLREDUCE_AUTO, (int)MX_ALLREDUCE_BASIC_LINEAR, (int)MX_ALLREDUCE_RECURSIVE_DOUBLING,
                      (int)MX_ALLREDUCE_RING, (int)MX_ALLREDUCE_SEGMENTED_RING, (int)MX_ALLREDUCE_RABENSEIFNER}) {
        if (!planned_allreduce(alg, n, count, tree, "allreduce", vm)) continue;
        check_all_ranks("allreduce", alg, n, count, tree, [&](Ranks &R, bool ip) {
          return mxo_allreduce(alg, SUM, I64, n, count, R.sbufs(ip), R.rp);
        });
      }
      // ---- segmented ring at segment sizes of 1-3 elements: the phases ------
      if (planned_allreduce(MX_ALLREDUCE_SEGMENTED_RING, n, count, tree, "allreduce segmented ring", false))
        for (size_t segcount = 1; segcount <= 3; segcount++) {
          if (count >= (size_t)n * segcount && count / ((size_t)n * segcount) >= 2) split_phases++;
          Ranks R(n, count, true);
          if (mxo_allreduce_segring(SUM, I64, n, count, R.rp, segcount * ES)) { fail("segring refused"); continue; }
          for (int q = 0; q < n; q++)
            for (size_t e = 0; e < count; e++) expect(R, q, e, e, tree[e], "allreduce segmented ring", (int)segcount, count, -1, 1);
        }
      // ---- allreduce NONOVERLAPPING: a rooted reduce to rank 0, then a bcast
      for (int ra = MX_REDUCE_AUTO; ra <= MX_REDUCE_IN_ORDER_BINARY; ra++)
        for (int fo : {0, 2}) {
          if (fo && ra != MX_REDUCE_CHAIN) continue;
          const int word = MX_ALG_WORD(MX_ALLREDUCE_NONOVERLAPPING, ra, fo);
          for (int inplace = 0; inplace < 2; inplace++) {
            Dag g(n);
            if (reduce_dag(g, reduce_word_of(word), count, ES, 0, inplace) != MX_SUCCESS || g.out.size() != 1) {
              fail("allreduce nonoverlapping word %#x n %d: reduce_dag", word, n);
              continue;
            }
            if (vm || ra == MX_REDUCE_AUTO) check_vm(g, "allreduce nonoverlapping", word, 0);
            const int t = d_tree(g, g.out[0].e);
            Ranks R(n, count, inplace);
            if (mxo_allreduce(word, SUM, I64, n, count, R.sbufs(inplace), R.rp)) { fail("nonoverlapping refused"); continue; }
            for (int q = 0; q < n; q++)
              for (size_t e = 0; e < count; e++) expect(R, q, e, e, t, "allreduce nonoverlapping", word, count, 0, inplace);
          }
        }
      // ---- libnbc iallreduce: ring, Rabenseifner (ring below pof2), recursive
      // doubling as nbc_allreduce plans them; binomial to rank 0 -----------------
      const struct { int nbc, plan; } iar[] = {
          {MX_IALLREDUCE_RING, kArNbcRing},
          {MX_IALLREDUCE_RABENSEIFNER, count >= (size_t)pof2_le(n) ? (int)MX_ALLREDUCE_RABENSEIFNER : kArNbcRing},
          {MX_IALLREDUCE_RECURSIVE_DOUBLING, MX_ALLREDUCE_RECURSIVE_DOUBLING}};
      for (const auto &a : iar) {
        if (!planned_allreduce(a.plan, n, count, tree, "iallreduce", vm)) continue;
        check_all_ranks("iallreduce", a.nbc, n, count, tree, [&](Ranks &R, bool ip) {
          return mxo_iallreduce(a.nbc, SUM, I64, n, count, R.sbufs(ip), R.rp);
        });
      }
      {
        Dag g(n);
        const int e = nbc_binomial_expr(g, 0);
        for (int d = 0; d < n; d++) g.emit(e, d);
        if (vm) check_vm(g, "iallreduce binomial", MX_IALLREDUCE_BINOMIAL, 0);
        tree.assign(count, d_tree(g, e));
        check_all_ranks("iallreduce binomial", MX_IALLREDUCE_BINOMIAL, n, count, tree, [&](Ranks &R, bool ip) {
          return mxo_iallreduce(MX_IALLREDUCE_BINOMIAL, SUM, I64, n, count, R.sbufs(ip), R.rp);
        });
      }
      // ---- reduce_scatter and ireduce_scatter: ragged counts with zeros ------
      size_t rc[MAXR], disp[MAXR], total = 0;
      for (int i = 0; i < n; i++) rc[i] = (i % 3 == 1) ? 0 : count / n + (size_t)(i % 4);
      rc[n - 1] += count % n;
      for (int i = 0; i < n; i++) { disp[i] = total; total += rc[i]; }
      for (int alg : {(int)MX_RS_AUTO, (int)MX_RS_RECURSIVE_HALVING, (int)MX_RS_RING, (int)MX_RS_BUTTERFLY}) {
        tree.assign(total, BAD);
        bool ok = true;
        for (int blk = 0; blk < n && ok; blk++) {
          std::vector<Seg> segs;
          ok = reduce_scatter_segments(alg, n, rc, ES, blk, segs) == MX_SUCCESS &&
               seg_trees(segs, n, disp[blk], disp[blk] + rc[blk], tree, "reduce_scatter", alg, vm);
        }
        if (!ok) { fail("reduce_scatter alg %d n %d count %zu: no plan", alg, n, count); continue; }
        for (int inplace = 0; inplace < 2; inplace++) {
          Ranks R(n, total, inplace);
          if (mxo_reduce_scatter(alg, SUM, I64, n, rc, R.sbufs(inplace), R.rp)) { fail("reduce_scatter refused"); continue; }
          for (int q = 0; q < n; q++)
            for (size_t i = 0; i < rc[q]; i++) expect(R, q, i, disp[q] + i, tree[disp[q] + i], "reduce_scatter", alg, total, -1, inplace);
        }
      }
      {
        Dag g(n);
        g.emit(nbc_binomial_expr(g, 0), -1);
        if (vm) check_vm(g, "ireduce_scatter", 0, 0);
        const int t = d_tree(g, g.out[0].e);
        for (int inplace = 0; inplace < 2 && total; inplace++) {
          Ranks R(n, total, inplace);
          if (mxo_ireduce_scatter(SUM, I64, n, rc, R.sbufs(inplace), R.rp)) { fail("ireduce_scatter refused"); continue; }
          for (int q = 0; q < n; q++)
            for (size_t i = 0; i < rc[q]; i++) expect(R, q, i, disp[q] + i, t, "ireduce_scatter", 0, total, -1, inplace);
        }
      }
      // ---- rooted reduce 1-6 and AUTO (and a chain of fanout 2), every root --
      for (int root = 0; root < n; root++) {
        for (int word : {(int)MX_REDUCE_AUTO, (int)MX_REDUCE_LINEAR, (int)MX_REDUCE_CHAIN, (int)MX_REDUCE_PIPELINE,
                         (int)MX_REDUCE_BINARY, (int)MX_REDUCE_BINOMIAL, (int)MX_REDUCE_IN_ORDER_BINARY,
                         MX_REDUCE_CHAIN | (2 << 16)}) {
          int variant[2] = {BAD, BAD};
          for (int inplace = 0; inplace < 2; inplace++) {
            Dag g(n);
            if (reduce_dag(g, word, count, ES, root, inplace) != MX_SUCCESS || g.out.size() != 1 || g.out[0].dst != root) {
              fail("reduce word %#x n %d root %d: reduce_dag", word, n, root);
              continue;
            }
            if (vm || word == MX_REDUCE_AUTO) check_vm(g, "reduce", word, root);
            variant[inplace] = d_tree(g, g.out[0].e);
            tree.assign(count, variant[inplace]);
            check_rooted("reduce", mxo_reduce, word, n, count, root, inplace, tree);
          }
          // what the part owners of a multi-process reduce run: both variants, guarded
          Dag g2(n);
          if (reduce_dag(g2, word, count, ES, root, 2) != MX_SUCCESS) { fail("reduce word %#x: guarded reduce_dag", word); continue; }
          if (vm || word == MX_REDUCE_AUTO) check_vm(g2, "reduce (guarded)", word, root);
          for (int info = 0; info < 2; info++) {
            int live = 0;
            for (const DagOut &o : g2.out)
              if (o.guard == 0 || o.guard == (info ? VM_IF_SET : VM_IF_CLEAR)) {
                live++;
                g_cmp++;
                if (d_tree(g2, o.e) != variant[info] || o.dst != root)
                  fail("reduce (guarded) word %#x n %d root %d info %d\n  guarded %s\n  variant %s", word, n, root, info,
                       t_str(d_tree(g2, o.e)).c_str(), t_str(variant[info]).c_str());
              }
            if (live != 1) fail("reduce (guarded) word %#x n %d root %d info %d: %d live outputs", word, n, root, info, live);
          }
        }
        // ---- libnbc ireduce: binomial, chain (two guarded outputs, as
        // nbc_reduce emits them), Rabenseifner (chain below pof2 or at n = 2) --
        {
          Dag g(n);
          g.emit(nbc_binomial_expr(g, root), root);
          if (vm) check_vm(g, "ireduce binomial", MX_IREDUCE_BINOMIAL, root);
          tree.assign(count, d_tree(g, g.out[0].e));
          for (int inplace = 0; inplace < 2; inplace++)
            check_rooted("ireduce binomial", mxo_ireduce, MX_IREDUCE_BINOMIAL, n, count, root, inplace, tree);
        }
        Dag c(n);
        const int e1 = nbc_chain_expr(c, root, true), e0 = nbc_chain_expr(c, root, false);
        c.emit(e1, root, VM_IF_SET);
        c.emit(e0, root, VM_IF_CLEAR);
        if (vm) check_vm(c, "ireduce chain", MX_IREDUCE_CHAIN, root);
        const bool rab = n > 2 && count >= (size_t)pof2_le(n);
        std::vector<int> rtree;
        if (rab && !planned_allreduce(MX_ALLREDUCE_RABENSEIFNER, n, count, rtree, "ireduce rabenseifner", false)) continue;
        if (rab && vm) {   // one program per segment, its output to the root, as nbc_reduce emits them
          std::vector<Seg> fs;
          allreduce_segments(MX_ALLREDUCE_RABENSEIFNER, n, count, ES, 0, count, fs);
          for (const Seg &f : fs) {
            Dag g(n);
            g.emit(fold_expr(g, f.p), root);
            check_vm(g, "ireduce rabenseifner", MX_IREDUCE_RABENSEIFNER, root);
          }
        }
        for (int inplace = 0; inplace < 2; inplace++) {
          tree.assign(count, d_tree(c, inplace ? e1 : e0));
          check_rooted("ireduce chain", mxo_ireduce, MX_IREDUCE_CHAIN, n, count, root, inplace, tree);
          check_rooted("ireduce rabenseifner", mxo_ireduce, MX_IREDUCE_RABENSEIFNER, n, count, root, inplace,
                       rab ? rtree : tree);
        }
      }
      // ---- reduce_scatter_block: the rooted DAG of rcount * n elements to
      // rank 0, its output going to each block's owner --------------------------
      for (int alg = MX_REDUCE_AUTO; alg <= MX_REDUCE_IN_ORDER_BINARY; alg++) {
        Dag g(n);
        if (reduce_dag(g, alg, count * n, ES, 0, 0) != MX_SUCCESS || g.out.size() != 1) { fail("reduce_scatter_block alg %d: reduce_dag", alg); continue; }
        g.out.back().dst = -1;
        if (vm || alg == MX_REDUCE_AUTO) check_vm(g, "reduce_scatter_block", alg, 0);
        const int t = d_tree(g, g.out[0].e);
        for (int inplace = 0; inplace < 2; inplace++) {
          Ranks R(n, count * n, inplace, count);
          if (mxo_reduce_scatter_block(alg, SUM, I64, n, count, R.sbufs(inplace), R.rp)) { fail("reduce_scatter_block refused"); continue; }
          for (int q = 0; q < n; q++)
            for (size_t i = 0; i < count; i++) expect(R, q, i, q * count + i, t, "reduce_scatter_block", alg, count, 0, inplace);
        }
      }
      // ---- scan / exscan ------------------------------------------------------
      for (int alg : {(int)MX_SCAN_AUTO, (int)MX_SCAN_LINEAR, (int)MX_SCAN_RECURSIVE_DOUBLING})
        for (int excl = 0; excl < 2; excl++) {
          Dag g(n);
          if (scan_dag(g, alg, excl != 0) != MX_SUCCESS) { fail("scan alg %d n %d: scan_dag", alg, n); continue; }
          if (vm) check_vm(g, excl ? "exscan" : "scan", alg, -1);
          if ((int)g.out.size() != n - excl) fail("scan alg %d n %d exclusive %d: %zu outputs", alg, n, excl, g.out.size());
          for (int inplace = 0; inplace < 2; inplace++) {
            Ranks R(n, count, inplace);
            if ((excl ? mxo_exscan : mxo_scan)(alg, SUM, I64, n, count, R.sbufs(inplace), R.rp)) { fail("scan refused"); continue; }
            for (const DagOut &o : g.out)
              for (size_t e = 0; e < count; e++)
                expect(R, o.dst, e, e, d_tree(g, o.e), excl ? "exscan" : "scan", alg, count, -1, inplace);
          }
        }
      // ---- OpenSHMEM scoll/basic recursive doubling -----------------------------
      {
        Dag g(n);
        if (shmem_basic_rd_dag(g) != MX_SUCCESS || (int)g.out.size() != n) { fail("shmem recursive doubling n %d", n); continue; }
        if (vm) check_vm(g, "shmem recursive doubling", 0, -1);
        for (int inplace = 0; inplace < 2; inplace++) {
          Ranks R(n, count, inplace);
          if (mxo_shmem_basic_reduce(SUM, I64, n, count, R.sbufs(inplace), R.rp)) { fail("shmem refused"); continue; }
          for (const DagOut &o : g.out)
            for (size_t e = 0; e < count; e++) expect(R, o.dst, e, e, d_tree(g, o.e), "shmem recursive doubling", 0, count, -1, inplace);
        }
      }
    }
  }
  if (split_phases == 0) { fail("no segmented-ring case split into phases"); }
  printf("plan_tree_check: %ld tree comparisons, %ld VM outputs, %ld decisions, %zu segmented-ring cases in phases, %d mismatches\n",
         g_cmp, g_vm, g_dec, split_phases, g_fail);
  return g_fail ? 1 : 0;
}
