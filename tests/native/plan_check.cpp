// plan_check.cpp -- host check of the planning unit (csrc/mx_plan.hip): walks
// every reduction order the collectives can ask for, for 2..MX_MAX_RANKS
// ranks, and checks the invariants the fold kernels assume.  Built with the
// host compiler under sanitizers (tests/test_plan_host.py); exits non-zero
// on the first violated invariant class, printing every violation.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "mx_plan.hpp"

using namespace mx;

// the decision functions ask for an element size only when given a type id;
// this walk always passes -element_size, so the library's table is not
// needed: a planner that asks for it here fails the check
extern "C" size_t mx_type_size(int type) {
  fprintf(stderr, "FAIL: the planner asked for the size of type id %d\n", type);
  abort();
}

static int g_fail = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (g_fail++ < 40) {                                    \
        fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        fprintf(stderr, __VA_ARGS__);                         \
        fprintf(stderr, "\n");                                \
      }                                                       \
    }                                                         \
  } while (0)

// every contribution 0..n-1 exactly once
static bool is_perm(std::vector<int> v, int n) {
  if ((int)v.size() != n) return false;
  std::sort(v.begin(), v.end());
  for (int i = 0; i < n; i++)
    if (v[i] != i) return false;
  return true;
}

static void check_prog(const FoldProg &p, int n, const char *what, int alg) {
  std::vector<int> leaves;
  if (p.kind == PROG_CHAIN) {
    CHECK(p.n == n, "%s alg %d n %d: chain of %d operands", what, alg, n, p.n);
    for (int j = 0; j < p.n && j < MAXR; j++) leaves.push_back(p.ord[j]);
  } else {
    CHECK(p.kind == PROG_BFLY, "%s alg %d n %d: kind %d", what, alg, n, p.kind);
    CHECK(p.D >= 0 && p.D <= 4 && p.n == 1 << p.D, "%s alg %d n %d: butterfly n %d D %d", what, alg, n, p.n, p.D);
    for (int i = 0; i < p.n && i < MAXR; i++) {
      leaves.push_back(p.la[i]);
      if (p.lb[i] >= 0) leaves.push_back(p.lb[i]);
    }
  }
  CHECK(is_perm(leaves, n), "%s alg %d n %d: the program does not name each contribution once", what, alg, n);
}

// sorted, disjoint, covering [lo, hi) exactly; every program well formed
static void check_segs(const std::vector<Seg> &segs, size_t lo, size_t hi, int n, const char *what, int alg) {
  size_t at = lo;
  for (const Seg &s : segs) {
    CHECK(s.lo == at && s.hi > s.lo && s.hi <= hi, "%s alg %d n %d: segment [%zu,%zu) after %zu in [%zu,%zu)", what,
          alg, n, s.lo, s.hi, at, lo, hi);
    at = s.hi;
    check_prog(s.p, n, what, alg);
  }
  CHECK(at == hi || (lo >= hi && segs.empty()), "%s alg %d n %d: [%zu,%zu) covered up to %zu", what, alg, n, lo, hi,
        at);
}

// the contributions under expression e, with multiplicity
static void leaves_of(const Dag &g, int e, std::vector<int> &out) {
  if (e < g.n) { out.push_back(e); return; }
  leaves_of(g, g.node[e - g.n].first, out);
  leaves_of(g, g.node[e - g.n].second, out);
}

// dag_compile succeeds for every owner; destinations are ranks of the communicator
static void check_dag(const Dag &g, const char *what, int alg) {
  const int n = g.n;
  for (int owner = 0; owner < n; owner++) {
    VmProg p;
    const int rc = dag_compile(g, owner, p);
    CHECK(rc == MX_SUCCESS, "%s alg %d n %d owner %d: dag_compile %d", what, alg, n, owner, rc);
    if (rc == MX_SUCCESS) {
      CHECK(p.nsrc == n && p.nins >= 0 && p.nins <= VM_MAXI && p.nregs <= VM_MAXREG, "%s alg %d n %d: program shape",
            what, alg, n);
      for (int i = 0; i < p.nins; i++) {
        const VmIns &in = p.ins[i];
        const bool emit = (in.op & 3) == VM_EMIT;
        CHECK(in.a >= 0 && in.a < p.nregs && (emit ? in.d >= 0 && in.d < n : in.d >= 0 && in.d < p.nregs && in.b >= 0 && in.b < p.nregs),
              "%s alg %d n %d owner %d: instruction %d out of range", what, alg, n, owner, i);
      }
    }
    const uint32_t m = dest_mask_of(g, owner);
    CHECK((m & ~((1u << n) - 1)) == 0, "%s alg %d n %d owner %d: destination mask %#x", what, alg, n, owner, m);
  }
  for (const DagOut &o : g.out) CHECK(o.e >= 0 && o.e < n + (int)g.node.size() && o.dst >= -1 && o.dst < n,
                                      "%s alg %d n %d: output out of range", what, alg, n);
}

// every output of a full reduction names each contribution exactly once
static void check_full_outputs(const Dag &g, const char *what, int alg) {
  for (const DagOut &o : g.out) {
    std::vector<int> lv;
    leaves_of(g, o.e, lv);
    CHECK(is_perm(lv, g.n), "%s alg %d n %d: an output does not name each contribution once", what, alg, g.n);
  }
}

int main() {
  const size_t es = 4;
  long cases = 0;
  for (int n = 2; n <= MX_MAX_RANKS; n++) {
    const size_t counts[5] = {1, (size_t)n - 1, (size_t)n, (size_t)n + 1, 4 * (size_t)n + 3};
    for (size_t count : counts) {
      // ---- allreduce: tuned 1-6 (and AUTO), libnbc's ring -----------------
      const int ar[] = {MX_ALLREDUCE_AUTO, MX_ALLREDUCE_BASIC_LINEAR, MX_ALLREDUCE_NONOVERLAPPING,
                        MX_ALLREDUCE_RECURSIVE_DOUBLING, MX_ALLREDUCE_RING, MX_ALLREDUCE_SEGMENTED_RING,
                        MX_ALLREDUCE_RABENSEIFNER, kArNbcRing};
      for (int alg : ar) {
        cases++;
        if (alg == MX_ALLREDUCE_NONOVERLAPPING) {
          // mx_allreduce: a rooted reduce to rank 0 (the reduce word of the
          // algorithm word: AUTO), then a bcast
          Dag g(n);
          const int rc = reduce_dag(g, reduce_word_of(alg), count, es, 0, 2);
          CHECK(rc == MX_SUCCESS, "allreduce nonoverlapping n %d: reduce_dag %d", n, rc);
          if (rc == MX_SUCCESS) { check_dag(g, "allreduce nonoverlapping", alg); check_full_outputs(g, "allreduce nonoverlapping", alg); }
          continue;
        }
        size_t off[MAXR], len[MAXR];
        blockcount(count, n, off, len);
        std::vector<Seg> all;
        int rc = allreduce_segments(alg, n, count, es, 0, count, all);
        CHECK(rc == MX_SUCCESS, "allreduce alg %d n %d count %zu: %d", alg, n, count, rc);
        if (rc != MX_SUCCESS) continue;
        check_segs(all, 0, count, n, "allreduce", alg);
        size_t at = 0;
        for (int p = 0; p < n; p++) {   // the part rank p folds
          CHECK(off[p] == at, "blockcount n %d count %zu: part %d at %zu, expected %zu", n, count, p, off[p], at);
          at += len[p];
          std::vector<Seg> part;
          rc = allreduce_segments(alg, n, count, es, off[p], off[p] + len[p], part);
          CHECK(rc == MX_SUCCESS, "allreduce alg %d n %d part %d: %d", alg, n, p, rc);
          check_segs(part, off[p], off[p] + len[p], n, "allreduce part", alg);
        }
        CHECK(at == count, "blockcount n %d count %zu: parts end at %zu", n, count, at);
        // libnbc's Rabenseifner reduce evaluates the same programs as expressions
        for (const Seg &s : all) {
          Dag g(n);
          g.emit(fold_expr(g, s.p), n - 1);
          check_dag(g, "fold_expr", alg);
          check_full_outputs(g, "fold_expr", alg);
        }
      }
      // ---- reduce_scatter 2-4 (and AUTO), ragged counts with a zero -------
      size_t rcounts[MAXR];
      for (int i = 0; i < n; i++) rcounts[i] = (i % 3 == 1) ? 0 : count / n + (size_t)(i % 4);
      rcounts[n - 1] += count % n;
      const int rs[] = {MX_RS_AUTO, MX_RS_RECURSIVE_HALVING, MX_RS_RING, MX_RS_BUTTERFLY};
      for (int alg : rs) {
        size_t disp = 0;
        for (int blk = 0; blk < n; blk++) {
          cases++;
          std::vector<Seg> segs;
          const int rc = reduce_scatter_segments(alg, n, rcounts, es, blk, segs);
          CHECK(rc == MX_SUCCESS, "reduce_scatter alg %d n %d blk %d: %d", alg, n, blk, rc);
          if (rc == MX_SUCCESS) check_segs(segs, disp, disp + rcounts[blk], n, "reduce_scatter", alg);
          disp += rcounts[blk];
        }
      }
      // ---- rooted reduce 1-6 (and AUTO): roots, in-place choices ----------
      for (int alg = MX_REDUCE_AUTO; alg <= MX_REDUCE_IN_ORDER_BINARY; alg++)
        for (int root : {0, n - 1})
          for (int inplace : {0, 1, 2}) {   // 2: both variants, guarded (multi-process part owners)
            cases++;
            Dag g(n);
            const int rc = reduce_dag(g, alg, count, es, root, inplace);
            CHECK(rc == MX_SUCCESS, "reduce alg %d n %d root %d inplace %d: %d", alg, n, root, inplace, rc);
            if (rc != MX_SUCCESS) continue;
            for (const DagOut &o : g.out) CHECK(o.dst == root, "reduce alg %d n %d: output to %d, root %d", alg, n, o.dst, root);
            check_dag(g, "reduce", alg);
            check_full_outputs(g, "reduce", alg);
            if (inplace == 2) continue;
            g.out.back().dst = -1;   // the reduce_scatter_block / NONOVERLAPPING use: the part's owner
            check_dag(g, "reduce (owner output)", alg);
          }
    }
    // ---- scan / exscan: rank r gets contributions 0..r (exscan: 0..r-1) ---
    for (int alg : {MX_SCAN_AUTO, MX_SCAN_LINEAR, MX_SCAN_RECURSIVE_DOUBLING})
      for (int exclusive = 0; exclusive < 2; exclusive++) {
        cases++;
        Dag g(n);
        const int rc = scan_dag(g, alg, exclusive != 0);
        CHECK(rc == MX_SUCCESS, "scan alg %d n %d exclusive %d: %d", alg, n, exclusive, rc);
        if (rc != MX_SUCCESS) continue;
        check_dag(g, exclusive ? "exscan" : "scan", alg);
        std::vector<int> seen(n, 0);
        for (const DagOut &o : g.out) {
          if (o.dst < 0 || o.dst >= n) continue;   // reported by check_dag
          seen[o.dst]++;
          std::vector<int> lv;
          leaves_of(g, o.e, lv);
          CHECK(is_perm(lv, o.dst + (exclusive ? 0 : 1)), "scan alg %d n %d exclusive %d: rank %d's prefix", alg, n,
                exclusive, o.dst);
        }
        for (int r = exclusive; r < n; r++) CHECK(seen[r] == 1, "scan alg %d n %d: %d outputs for rank %d", alg, n, seen[r], r);
      }
    // ---- libnbc's binomial and chain, scoll/basic's recursive doubling ----
    for (int root : {0, n - 1}) {
      cases++;
      Dag b(n);
      b.emit(nbc_binomial_expr(b, root), root);
      check_dag(b, "nbc binomial", root);
      check_full_outputs(b, "nbc binomial", root);
      Dag c(n);
      c.emit(nbc_chain_expr(c, root, true), root, VM_IF_SET);
      c.emit(nbc_chain_expr(c, root, false), root, VM_IF_CLEAR);
      check_dag(c, "nbc chain", root);
      check_full_outputs(c, "nbc chain", root);
    }
    {
      cases++;
      Dag g(n);
      CHECK(shmem_basic_rd_dag(g) == MX_SUCCESS, "shmem recursive doubling n %d", n);
      check_dag(g, "shmem recursive doubling", 0);
      check_full_outputs(g, "shmem recursive doubling", 0);
      CHECK((int)g.out.size() == n, "shmem recursive doubling n %d: %zu outputs", n, g.out.size());
    }
  }
  printf("plan_check: %ld cases, %d failures\n", cases, g_fail);
  return g_fail ? 1 : 0;
}
