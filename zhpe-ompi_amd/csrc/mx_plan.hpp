// mx_plan.hpp -- host-only reduction-order planning (mx_plan.hip): which
// tree every element of a collective gets, restating the reference's
// algorithms, and the plain programs the fold kernels (mx_fold.hpp) evaluate.
// No HIP API, no communicator, no launch: it compiles with a host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <map>
#include <utility>
#include <vector>

#include "../../include/mx_kernels.h"
#include "../../include/mx_coll.h"
#include "mx_slots.hpp"

namespace mx {

constexpr int MAXR = MX_MAX_RANKS;
constexpr int OS_MAXSEG = 16;

// ---------------------------------------------------------------------------
// fold programs
// ---------------------------------------------------------------------------
enum { PROG_CHAIN = 0, PROG_BFLY = 1 };

struct FoldProg {
  int kind;
  int n;           // chain: number of operands; butterfly: p' leaves
  int D;           // butterfly depth (p' = 1 << D)
  int acc_first;   // chain: accumulator is the target (first operand)
  uint32_t pref;   // butterfly: bit s set -> upper half is the target at level s
  int8_t ord[MAXR];  // chain: source index per step
  int8_t la[MAXR];   // butterfly leaf slot i: first operand source
  int8_t lb[MAXR];   //   second operand source, -1 = plain leaf
};

constexpr int VM_MAXI = 192;     // instructions per program
constexpr int VM_MAXREG = 40;    // registers (contributions + temporaries)
// op: VM_COMB / VM_EMIT, optionally guarded by the call's info bit (the
// root's MPI_IN_PLACE in a rooted reduce): executed only if set / clear
enum { VM_COMB = 0, VM_EMIT = 1, VM_IF_SET = 4, VM_IF_CLEAR = 8 };
struct VmIns { int8_t op, d, a, b; };
struct VmProg {
  int nsrc, nregs, nins;
  VmIns ins[VM_MAXI];
};

// ---- fold partitions ------------------------------------------------------
struct Seg { size_t lo, hi; FoldProg p; };

// COLL_BASE_COMPUTE_BLOCKCOUNT (coll_base_functions.h:428-435)
void blockcount(size_t count, int nblocks, size_t *off, size_t *len);
int pof2_le(int n);   // the largest power of two <= n

// the reduce word (MX_REDUCE_* | fanout << 16) carried by an algorithm word
// (MX_ALG_WORD) of the algorithms built on a rooted reduce
inline int reduce_word_of(int alg) { return ((alg >> 8) & 0xff) | (alg & 0xff0000); }

// Internal allreduce algorithm id: libnbc's ring (allred_sched_ring,
// nbc_iallreduce.c:629-860), reached through mx_iallreduce.
constexpr int kArNbcRing = 201;   // fits the algorithm byte of an MX_ALG_WORD

// Allreduce fold segments restricted to [rlo, rhi).
int allreduce_segments(int alg, int n, size_t count, size_t es, size_t rlo, size_t rhi, std::vector<Seg> &out);
// Reduce-scatter fold segments for output block `blk` (elements relative to
// the full vector).
int reduce_scatter_segments(int alg, int n, const size_t *rcounts, size_t es, int blk, std::vector<Seg> &out);

// ---- expression DAGs and their VM programs --------------------------------
// output: expression -> destination rank (-1 = the part's owner), guard 0
// always / VM_IF_SET / VM_IF_CLEAR (the root's MPI_IN_PLACE variant)
struct DagOut { int e, dst, guard; };
struct Dag {
  int n;
  std::vector<std::pair<int, int>> node;     // node id n + i = COMB(first, second)
  std::map<std::pair<int, int>, int> memo;   // structural sharing
  std::vector<DagOut> out;
  explicit Dag(int n_) : n(n_) {}
  void emit(int e, int dst, int guard = 0) { out.push_back(DagOut{e, dst, guard}); }
  int comb(int target, int source) {
    const auto k = std::make_pair(target, source);
    const auto it = memo.find(k);
    if (it != memo.end()) return it->second;
    const int id = n + (int)node.size();
    node.push_back(k);
    memo[k] = id;
    return id;
  }
};

int dag_compile(const Dag &g, int owner, VmProg &p);
uint32_t dest_mask_of(const Dag &g, int owner_rank);
int reduce_dag(Dag &g, int word, size_t count, size_t es, int root, int root_inplace);
int scan_dag(Dag &g, int alg, bool exclusive);
int shmem_basic_rd_dag(Dag &g);
int nbc_binomial_expr(Dag &g, int vroot);
int nbc_chain_expr(Dag &g, int root, bool root_inplace);
int fold_expr(Dag &g, const FoldProg &p);

}  // namespace mx
