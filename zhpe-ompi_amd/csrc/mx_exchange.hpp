// mx_exchange.hpp -- the exchange kernel (mx_exchange.hip): one launch moves a
// table of {src, dst, bytes} jobs of unequal size and any byte alignment
// (alltoall, alltoallv, allgatherv).  The tables and the launch geometry are
// planned on the host (mx_exchange_plan.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "mx_exchange_plan.hpp"
#include "mx_exchange_vec_plan.hpp"

namespace mx {

// Up to this many jobs travel in the kernel's argument block; longer tables
// (the n x n jobs of a local communicator) go through an XTable.
constexpr int kXInline = MX_MAX_RANKS;

// Table memory of one communicator for launches of more than kXInline jobs:
// two slots of pinned host memory and device memory, used in turn.  A slot
// is written again only after the event behind its last launch has passed,
// so neither the asynchronous copy nor the kernel can see the next table.
struct XTable {
  char *host[2], *dev[2];
  hipEvent_t ev[2];
  bool used[2];
  unsigned next;
};
XTable *xtable_new();            // nullptr: out of memory
void xtable_free(XTable *t);

// Enqueues the jobs on `s` (empty jobs dropped; nothing to do: no launch).
// poison: the communicator's poison word or null.  The ranges of different
// jobs must not overlap a destination range.  More than kXInline jobs go out
// as one launch through `tab`; without one, as launches of kXInline jobs.
int exchange_launch(const XJob *jobs, size_t n, const int *poison, hipStream_t s, XTable *tab = nullptr);

// the layout of a committed datatype (mx_convertor.hip)
const DdtLayout *ddt_layout(const mx_ddt *d);

// The strided exchange kernel (mx_exchange_vec.hip): enqueues jobs made by
// xvjob_make on `s`, one launch per word width and kXInline jobs; jobs whose
// two sides are flat go to exchange_launch.  No two jobs may write the same byte.
int exchange_vec_launch(const XVJob *jobs, size_t n, const int *poison, hipStream_t s);

}  // namespace mx

// For the tests (not part of include/mx_coll.h): the destination bytes one
// workgroup and one wave step of k_exchange move -- sizes around them are
// where its paths change -- and the staging rounds a staged exchange whose
// largest pair is max_pair bytes takes on this communicator (0 for an empty
// call or a local communicator; MX_ERR_NOMEM: the staging holds none).
extern "C" int mx_exchange_geometry(size_t *block_bytes, size_t *wave_bytes);
// XTables alive in this process: a communicator's goes back to the pools when it is destroyed
extern "C" int mx_exchange_tables_live(void);
extern "C" long long mx_comm_exchange_rounds(const mx_comm_t *comm, size_t max_pair);
// k_exchange_vec: the stream bytes one workgroup and one wave step move at
// word width W (4, 8, 16), and the jobs this process launched at W = 4, 8, 16
extern "C" int mx_exchange_vec_geometry(unsigned W, size_t *block_bytes, size_t *wave_bytes);
extern "C" int mx_exchange_vec_widths(uint64_t out[3]);
