// mx_rooted_plan.hpp -- host-only planning of the rooted exchanges (gather,
// gatherv, scatter, scatterv; mx_rooted_plan.hip): what a rank publishes of
// its sides, the verdict every rank draws from the published rows, the
// staging geometry, and for (kind, root, rank, round) the jobs a rank
// launches before and after READY with the ranks its waits depend on.  The
// jobs go to the two exchange kernels unchanged.  No HIP API, no
// communicator, no launch: it compiles with a host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "mx_exchange_vec_plan.hpp"

namespace mx {

enum { RK_GATHER = 0, RK_SCATTER = 1 };

// What one rank publishes.  Every rank has a SINGLE side -- the block it
// sends (gather) or receives (scatter); the root also has the MULTI side
// with one block per rank -- where a gather lands, what a scatter reads.
// Nothing here is assumed equal on two ranks: the root may describe a vector
// type where its peers describe bytes, and only the root knows.
struct RRowHead {
  int32_t root, kind;
  int32_t verdict;   // this rank can take part on the device (its datatypes qualify)
  int32_t inplace;   // the root only: its own block is where it belongs
  XLay lay;          // the single side's layout
  int64_t lo;        // lower bound, from the user pointer, of the span the rank registers
  uint64_t bytes;    // the single side's stream bytes
  uint32_t unit;     // its access unit (layout and address)
  uint32_t mis;      // a flat single side: the address of its first byte mod 16
  // the root only
  XLay mlay;
  int64_t mlo;
  uint32_t munit;    // the multi side's access unit (layout and address)
  uint32_t mmis;     // a flat multi side: the address of offset 0 mod 16
};
struct RRow {
  RRowHead h;
  uint64_t mbytes[MX_MAX_RANKS];   // the root only: stream bytes of rank p's block in the multi side
  int64_t moffs[MX_MAX_RANKS];     // ... and its displacement there in bytes
};

// What every rank derives from the rows, alike.
struct RHead {
  int n, root, kind;
  bool inplace;
  uint64_t len[MX_MAX_RANKS];    // stream bytes of rank p's block that move: never past the receiver's room
  bool bytepair[MX_MAX_RANKS];   // both sides flat: a byte job of any length and alignment (no word rule)
  uint64_t max_block;            // the largest len
};

// MX_SUCCESS: the call is taken, *h filled.  MX_ERR_ARG: the rows disagree on
// root or kind (or the root is out of range).  MX_ERR_UNSUPPORTED: a negative
// verdict, a pair whose word would be below 4 bytes, or size x largest block
// at or under xmin (0: no minimum).  A function of the rows alone.
int rooted_verdict(const RRow *rows, int n, size_t xmin, RHead *h);

// Staging of a staged call.  A gather's root receives from n - 1 senders: n
// slots as in the all-to-all forms.  A scatter's receivers each have ONE
// sender, so a round carries the whole staging.
struct RGeom {
  size_t slot, cap;
  uint64_t rounds;
};
bool rooted_geom(size_t main_bytes, int n, int kind, uint64_t max_block, RGeom *g);

// One job: `len` stream bytes from position pos_s of the source side to
// position pos_d of the destination side.  A side is a buffer of a rank, a
// byte offset into it and a layout.
enum { RB_SINGLE = 0, RB_MULTI = 1, RB_STAGE = 2 };
struct REnd {
  int buf, rank;   // RB_SINGLE / RB_STAGE of `rank`; RB_MULTI is the root's
  int64_t off;
  XLay lay;
  uint64_t pos;
};
struct RJob {
  REnd s, d;
  uint64_t len;
  bool bytes;      // an XJob for k_exchange; else xvjob_make's rule holds for it
};

// The staged path: the jobs `rank` launches in round q before READY (phase 0:
// pushes into a peer's staging, the root's own block) and after it (phase 1:
// moves out of its own staging), and the ranks its two waits depend on:
// whose DONE(g - 1) the phase 0 jobs need (the owners of the stagings they
// write) and whose READY the phase 1 jobs need.
void rooted_staged_jobs(const RHead &h, const RRow *rows, const RGeom &g, int rank, uint64_t q, int phase,
                        std::vector<RJob> &out);
uint32_t rooted_staged_done_mask(const RHead &h, const RGeom &g, int rank, uint64_t q);
uint32_t rooted_staged_ready_mask(const RHead &h, const RGeom &g, int rank, uint64_t q);

// The zero-copy path: the one launch of `rank` (the gather's root pulls every
// block, a scatter's non-root its own; the root's own block moves directly),
// whose READY it waits for before, and whose PUSHED it waits for after
// (the readers of its registered buffer).
void rooted_zc_jobs(const RHead &h, const RRow *rows, int rank, std::vector<RJob> &out);
uint32_t rooted_zc_ready_mask(const RHead &h, int rank);
uint32_t rooted_zc_pushed_mask(const RHead &h, int rank);

// A communicator of one process: every block straight from its source to its place.
void rooted_local_jobs(const RHead &h, const RRow *rows, std::vector<RJob> &out);

}  // namespace mx
