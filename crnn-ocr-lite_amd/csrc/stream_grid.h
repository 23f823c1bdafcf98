// The two workgroup grids of the streamed pointwise GEMMs: one host plan each, and the stripe grid's device decode ("The streamed GEMMs'
// two grids").  Include after common.h.
//   StripeGrid: gemm_wres.hip, gemm_wres3.hip, gemm_pres.hip -- persistent workgroups, weights resident, the pixel stripes stream.
//   SplitGrid:  gemm_wgrad.hip, gemm_wgrad3.hip -- one output tile per workgroup over a contiguous range of the pixel reduction.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------- stripe grid
// grid = nxcd x Q x S workgroups.  Workgroup ids go round-robin over the 8 XCDs, so id -> (x = id % nxcd, slice = (id / nxcd) % S, q = id / nxcd / S):
// the S channel slices of a stripe run at the same time on CUs of ONE XCD (HBM sees the stripe once, the other slices hit that XCD's L2), and the
// Q * nxcd stripe lanes (lane = q * nxcd + x) walk the stripes lane, lane + Q * nxcd, ...
struct StripeGrid {
  int stripes;   // pixel stripes of the launch
  int S;         // channel slices
  int Q;         // stripe lanes per XCD (workgroups per XCD / S)
  int nxcd;      // XCDs the grid spans
};

// Fills g and returns the grid size.  cus * occ / 8 workgroups per XCD.  More slices than that: flat_overflow (gemm_wres.hip; dense1's data gradient, 36
// slices of a 3.4 MB operand) gives every (slice, lane) pair one workgroup, at most one per CU -- the lanes no longer coincide with XCDs, which only
// matters for operands that do not fit the L2s; otherwise the XCD takes S workgroups anyway (Q = 1).
static inline int stripe_grid_plan(StripeGrid& g, int stripes, int slices, int cus, int occ, bool flat_overflow) {
  g.stripes = stripes; g.S = slices; g.nxcd = 8;
  int per_xcd = cus / 8 * occ;
  if (g.S > per_xcd) {
    if (flat_overflow) {
      g.nxcd = cus / g.S < 1 ? 1 : cus / g.S;
      g.Q = 1;
      if (g.nxcd > g.stripes) g.nxcd = g.stripes;
      return g.nxcd * g.S;
    }
    per_xcd = g.S;
  }
  g.Q = per_xcd / g.S;
  const int need = cdiv(g.stripes, g.nxcd);                    // stripe lanes that have any work
  if (g.Q > need) g.Q = need;
  return g.nxcd * g.Q * g.S;
}
// stripe lanes: the partial-statistics rows of a launch are this times the statistics waves of a workgroup
static inline int stripe_grid_lanes(const StripeGrid& g) { return g.Q * g.nxcd; }

// This workgroup's place in the grid: its channel slice, its stripe lane (= the first stripe it takes; also numbers its statistics rows), the stride
// between its stripes and how many it takes (0: none -- its statistics rows must still be written as zeros)
struct StripeLane { int slice, first, step, mine; };
__device__ __forceinline__ StripeLane stripe_lane(const StripeGrid g) {
  const int wg = blockIdx.x;
  const int x = wg % g.nxcd, jq = wg / g.nxcd;
  StripeLane l;
  l.slice = jq % g.S;
  const int q = jq / g.S;
  l.step = g.Q * g.nxcd;
  l.first = q * g.nxcd + x;
  l.mine = l.first < g.stripes ? (g.stripes - l.first + l.step - 1) / l.step : 0;
  return l;
}

// ---------------------------------------------------------------------------------------------------------------- reduction-split grid
// TI x TJ output tiles x nsplit contiguous ranges of `per` chunks of the pixel reduction (the last range may be shorter); the fp32 partial tiles go to
// scratch [nsplit][rows][cols] and a fixed-order second stage sums them.  grid = 8 * ceil(nsplit / 8) * tiles, id -> (x = id % 8, tile = (id / 8) % tiles,
// range = 8 * (id / 8 / tiles) + x): the tiles of a range are neighbours on one XCD (they read the same pixel rows).  flat (more tiles than an XCD has
// CUs; dense1: 36): grid = tiles * nsplit, id -> (tile = id % tiles, range = id / tiles) -- a range's tiles spread over the XCDs (one XCD would run 32
// of them and then the other 4: twice the time, measured).
// The plan is shared; the decode stays spelled out in the two kernels, and `flat` stays where it was in their parameter blocks (behind lda / ldg): moved
// into a helper, or to another argument offset, either changed the kernels' vector code (profiles/stream_grid_refactor.txt).
struct SplitGrid {
  int chunks;        // chunks of the reduction
  int TI, TJ;        // output tiles along the rows and the columns
  int nsplit, per;   // ranges, chunks per range
};

// Fills g and flat and returns the grid size: one workgroup per CU, a multiple of 8 ranges (flat: cus / tiles ranges), a range at least two pipeline
// depths long
static inline int split_grid_plan(SplitGrid& g, int& flat, int chunks, int TI, int TJ, int cus, int depth) {
  g.chunks = chunks; g.TI = TI; g.TJ = TJ;
  const int tiles = TI * TJ;
  int ns = (cus / tiles) & ~7;
  flat = tiles > cus / 8;
  if (flat) ns = cus / tiles < 1 ? 1 : cus / tiles;
  else if (ns < 8) ns = 8;
  while (ns > 8 && chunks / ns < 2 * depth) ns -= 8;
  if (ns > chunks) ns = chunks;                                // (tiny inputs: ranges of one chunk; some of the 8 XCD lanes stay empty)
  g.per = cdiv(chunks, ns);
  g.nsplit = cdiv(chunks, g.per);                              // drop empty tail ranges
  return flat ? g.nsplit * tiles : 8 * cdiv(g.nsplit, 8) * tiles;
}
