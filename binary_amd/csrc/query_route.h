// query_route.h — which kernels answer a single-pass query batch (bivx_query_dev*, bivx_count_dev*, bivx_query_dev_u,
// bivx_self_overlaps_dev), and in launches of how many queries. Host code only, no HIP header: tests/cpp/query_route.cpp
// compiles it with g++ and pins the policy at every threshold. launch_single_pass (query_fused.hip) carries a plan out.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace bivx {

// ---- what the policy knows of the kernels ------------------------------------------------------------------------
// Workgroup sizes are build-time tuning knobs (tools sweep them): every translation unit must be built with the same ones.
#ifndef BIVX_FUSED_THREADS
#define BIVX_FUSED_THREADS 1024
#endif
#ifndef BIVX_PIPE_THREADS
#define BIVX_PIPE_THREADS 1024  // (experiments: 512 = seven workers and the service wavefront)
#endif
// queries per tile (workgroup)
constexpr uint32_t kFusedTile = BIVX_FUSED_THREADS;                // k_query_fused: one query per thread
constexpr uint32_t kPipeTile = (BIVX_PIPE_THREADS / 64 - 1) * 64;  // k_query_pipe(_dense): 960, a query per worker lane
constexpr uint32_t kMsTile = 448;                                  // k_query_pipe_ms: seven workers of 64 lanes
// tiles per launch: ordered output is limited to what one prefix sweep covers; k_query_fused's unordered output only by
// the departure count's 20 bits in ws[kWsDone]
constexpr unsigned kFMaxTiles = 65536;
constexpr unsigned kFUnorderedMaxTiles = 1u << 19;
constexpr uint32_t kMaxCellForPipe = 64;    // indexes with a fuller directory cell than this stay on k_query_fused
constexpr uint32_t kMsGroupMax = 1024;      // slots of the longest window a group of lanes walks in k_query_pipe_ms
constexpr uint32_t kPipeStageMaxAvg = 6;    // ids per query (by buffer capacity) up to which a wavefront's lists fit its stage
constexpr uint32_t kFusedSortMaxAvg = 6;    // ids per query (by buffer capacity) up to which k_query_fused orders ids itself
constexpr size_t kPipeMinQueries = (size_t)768 * 1024;        // ordered output
constexpr size_t kPipeUnorderedMinQueries = (size_t)4 << 20;  // begin / count output
constexpr size_t kDenseMinQueries = (size_t)4 * 512 * kPipeTile;
constexpr size_t kSelfMinQueries = (size_t)64 * kPipeTile;
constexpr uint32_t kPipeMaxSlots = 1u << 28;  // 32-bit byte offsets into the records
constexpr uint32_t kMsMaxSlots = 1u << 27;    // ... and ids, 8 bytes per pair, behind se[] in the same block

// ---- the environment knobs, read once per public call (tests switch them between calls) --------------------------
struct RouteKnobs {
  int pipe = 1;            // BIVX_PIPE: 0 = never a pipelined kernel, 1 = when eligible, 2 = also small batches and hotspots (tests)
  bool ms = true;          // BIVX_PIPE_MS=0: never k_query_pipe_ms (tests compare the two kernels)
  unsigned wgs = 0;        // BIVX_PIPE_WGS: workgroups of the pipelined kernels (0: two per compute unit)
  long max_tiles = 0;      // BIVX_MAX_TILES_PER_LAUNCH: forces the chained-launch path (0: the kernels' own limits)
  int wait_log2 = 0;       // BIVX_PREFIX_WAIT_LOG2: bound of a prefix wait as log2 of 10 ns ticks (0: the default); 1 makes
                           // every wait that is not satisfied at once expire, which is how the error path is exercised
};

inline RouteKnobs read_route_knobs() {
  RouteKnobs k;
  if (const char *e = std::getenv("BIVX_PIPE")) k.pipe = std::atoi(e);
  if (const char *e = std::getenv("BIVX_PIPE_MS")) k.ms = std::atoi(e) != 0;
  if (const char *e = std::getenv("BIVX_PIPE_WGS")) {
    const long w = std::atol(e);
    if (w >= 1 && w <= 65536) k.wgs = (unsigned)w;
  }
  if (const char *e = std::getenv("BIVX_MAX_TILES_PER_LAUNCH")) k.max_tiles = std::atol(e);
  if (const char *e = std::getenv("BIVX_PREFIX_WAIT_LOG2")) {
    const long w = std::atol(e);
    if (w > 0 && w < 64) k.wait_log2 = (int)w;
  }
  return k;
}

// ---- the plan ----------------------------------------------------------------------------------------------------
// What the eligibility checks read of a built index (shape_of(IndexView), capi.hip).
struct RouteShape {
  bool filtered;        // a fused post-filter (bivx_filter)
  uint32_t max_segs;    // most segments any one chromosome has
  bool fits_lds;        // the segment descriptors fit the kernels' LDS copy
  uint32_t nslots;
  uint32_t max_cell;    // most slots any directory cell holds
  uint32_t max_window;  // slots a query's window is expected to hold where that is most
  bool rec_span_32;     // se[] .. the end of rec[] within 32-bit byte offsets (se[] and rec[] are one block)
};

enum class QueryRoute { Fused, Pipe, Ms, DenseFused, DenseMs };

// The dense routes launch k_query_pipe_dense in front of the second kernel: it takes the launch if k_probe_order finds the
// batch position-sorted, and the second kernel returns at once; otherwise the second kernel does the work.
inline const char *route_name(QueryRoute r) {
  switch (r) {
    case QueryRoute::Pipe: return "k_query_pipe";
    case QueryRoute::Ms: return "k_query_pipe_ms";
    case QueryRoute::DenseFused: return "k_query_pipe_dense|k_query_fused";
    case QueryRoute::DenseMs: return "k_query_pipe_dense|k_query_pipe_ms";
    default: return "k_query_fused";
  }
}

struct Plan {
  QueryRoute route;
  size_t tile_q;      // queries per tile of the route's kernel with the smallest tiles (how many tile words a launch uses)
  size_t per_launch;  // queries per launch; a larger batch runs as consecutive launches
  bool sort_inside;   // ascending ids are ordered inside k_query_fused (k_sort_hits only runs if a wavefront asks for it)
};

inline size_t tiles_per_launch(unsigned limit, const RouteKnobs &k) {
  return k.max_tiles >= 1 && k.max_tiles < (long)limit ? (size_t)k.max_tiles : limit;
}

// d_counts != nullptr in the caller (begin / count output) is `unordered`.
inline Plan plan_single_pass(const RouteShape &s, size_t q, uint64_t cap, bool sort_ids, bool unordered, const RouteKnobs &k) {
  const bool forced = k.pipe == 2;
  // few ids per query: a wavefront's 64 lists fit the pipelined kernels' stage (the capacity is the only bound the host has)
  const bool few = cap <= (uint64_t)kPipeStageMaxAvg * q;
  // One segment per chromosome, no filter, no positional hotspot: k_query_pipe and k_query_pipe_dense. (Hotspots — thousands
  // of intervals starting inside one directory cell — make single slices take hundreds of microseconds; a pipe tile waits
  // for all fifteen of its slices, k_query_fused's tiles wait for nobody but their predecessors' totals:
  // tools/clustered_bench.py, zero-capacity count: 1.32 ms there, 0.78 in k_query_fused.)
  const bool simple = k.pipe != 0 && !s.filtered && s.max_segs <= 1 && s.fits_lds && s.nslots <= kPipeMaxSlots &&
                      (s.max_cell <= kMaxCellForPipe || forced);
  const size_t pipe_tiles = tiles_per_launch(kFMaxTiles, k);
  bool pipe;
  if (unordered)  // (one launch only: there is no entry q_end to chain launches through. At 1 M queries k_query_fused<U>,
                  // whose tiles wait for nobody, takes 43 us (22 position-sorted) against 48 (32) here.)
    pipe = simple && few && !sort_ids && (q >= kPipeUnorderedMinQueries || forced) && q <= pipe_tiles * kPipeTile;
  else  // (a pipeline has to fill and drain: below about 0.7 M queries — 1.4 tiles per resident workgroup — k_query_fused
        // is the faster one. 0.25 M: 19.7 against 23.7 us, 0.5 M: 32 / 35, 0.75 M: 45 / 43, 1 M: 54 / 49, 1.3 M: 70 / 60)
    pipe = simple && few && (q >= kPipeMinQueries || forced);
  // many ids per query (more than the stages hold): the regenerating form of the pipeline, for position-sorted batches
  const bool dense = !unordered && simple && !few && (q >= kDenseMinQueries || forced);
  // What k_query_pipe leaves out — several segments per chromosome, a fused filter — in index order. (Many ids per query on
  // ONE length class, queries in any order: k_query_fused is the faster one — config 5 in generation order 7.7 ms against
  // 8.5 here; tests send it here with BIVX_PIPE=2.) Windows beyond kMsGroupMax slots go through the general enumeration
  // twice here.
  const bool ms = !pipe && k.ms && k.pipe != 0 && !unordered && s.fits_lds && (q >= kPipeMinQueries || forced) &&
                  s.nslots <= kMsMaxSlots && s.rec_span_32 &&
                  ((s.max_cell <= kMsGroupMax / 4 && s.max_window <= kMsGroupMax / 2) || forced) &&
                  (s.max_segs > 1 || s.filtered || (forced && !few));
  Plan p;
  p.route = pipe ? QueryRoute::Pipe : dense ? (ms ? QueryRoute::DenseMs : QueryRoute::DenseFused) : ms ? QueryRoute::Ms : QueryRoute::Fused;
  // (k_query_pipe_dense in front of k_query_pipe_ms: the launch is cut at the smaller tiles of the two)
  p.tile_q = ms ? kMsTile : pipe || dense ? kPipeTile : kFusedTile;
  p.per_launch = p.tile_q * (pipe || dense || ms ? pipe_tiles : tiles_per_launch(unordered ? kFUnorderedMaxTiles : kFMaxTiles, k));
  // Ordering ids inside the kernel pays while a wavefront's 64 lists fit half its output stage (one round, all lanes
  // busy). Denser results are ordered by k_sort_hits afterwards, whose stage is eight times larger.
  p.sort_inside = sort_ids && !unordered && !ms && cap <= (uint64_t)kFusedSortMaxAvg * q;
  return p;
}

// bivx_self_overlaps_dev: true if the index's own intervals go through k_query_pipe_dense in slot order (one launch:
// nothing chains output positions across launches); false for the general path, the intervals as a query batch.
inline bool plan_self_overlaps(const RouteShape &s, size_t n, const RouteKnobs &k) {
  return k.pipe != 0 && !s.filtered && s.max_segs <= 1 && s.fits_lds && s.nslots <= kPipeMaxSlots &&
         s.max_cell <= kMaxCellForPipe && n <= (size_t)kFMaxTiles * kPipeTile && (n >= kSelfMinQueries || k.pipe == 2);
}

}  // namespace bivx
