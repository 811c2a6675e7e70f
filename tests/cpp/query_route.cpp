// The single-pass route policy (binary_amd/csrc/query_route.h) at each of its thresholds: which kernels a batch goes to,
// in launches of how many queries, and whether ids are ordered inside k_query_fused. Host code only: g++ -std=c++17.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "query_route.h"

using namespace bivx;

static int g_pass = 0, g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (c) {                                                      \
      ++g_pass;                                                   \
    } else {                                                      \
      ++g_fail;                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                             \
  } while (0)

// no filter, one segment per chromosome, descriptors in LDS, no hotspot
static RouteShape simple() { return RouteShape{false, 1, true, 1000000, 64, 100, true}; }

static const char *name(const RouteShape &s, size_t q, uint64_t cap, const RouteKnobs &k = RouteKnobs{}, bool sort_ids = false,
                        bool unordered = false) {
  return route_name(plan_single_pass(s, q, cap, sort_ids, unordered, k).route);
}
static bool is(const char *a, const char *b) { return std::strcmp(a, b) == 0; }

int main() {
  const RouteKnobs dflt;
  RouteKnobs never, forced, no_ms, three;
  never.pipe = 0;
  forced.pipe = 2;
  no_ms.ms = false;
  three.max_tiles = 3;
  const RouteShape s = simple();

  // ordered output, default knobs, simple shape
  CHECK(is(name(s, 786431, 0), "k_query_fused"));
  CHECK(is(name(s, 786432, 6ull * 786432), "k_query_pipe"));
  CHECK(is(name(s, 786432, 6ull * 786432 + 1), "k_query_fused"));
  CHECK(is(name(s, 1966079, 6ull * 1966079 + 1), "k_query_fused"));
  CHECK(is(name(s, 1966080, 6ull * 1966080 + 1), "k_query_pipe_dense|k_query_fused"));
  {
    RouteShape hot = s;
    hot.max_cell = 65;
    CHECK(is(name(hot, 1 << 22, 0), "k_query_fused"));
  }

  // several segments per chromosome or a filter: k_query_pipe_ms, within its slot and window limits
  RouteShape multi = s;
  multi.max_segs = 2;
  multi.nslots = 1u << 27;
  multi.max_window = 512;
  RouteShape filt = s;
  filt.filtered = true;
  filt.nslots = 1u << 27;
  filt.max_window = 512;
  CHECK(is(name(multi, 786432, 0), "k_query_pipe_ms"));
  CHECK(is(name(multi, 786432, 100ull * 786432), "k_query_pipe_ms"));
  CHECK(is(name(filt, 786432, 0), "k_query_pipe_ms"));
  CHECK(is(name(multi, 786431, 0), "k_query_fused"));
  CHECK(is(name(multi, 786432, 0, no_ms), "k_query_fused"));
  CHECK(is(name(filt, 786432, 0, no_ms), "k_query_fused"));
  {
    RouteShape m = multi;
    m.nslots = (1u << 27) + 1;
    CHECK(is(name(m, 786432, 0), "k_query_fused"));
    m = multi;
    m.max_window = 513;
    CHECK(is(name(m, 786432, 0), "k_query_fused"));
    CHECK(is(name(m, 786432, 0, forced), "k_query_pipe_ms"));
    m = multi;
    m.max_cell = 257;
    CHECK(is(name(m, 786432, 0), "k_query_fused"));
    m = multi;
    m.rec_span_32 = false;
    CHECK(is(name(m, 786432, 0), "k_query_fused"));
    m = multi;
    m.fits_lds = false;
    CHECK(is(name(m, 786432, 0), "k_query_fused"));
  }

  // BIVX_PIPE=0: k_query_fused for every shape
  for (const RouteShape &sh : {s, multi, filt})
    for (size_t q : {(size_t)1000, (size_t)786432, (size_t)1966080, (size_t)(4u << 20)})
      for (uint64_t cap : {(uint64_t)0, (uint64_t)6 * q, (uint64_t)6 * q + 1}) CHECK(is(name(sh, q, cap, never), "k_query_fused"));

  // BIVX_PIPE=2: small batches and hotspots too
  CHECK(is(name(s, 1000, 6000, forced), "k_query_pipe"));
  {
    RouteShape hot = s;
    hot.max_cell = 65;
    CHECK(is(name(hot, 1000, 6000, forced), "k_query_pipe"));
  }
  CHECK(is(name(s, 1000, 6001, forced), "k_query_pipe_dense|k_query_pipe_ms"));
  CHECK(is(name(s, 1000, 6001, forced, false, true), "k_query_fused"));
  {
    RouteShape big = s;
    big.nslots = (1u << 28) + 1;
    CHECK(is(name(big, 786432, 0), "k_query_fused"));
    CHECK(is(name(big, 786432, 0, forced), "k_query_fused"));
    big.nslots = 1u << 28;
    CHECK(is(name(big, 786432, 0), "k_query_pipe"));
  }

  // unordered (begin / count) output
  CHECK(is(name(s, (4u << 20) - 1, 0, dflt, false, true), "k_query_fused"));
  CHECK(is(name(s, 4u << 20, 6ull * (4u << 20), dflt, false, true), "k_query_pipe"));
  CHECK(is(name(s, 4u << 20, 6ull * (4u << 20) + 1, dflt, false, true), "k_query_fused"));
  CHECK(is(name(s, 4u << 20, 0, dflt, true, true), "k_query_fused"));
  CHECK(is(name(s, 62914560, 0, dflt, false, true), "k_query_pipe"));
  CHECK(is(name(s, 62914561, 0, dflt, false, true), "k_query_fused"));
  CHECK(is(name(s, 2881, 0, [] { RouteKnobs k; k.pipe = 2; k.max_tiles = 3; return k; }(), false, true), "k_query_fused"));
  CHECK(is(name(s, 2880, 0, [] { RouteKnobs k; k.pipe = 2; k.max_tiles = 3; return k; }(), false, true), "k_query_pipe"));
  CHECK(is(name(multi, 4u << 20, 0, dflt, false, true), "k_query_fused"));

  // queries per launch (and per tile)
  {
    const Plan pipe = plan_single_pass(s, 786432, 0, false, false, dflt);
    const Plan dense = plan_single_pass(s, 1966080, 1ull << 40, false, false, dflt);
    const Plan ms = plan_single_pass(multi, 786432, 0, false, false, dflt);
    const Plan dense_ms = plan_single_pass(s, 1000, 6001, false, false, forced);
    const Plan fused = plan_single_pass(s, 1000, 0, false, false, dflt);
    const Plan fused_u = plan_single_pass(s, 1000, 0, false, true, dflt);
    CHECK(pipe.per_launch == 62914560 && pipe.tile_q == 960);
    CHECK(dense.per_launch == 62914560 && dense.tile_q == 960);
    CHECK(ms.per_launch == 29360128 && ms.tile_q == 448);
    CHECK(dense_ms.per_launch == 29360128 && dense_ms.tile_q == 448);
    CHECK(fused.per_launch == (size_t)65536 * 1024 && fused.tile_q == 1024);
    CHECK(fused_u.per_launch == ((size_t)1 << 19) * 1024 && fused_u.tile_q == 1024);
    CHECK(plan_single_pass(s, 786432, 0, false, false, three).per_launch == 3 * 960);
    CHECK(plan_single_pass(s, 1966080, 1ull << 40, false, false, three).per_launch == 3 * 960);
    CHECK(plan_single_pass(multi, 786432, 0, false, false, three).per_launch == 3 * 448);
    CHECK(plan_single_pass(s, 1000, 0, false, false, three).per_launch == 3 * 1024);
    CHECK(plan_single_pass(s, 1000, 0, false, true, three).per_launch == 3 * 1024);
    RouteKnobs beyond;  // (at or above a kernel's limit the knob is ignored)
    beyond.max_tiles = 65536;
    CHECK(plan_single_pass(s, 1000, 0, false, false, beyond).per_launch == (size_t)65536 * 1024);
    CHECK(plan_single_pass(s, 1000, 0, false, true, beyond).per_launch == (size_t)65536 * 1024);
    CHECK(plan_single_pass(s, 786432, 0, false, false, beyond).per_launch == 62914560);
  }

  // ids ordered inside k_query_fused: sort_ids, ordered output, few ids per query, not the ms route
  CHECK(plan_single_pass(s, 1000, 6000, true, false, dflt).sort_inside);
  CHECK(!plan_single_pass(s, 1000, 6001, true, false, dflt).sort_inside);
  CHECK(!plan_single_pass(s, 1000, 6000, false, false, dflt).sort_inside);
  CHECK(!plan_single_pass(s, 1000, 6000, true, true, dflt).sort_inside);
  CHECK(!plan_single_pass(multi, 786432, 786432, true, false, dflt).sort_inside);
  CHECK(plan_single_pass(multi, 786432, 786432, true, false, no_ms).sort_inside);
  CHECK(plan_single_pass(s, 786432, 786432, true, false, dflt).sort_inside);  // (the pipe route orders lists itself)

  // bivx_self_overlaps_dev
  CHECK(!plan_self_overlaps(s, 61439, dflt));
  CHECK(plan_self_overlaps(s, 61440, dflt));
  CHECK(plan_self_overlaps(s, 62914560, dflt));
  CHECK(!plan_self_overlaps(s, 62914561, dflt));
  CHECK(plan_self_overlaps(s, 1000, forced));
  CHECK(!plan_self_overlaps(s, 62914561, forced));
  CHECK(!plan_self_overlaps(s, 61440, never));
  CHECK(!plan_self_overlaps(multi, 61440, dflt));
  CHECK(!plan_self_overlaps(filt, 61440, dflt));
  {
    RouteShape hot = s;
    hot.max_cell = 65;
    CHECK(!plan_self_overlaps(hot, 61440, forced));  // (no exception for hotspots here)
  }

  // the knobs, parsed as atoi / atol with range checks
  unsetenv("BIVX_PIPE");
  unsetenv("BIVX_PIPE_MS");
  unsetenv("BIVX_PIPE_WGS");
  unsetenv("BIVX_MAX_TILES_PER_LAUNCH");
  unsetenv("BIVX_PREFIX_WAIT_LOG2");
  {
    const RouteKnobs k = read_route_knobs();
    CHECK(k.pipe == 1 && k.ms && k.wgs == 0 && k.max_tiles == 0 && k.wait_log2 == 0);
  }
  setenv("BIVX_PIPE", "2", 1);
  setenv("BIVX_PIPE_MS", "0", 1);
  setenv("BIVX_PIPE_WGS", "300", 1);
  setenv("BIVX_MAX_TILES_PER_LAUNCH", "3", 1);
  setenv("BIVX_PREFIX_WAIT_LOG2", "1", 1);
  {
    const RouteKnobs k = read_route_knobs();
    CHECK(k.pipe == 2 && !k.ms && k.wgs == 300 && k.max_tiles == 3 && k.wait_log2 == 1);
  }
  setenv("BIVX_PIPE_MS", "1", 1);
  setenv("BIVX_PIPE_WGS", "0", 1);
  setenv("BIVX_PREFIX_WAIT_LOG2", "64", 1);
  {
    const RouteKnobs k = read_route_knobs();
    CHECK(k.ms && k.wgs == 0 && k.wait_log2 == 0);
  }
  setenv("BIVX_PIPE_WGS", "65537", 1);
  setenv("BIVX_PREFIX_WAIT_LOG2", "0", 1);
  CHECK(read_route_knobs().wgs == 0 && read_route_knobs().wait_log2 == 0);
  setenv("BIVX_PIPE_WGS", "65536", 1);
  setenv("BIVX_PREFIX_WAIT_LOG2", "63", 1);
  CHECK(read_route_knobs().wgs == 65536 && read_route_knobs().wait_log2 == 63);
  setenv("BIVX_PIPE_WGS", "-5", 1);
  setenv("BIVX_PREFIX_WAIT_LOG2", "-1", 1);
  CHECK(read_route_knobs().wgs == 0 && read_route_knobs().wait_log2 == 0);
  setenv("BIVX_PIPE", "0", 1);
  CHECK(read_route_knobs().pipe == 0);

  std::printf("%d passed, %d failed\n", g_pass, g_fail);
  return g_fail != 0;
}
