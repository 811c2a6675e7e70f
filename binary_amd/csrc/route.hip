// route.hip — a device-resident batch split over the devices of a sharded handle (bivx_query_sharded_dev_q), and its
// gathered CSR put back into batch order, hand-written for gfx950.
//
// Routing is a stable multi-way partition of the queries by shard in three launches: every tile of 8 192 queries counts
// its queries per shard into a shard-major counts[shard][tile] array; one exclusive scan of that array (scan.hip) gives
// every (shard, tile) pair the place where its queries begin; every tile then scatters its queries there, ranked inside
// the tile in batch order by wavefront ballots and v_mbcnt. No workgroup waits for another (a single-pass
// look-back chain needs every predecessor resident). 12 bytes read and 16 written per query, 4 more read by the count.
#include "common.h"

namespace bivx {
namespace {

constexpr int kRThreads = 1024;
constexpr int kRWaves = kRThreads / kWave;
constexpr int kRItems = 8;
constexpr int kRTile = kRThreads * kRItems;  // 8 192 queries per workgroup (1 221 tiles at 10 M queries)
static_assert(kRouteMaxShards <= kWave, "one LDS slot per shard and lane, six bits of shard id in the ballots below");

__device__ __forceinline__ uint32_t shard_of(const uint8_t *__restrict__ table, uint32_t ntab, uint32_t c) {
  return c < ntab ? table[c] : 0u;  // (a chromosome beyond the table, 0xFFFFFFFF among them: shard 0)
}

// the lanes of the wavefront whose query goes to the same shard as this lane's (shard ids below 64: six ballots)
__device__ __forceinline__ uint64_t same_shard(uint32_t s, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const bool bit = (s >> b) & 1u;
    const uint64_t ones = __ballot(bit);
    m &= bit ? ones : ~ones;
  }
  return m;
}

// lanes of `m` below this one
__device__ __forceinline__ uint32_t rank_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(kRThreads) void k_route_count(const uint8_t *__restrict__ table, uint32_t ntab,
                                                           const uint32_t *__restrict__ qchrom, size_t q, uint32_t k,
                                                           uint32_t ntiles, uint32_t *__restrict__ counts) {
  __shared__ uint32_t h[kRouteMaxShards];
  if (threadIdx.x < kRouteMaxShards) h[threadIdx.x] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * kRTile;
#pragma unroll
  for (int it = 0; it < kRItems; ++it) {
    const size_t i = base + (size_t)it * kRThreads + threadIdx.x;
    const bool valid = i < q;
    const uint32_t c = valid && qchrom ? __builtin_nontemporal_load(qchrom + i) : 0u;
    const uint32_t s = valid ? shard_of(table, ntab, c) : 0u;
    const uint64_t m = same_shard(s, valid);
    if (valid && rank_below(m) == 0) atomicAdd(&h[s], (uint32_t)__popcll(m));  // one add per shard and wavefront
  }
  __syncthreads();
  if (threadIdx.x < k) counts[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// pos = the exclusive scan of counts (k * ntiles + 1 entries). Shard s's block of the output begins at row disp[s] = pos[s *
// ntiles] and holds n_s = disp[s + 1] - disp[s] queries as three columns [chrom | low | high] from word 3 disp[s] on; row r of
// the grouped result answers batch query query_of_row[r].
__global__ __launch_bounds__(kRThreads) void k_route_scatter(const uint8_t *__restrict__ table, uint32_t ntab,
                                                             const uint32_t *__restrict__ qchrom,
                                                             const uint32_t *__restrict__ qlow,
                                                             const uint32_t *__restrict__ qhigh, size_t q, uint32_t k,
                                                             uint32_t ntiles, const uint64_t *__restrict__ pos,
                                                             uint32_t *__restrict__ out, uint32_t *__restrict__ query_of_row,
                                                             uint64_t *__restrict__ disp) {
  __shared__ uint32_t wc[kRWaves][kRouteMaxShards];  // this round: queries per (wavefront, shard)
  __shared__ uint32_t run[kRouteMaxShards];          // queries of the tile's earlier rounds per shard
  __shared__ uint64_t first[kRouteMaxShards], dsp[kRouteMaxShards], len[kRouteMaxShards];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (threadIdx.x < k) {
    const uint64_t d0 = pos[(size_t)threadIdx.x * ntiles], d1 = pos[(size_t)(threadIdx.x + 1) * ntiles];
    dsp[threadIdx.x] = d0;
    len[threadIdx.x] = d1 - d0;
    first[threadIdx.x] = pos[(size_t)threadIdx.x * ntiles + blockIdx.x] - d0;
    run[threadIdx.x] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x <= k) disp[threadIdx.x] = pos[(size_t)threadIdx.x * ntiles];
  const size_t base = (size_t)blockIdx.x * kRTile;
  for (int it = 0; it < kRItems; ++it) {
    wc[wave][lane] = 0;
    __syncthreads();
    const size_t i = base + (size_t)it * kRThreads + threadIdx.x;
    const bool valid = i < q;
    uint32_t c = 0, lo = 0, hi = 0;
    if (valid) {
      c = qchrom ? __builtin_nontemporal_load(qchrom + i) : 0u;
      lo = __builtin_nontemporal_load(qlow + i);
      hi = __builtin_nontemporal_load(qhigh + i);
    }
    const uint32_t s = valid ? shard_of(table, ntab, c) : 0u;
    const uint64_t m = same_shard(s, valid);
    const uint32_t rank = rank_below(m);
    if (valid && rank == 0) wc[wave][s] = (uint32_t)__popcll(m);
    __syncthreads();
    if (valid) {
      uint64_t j = first[s] + run[s] + rank;  // the query's place inside its shard's block
      for (uint32_t w = 0; w < wave; ++w) j += wc[w][s];
      const uint64_t d = dsp[s], n = len[s];
      uint32_t *col = out + 3 * d;
      col[j] = c;
      col[n + j] = lo;
      col[2 * n + j] = hi;
      query_of_row[d + j] = (uint32_t)i;
    }
    __syncthreads();
    if (threadIdx.x < k) {
      uint32_t t = 0;
      for (int w = 0; w < kRWaves; ++w) t += wc[w][threadIdx.x];
      run[threadIdx.x] += t;
    }
    __syncthreads();  // (before the next round clears wc)
  }
}

__global__ __launch_bounds__(256) void k_iota(uint32_t *__restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (uint32_t)i;
}

// ---- the grouped CSR back in batch order ---------------------------------------------------------------------------------

// row r answers query query_of_row[r]: that query's list length and where its list begins in the grouped ids
__global__ __launch_bounds__(256) void k_rows_to_queries(const uint64_t *__restrict__ off, const uint32_t *__restrict__ query_of_row,
                                                         size_t rows, uint32_t *__restrict__ qlen, uint64_t *__restrict__ qsrc) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const uint64_t o0 = off[r], o1 = off[r + 1];
  const uint32_t qi = query_of_row[r];
  qlen[qi] = (uint32_t)(o1 - o0);
  qsrc[qi] = o0;
}

// query i's list: src_hits[qsrc[i] ..) of qoff[i + 1] - qoff[i] ids, to hits[qoff[i] ..). A wavefront takes 64 consecutive
// queries — one contiguous piece of the output — and every lane one output element at a time: the element's list is found
// by bisection of the 64 list ends in LDS, its source is a gather, the stores are a stream (a list of thousands of ids keeps
// all 64 lanes busy, 64 lists of three ids take one trip). Every element stored is one that was loaded; nothing else is
// written.
__global__ __launch_bounds__(256) void k_batch_lists(const uint64_t *__restrict__ qoff, const uint64_t *__restrict__ qsrc,
                                                     const uint32_t *__restrict__ src_hits, uint32_t *__restrict__ hits,
                                                     size_t n) {
  __shared__ uint32_t s_end[4][kWave];
  __shared__ uint64_t s_src[4][kWave];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t o0 = qoff[i < n ? i : n], o1 = qoff[i < n ? i + 1 : n];
  const uint64_t sp = i < n ? qsrc[i] : 0ull;
  const uint64_t wb = __shfl((unsigned long long)o0, 0, kWave);  // the wavefront's piece of the output: [wb, we)
  const uint64_t we = __shfl((unsigned long long)o1, kWave - 1, kWave);
  if (we - wb > 0xFFFFFFFFull) {  // (more than 2^32 ids in 64 lists: every lane copies its own)
    for (uint64_t e = 0; e < o1 - o0; ++e) hits[o0 + e] = src_hits[sp + e];
    return;
  }
  s_end[wave][lane] = (uint32_t)(o1 - wb);
  s_src[wave][lane] = sp - (o0 - wb);  // source of the list's first element, minus its place in the piece
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t total = (uint32_t)(we - wb);
  constexpr uint32_t kRowsPerTrip = 4;  // four bisections, then four gathers in flight, then four 256-byte row stores
  for (uint32_t e0 = lane; e0 < total; e0 += kWave * kRowsPerTrip) {
    uint32_t x[kRowsPerTrip];
#pragma unroll
    for (uint32_t r = 0; r < kRowsPerTrip; ++r) {
      const uint32_t e = e0 + r * kWave;
      uint32_t lo = 0, hi = kWave - 1;  // first list whose end is beyond e
#pragma unroll
      for (int step = 0; step < 6; ++step) {
        const uint32_t mid = (lo + hi) >> 1;
        const bool right = s_end[wave][mid] <= e;
        lo = right ? mid + 1 : lo;
        hi = right ? hi : mid;
      }
      const uint32_t owner = lo < kWave ? lo : kWave - 1;
      x[r] = e < total ? __builtin_nontemporal_load(src_hits + s_src[wave][owner] + e) : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < kRowsPerTrip; ++r) {
      const uint32_t e = e0 + r * kWave;
      if (e < total) __builtin_nontemporal_store(x[r], hits + wb + e);
    }
  }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

size_t route_scratch_bytes(size_t q, uint32_t k) {  // [counts: u32 k * ntiles | pos: u64 k * ntiles + 1 | scan scratch]
  const size_t cells = (size_t)k * ((q + kRTile - 1) / kRTile);
  return align256(cells * 4) + align256((cells + 1) * 8) + scan_scratch_bytes(cells);
}

int route_queries(const uint8_t *d_table, uint32_t ntab, const uint32_t *d_qchrom, const uint32_t *d_qlow,
                  const uint32_t *d_qhigh, size_t q, uint32_t k, uint32_t *d_out, uint32_t *d_query_of_row,
                  uint64_t *d_disp, void *d_scratch, hipStream_t s) {
  if (k < 1 || k > kRouteMaxShards || q > 0xFFFFFFFFull) {
    set_error("route_queries: %u shards, %zu queries", k, q);
    return BIVX_E_RANGE;
  }
  if (q == 0) {
    BIVX_HIP(hipMemsetAsync(d_disp, 0, (k + 1) * sizeof(uint64_t), s));
    return 0;
  }
  const uint32_t ntiles = (uint32_t)((q + kRTile - 1) / kRTile);
  const size_t cells = (size_t)k * ntiles;
  char *p = static_cast<char *>(d_scratch);
  uint32_t *counts = reinterpret_cast<uint32_t *>(p);
  uint64_t *pos = reinterpret_cast<uint64_t *>(p + align256(cells * 4));
  void *scan = p + align256(cells * 4) + align256((cells + 1) * 8);
  hipLaunchKernelGGL(k_route_count, dim3(ntiles), dim3(kRThreads), 0, s, d_table, ntab, d_qchrom, q, k, ntiles, counts);
  BIVX_HIP(hipGetLastError());
  BIVX_TRY(exclusive_scan_u32_u64(counts, pos, cells, scan, s));
  hipLaunchKernelGGL(k_route_scatter, dim3(ntiles), dim3(kRThreads), 0, s, d_table, ntab, d_qchrom, d_qlow, d_qhigh, q, k,
                     ntiles, (const uint64_t *)pos, d_out, d_query_of_row, d_disp);
  BIVX_HIP(hipGetLastError());
  return 0;
}

int launch_iota_u32(uint32_t *d_out, size_t n, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_iota, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_out, n);
  BIVX_HIP(hipGetLastError());
  return 0;
}

size_t batch_order_scratch_bytes(size_t q) {  // [lengths: u32 q | sources: u64 q | scan scratch]
  return align256(q * 4) + align256(q * 8) + scan_scratch_bytes(q);
}

int batch_order_csr(const uint64_t *d_row_off, const uint32_t *d_row_hits, const uint32_t *d_query_of_row, size_t q,
                    uint64_t *d_off, uint32_t *d_hits, void *d_scratch, hipStream_t s) {
  char *p = static_cast<char *>(d_scratch);
  uint32_t *qlen = reinterpret_cast<uint32_t *>(p);
  uint64_t *qsrc = reinterpret_cast<uint64_t *>(p + align256(q * 4));
  void *scan = p + align256(q * 4) + align256(q * 8);
  if (q) {
    hipLaunchKernelGGL(k_rows_to_queries, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, s, d_row_off, d_query_of_row, q,
                       qlen, qsrc);
    BIVX_HIP(hipGetLastError());
  }
  BIVX_TRY(exclusive_scan_u32_u64(qlen, d_off, q, scan, s));
  if (q) {
    hipLaunchKernelGGL(k_batch_lists, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, s, (const uint64_t *)d_off,
                       (const uint64_t *)qsrc, d_row_hits, d_hits, q);
    BIVX_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace bivx
