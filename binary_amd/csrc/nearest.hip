// nearest.hip — batched nearest-interval queries (bivx_nearest*, include/bivx.h), gfx950, wave64.
//
// The distance of query q and stored interval i on the same chromosome is d = max(0, q.low - high, low - q.high); the
// answer of q is the interval of smallest (d, id), or BIVX_NO_HIT when no interval has d <= max_dist. One lane per query,
// in two steps over the query's segments (one per length class of its chromosome, descriptors staged through LDS):
//   1. bound: per segment, one or two REAL intervals next to the query, read off the bucket directory — the first slot
//      of the cell after q.high's (every slot from there on starts beyond q.high) and the last slot of the cell before
//      q.low's. Any real interval's distance bounds the answer's: D = min(that, max_dist).
//   2. exact pass: d(q, i) <= D exactly when i overlaps the widened query [q.low - D, q.high + D] (saturated at 0 and
//      2^32 - 1), so seg_window of the widened query holds every interval that can be the answer. Each candidate's
//      (d << 32 | id) is evaluated and the minimum kept. Windows of up to kLight slots are read by their lane, longer
//      ones by the whole wavefront (coalesced rows, a wavefront-wide 64-bit minimum, a 64-ary trim above kTrim) — the
//      Mode::Any heavy path of enumerate_hits (query_device.h) with the distance in front of the id.
// Slots inside a directory cell are not ordered by low when the index is ordered by cell (IndexView::order_shift): the
// bound takes whichever interval a slot holds, and the pass evaluates whole cells, so neither depends on that order.
// The query kernels of query.hip / query_fused.hip / query_pipe.hip are not touched; the device code is shared through
// query_device.h and wave_device.h.
#include "query_device.h"

namespace bivx {
namespace {

constexpr uint64_t kNoBest = ~0ull;  // (d, id) key of "nothing yet": above every real key (ids are below 2^32 - 1)

// d(q, i) in exact unsigned arithmetic; 0 exactly when q.low <= high && low <= q.high
__device__ __forceinline__ uint32_t interval_dist(uint32_t lo, uint32_t hi, uint32_t low, uint32_t high) {
  const uint32_t left = lo > high ? lo - high : 0u;   // i lies before q
  const uint32_t right = low > hi ? low - hi : 0u;    // i lies after q
  return max(left, right);
}

__device__ __forceinline__ uint64_t dist_key(uint32_t d, uint32_t id) { return (uint64_t)d << 32 | id; }

// Step 1 for one segment: the distance of one or two real intervals next to [lo, hi] (UINT32_MAX: only if that is theirs).
__device__ __forceinline__ uint32_t seg_bound(const IndexView &v, const SegDesc &d, uint32_t lo, uint32_t hi) {
  const uint32_t sh = d.shift & 31u;
  const uint32_t *t = v.table + d.table_off;
  // first slot of the cell after q.high's (every slot there and beyond starts after q.high)
  const uint32_t r = hi < d.base ? d.begin : hi >= d.last ? d.end : t[((hi - d.base) >> sh) + 1u];
  // the slot before the first of q.low's cell (it starts before q.low)
  const uint32_t l = lo > d.last ? d.end : lo <= d.base ? d.begin : t[(lo - d.base) >> sh];
  const bool has_r = r < d.end, has_l = l > d.begin;
  // neither: every slot lies in the cells of [q.low, q.high], and the segment's first one is as good a bound as any
  const uint2 er = v.se[has_r ? r : d.begin];
  uint32_t b = interval_dist(lo, hi, er.x, er.y);
  if (has_l) {
    const uint2 el = v.se[l - 1u];
    b = min(b, interval_dist(lo, hi, el.x, el.y));
  }
  return b;
}

// (smallest (d, id) of the slots [a, b) of one lane's window, at most kLight of them; four loads of each kind in flight)
__device__ __forceinline__ uint64_t light_best(const IndexView &v, uint32_t a, uint32_t b, uint32_t lo, uint32_t hi,
                                               uint64_t best) {
#pragma unroll 1
  for (uint32_t j0 = a; j0 < b; j0 += 4u) {
    uint2 e[4];
    uint32_t idv[4];
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r)
      if (j0 + r < b) {
        e[r] = v.se[j0 + r];
        idv[r] = v.id[j0 + r];
      }
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r)
      if (j0 + r < b) best = min(best, dist_key(interval_dist(lo, hi, e[r].x, e[r].y), idv[r]));
  }
  return best;
}

// wavefront-wide minimum of 64-bit (d, id) keys (wavefront-uniform result)
__device__ __forceinline__ uint64_t wave_min_key(uint64_t k) {
  const uint32_t dmin = wave_min((uint32_t)(k >> 32));
  const uint32_t imin = wave_min((uint32_t)(k >> 32) == dmin ? (uint32_t)k : 0xFFFFFFFFu);
  return dist_key(dmin, imin);
}

template <bool LDS_DESC>
__global__ __launch_bounds__(kQThreads) void k_nearest(IndexView v, const uint32_t *__restrict__ qchrom,
                                                       const uint32_t *__restrict__ qlow,
                                                       const uint32_t *__restrict__ qhigh, size_t nq, uint32_t max_dist,
                                                       uint32_t *__restrict__ id_out, uint32_t *__restrict__ dist_out) {
  __shared__ SegDesc s_seg[LDS_DESC ? kLdsSegs : 1];
  __shared__ uint2 s_cs[LDS_DESC ? kLdsChroms : 1];
  const SegDesc *segs;
  const uint2 *cs;
  stage_descriptors<LDS_DESC>(v, s_seg, s_cs, segs, cs);
  if (LDS_DESC) __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const size_t q = (size_t)blockIdx.x * kQThreads + threadIdx.x;
  const bool valid = q < nq;
  const Query qy = load_query<false>(v, cs, qchrom, qlow, qhigh, q, valid);
  const uint32_t lo = qy.lo, hi = qy.hi;

  // ---- 1. the bound ----
  uint32_t bound = 0xFFFFFFFFu;
  for (uint32_t k = 0; k < qy.nseg; ++k) {
    const SegDesc d = load_seg(segs + qy.s0 + k);
    if (d.end > d.begin) bound = min(bound, seg_bound(v, d, lo, hi));
  }
  const uint32_t D = min(bound, max_dist);
  // the widened query: exactly the intervals with d <= D overlap it
  const uint32_t wlo = lo > D ? lo - D : 0u;
  const uint32_t whi = hi < 0xFFFFFFFFu - D ? hi + D : 0xFFFFFFFFu;

  // ---- 2. the exact pass over the widened query's windows (segment loop wavefront-uniform: the heavy path ballots) ----
  uint64_t best = kNoBest;
  for (uint32_t k = 0; __any(k < qy.nseg); ++k) {
    Window w{0u, 0u, 0u, 0u, false};
    uint32_t xlow = 0;
    if (k < qy.nseg) {
      const SegDesc d = load_seg(segs + qy.s0 + k);
      w = seg_window(v, d, wlo, whi);
      xlow = wlo > d.maxlen ? wlo - d.maxlen : 0u;
    }
    const bool nonempty = w.span != 0 && w.b > w.a;
    const bool heavy = nonempty && w.b - w.a > kLight;
    if (nonempty && !heavy) best = light_best(v, w.a, w.b, lo, hi, best);
    uint64_t hm = __ballot(heavy);
    while (hm) {
      const int src = __ffsll((long long)hm) - 1;
      hm &= hm - 1;
      auto of_src = [&](uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)x, src); };
      uint32_t ca = of_src(w.a), cb = of_src(w.b);
      const uint32_t cl = of_src(lo), ch = of_src(hi), cwh = of_src(whi);
      if (cb - ca > kTrim) {  // long window: trim it to the slots with low in [widened low - maxlen, widened high]
        uint32_t cbase = 0, gran = 0;
        if (v.order_shift) {  // (ordered by cell: trimmed to whole cells)
          const SegDesc *sd = segs + of_src(qy.s0) + k;
          cbase = sd->base;
          gran = sd->shift & 31u;
        }
        ca = wave_lower_bound_low(v.se, ca, cb, of_src(xlow), lane, cbase, gran);
        const uint32_t nx = gran ? (((cwh > cbase ? (cwh - cbase) >> gran : 0u) + 1u) << gran) + cbase : cwh + 1u;
        if (nx > cwh) cb = wave_lower_bound_low(v.se, ca, cb, nx, lane, cbase, gran);  // (no wrap past 2^32)
      }
      uint64_t m = kNoBest;
      for (uint32_t j0 = ca + lane; j0 < cb; j0 += kRows * kWave) {  // kRows rows of 64 slots in flight
        uint2 e[kRows];
        uint32_t idv[kRows];
#pragma unroll
        for (uint32_t r = 0; r < kRows; ++r)
          if (j0 + r * kWave < cb) {
            e[r] = v.se[j0 + r * kWave];
            idv[r] = v.id[j0 + r * kWave];
          }
#pragma unroll
        for (uint32_t r = 0; r < kRows; ++r)
          if (j0 + r * kWave < cb) m = min(m, dist_key(interval_dist(cl, ch, e[r].x, e[r].y), idv[r]));
      }
      m = wave_min_key(m);
      if (lane == src) best = min(best, m);
    }
  }
  if (!valid) return;
  const bool hit = best != kNoBest && (uint32_t)(best >> 32) <= max_dist;
  id_out[q] = hit ? (uint32_t)best : BIVX_NO_HIT;
  if (dist_out) dist_out[q] = hit ? (uint32_t)(best >> 32) : 0xFFFFFFFFu;
}

}  // namespace

int launch_nearest(const IndexView &v, const uint32_t *d_qchrom, const uint32_t *d_qlow, const uint32_t *d_qhigh,
                   size_t q, uint32_t max_dist, uint32_t *d_id, uint32_t *d_dist, hipStream_t s) {
  if (q == 0) return 0;
  const dim3 grid(tiles_for(q)), block(kQThreads);
  if (fits_lds(v))
    hipLaunchKernelGGL(k_nearest<true>, grid, block, 0, s, v, d_qchrom, d_qlow, d_qhigh, q, max_dist, d_id, d_dist);
  else
    hipLaunchKernelGGL(k_nearest<false>, grid, block, 0, s, v, d_qchrom, d_qlow, d_qhigh, q, max_dist, d_id, d_dist);
  BIVX_HIP(hipGetLastError());
  return 0;
}

}  // namespace bivx
