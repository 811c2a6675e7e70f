/* A caller whose queries already live on the GPU, with an index sharded over several devices (include/bivx.h,
 * bivx_query_sharded_dev_q): the query columns are hipMalloc'ed on devices[0], the handle routes them to their chromosomes'
 * devices on the GPU and leaves the canonical CSR in batch order in devices[0]'s memory — what bivx_query_dev_s gives on
 * one device. The handle names device 0 twice (two shards on one card); every list is checked against a brute-force scan.
 * Exit status 0 and "sharded_device_queries: ok" on success, 3 without a GPU. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "bivx.h"

#define NCHROM 3u   /* chromosomes with intervals; queries also ask for chromosome 3, which nobody holds */
#define PER 2000u   /* intervals per chromosome */
#define Q 5000u

#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      printf(__VA_ARGS__);        \
      printf("\n");               \
      return 1;                   \
    }                             \
  } while (0)

int main(void) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    printf("sharded_device_queries: no GPU\n");
    return 3;
  }
  static uint32_t chrom[NCHROM * PER], low[NCHROM * PER], high[NCHROM * PER];
  static uint32_t qc[Q], ql[Q], qh[Q];
  for (uint32_t i = 0; i < NCHROM * PER; ++i) {
    chrom[i] = i % NCHROM; /* chromosomes interleaved in append order */
    low[i] = (i * 7919u) % 20000u;
    high[i] = low[i] + (i % 50u);
  }
  for (uint32_t i = 0; i < Q; ++i) {
    qc[i] = (i * 13u) % (NCHROM + 1u);
    ql[i] = (i * 104729u) % 20000u;
    qh[i] = ql[i] + (i % 30u);
  }
  const int devices[2] = {0, 0};
  bivx_index *idx = NULL;
  CHECK(bivx_create_sharded(&idx, devices, 2) == 0, "bivx_create_sharded: %s", bivx_last_error());
  CHECK(bivx_append(idx, chrom, low, high, NCHROM * PER) == 0, "bivx_append: %s", bivx_last_error());
  CHECK(bivx_build(idx) == 0, "bivx_build: %s", bivx_last_error());

  uint32_t *d_qc = NULL, *d_ql = NULL, *d_qh = NULL;
  CHECK(hipMalloc((void **)&d_qc, Q * 4) == hipSuccess && hipMalloc((void **)&d_ql, Q * 4) == hipSuccess &&
            hipMalloc((void **)&d_qh, Q * 4) == hipSuccess,
        "hipMalloc failed");
  CHECK(hipMemcpy(d_qc, qc, Q * 4, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_ql, ql, Q * 4, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_qh, qh, Q * 4, hipMemcpyHostToDevice) == hipSuccess,
        "hipMemcpy failed");

  bivx_sharded_result res;
  CHECK(bivx_query_sharded_dev_q(idx, d_qc, d_ql, d_qh, Q, 1, 1, &res, NULL) == 0, "bivx_query_sharded_dev_q: %s",
        bivx_last_error());
  CHECK(res.rows == Q && res.d_query_of_row == NULL && res.device == 0, "unexpected result shape");
  uint64_t *off = malloc((Q + 1) * sizeof(uint64_t));
  uint32_t *ids = malloc((res.total ? res.total : 1) * sizeof(uint32_t));
  CHECK(off && ids, "out of host memory");
  CHECK(hipMemcpy(off, res.d_offsets, (Q + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess, "hipMemcpy failed");
  if (res.total)
    CHECK(hipMemcpy(ids, res.d_hit_ids, res.total * 4, hipMemcpyDeviceToHost) == hipSuccess, "hipMemcpy failed");
  CHECK(off[0] == 0 && off[Q] == res.total, "offsets do not span the ids");
  uint64_t checked = 0;
  for (uint32_t i = 0; i < Q; ++i) { /* ascending ids: the brute-force scan's order */
    uint64_t at = off[i];
    for (uint32_t j = 0; j < NCHROM * PER; ++j) {
      if (chrom[j] != qc[i] || low[j] > qh[i] || ql[i] > high[j]) continue;
      CHECK(at < off[i + 1] && ids[at] == j, "query %u: list differs at id %u", i, j);
      ++at;
    }
    CHECK(at == off[i + 1], "query %u: %llu ids, expected %llu", i, (unsigned long long)(off[i + 1] - off[i]),
          (unsigned long long)(at - off[i]));
    checked += at - off[i];
  }
  printf("sharded_device_queries: ok (%u queries, %llu ids)\n", Q, (unsigned long long)checked);
  free(off);
  free(ids);
  (void)hipFree(d_qc);
  (void)hipFree(d_ql);
  (void)hipFree(d_qh);
  bivx_destroy(idx);
  return 0;
}
