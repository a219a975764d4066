// The count-min gate of the inserting lookups: the one helper swps_lookup
// (swps_dup.hip) and swps_lookup_bag (swps_bag.hip) call in place of table_find_or_insert on a
// table with admission on.  The rule is part of the ABI (include/swps.h).
//
// Two one-thread-per-key kernels with the kernel boundary between them as the only dependency: the
// ADD pass raises the cells of every absent key (saturating, by compare-and-swap: the result is
// the saturating sum in whatever order the threads run), the TEST pass reads the finished cells.
// No thread waits on another.  The admitted keys are compacted by a scan, so they keep their
// first-occurrence order and an SWPS_INIT_FLCG table draws in it.
#pragma once
#include "swps_internal.h"
#include "swps_scan.h"

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"

namespace {
using namespace swps;

__device__ __forceinline__ uint64_t admit_cell(uint64_t seed, uint64_t width, int j, uint64_t key) {
  return (uint64_t)j * width + (fmix64(key ^ fmix64(seed + (uint64_t)j)) & (width - 1));
}

// every key without a row: cells[cell(j, key)] = min(2^32 - 1, cells[...] + min(count, min_count))
__global__ __launch_bounds__(256) void k_admit_add(const uint64_t *__restrict__ uniq,
                                                   const uint32_t *__restrict__ count,
                                                   const uint32_t *__restrict__ row_u, uint64_t nu, uint32_t *cells,
                                                   uint64_t width, uint64_t seed, uint32_t min_count) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nu || row_u[u] != kNoRow) return;
  const uint64_t key = uniq[u];
  const uint32_t c = count[u], inc = c < min_count ? c : min_count;
  uint32_t *p[SWPS_ADMIT_DEPTH];
  uint32_t cur[SWPS_ADMIT_DEPTH];
#pragma unroll
  for (int j = 0; j < SWPS_ADMIT_DEPTH; j++) {
    p[j] = cells + admit_cell(seed, width, j, key);
    cur[j] = __hip_atomic_load(p[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int j = 0; j < SWPS_ADMIT_DEPTH; j++) {
    while (cur[j] != 0xFFFFFFFFu) {  // a saturated cell stays saturated: nothing to add
      const uint32_t sum = cur[j] + inc, nv = sum < cur[j] ? 0xFFFFFFFFu : sum;
      if (__hip_atomic_compare_exchange_weak(p[j], &cur[j], nv, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
        break;  // a lost exchange left the cell's value in cur[j]: try again from it
    }
  }
}

// flags[u] = (no row) << 32 | (no row and min_j cells[cell(j, key)] >= min_count): one scan of the
// packed word numbers the admitted keys and counts the tested ones
__global__ __launch_bounds__(256) void k_admit_test(const uint64_t *__restrict__ uniq,
                                                    const uint32_t *__restrict__ row_u, uint64_t nu,
                                                    const uint32_t *__restrict__ cells, uint64_t width,
                                                    uint64_t seed, uint32_t min_count, uint64_t *__restrict__ flags) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nu) return;
  uint64_t f = 0;
  if (row_u[u] == kNoRow) {
    const uint64_t key = uniq[u];
    uint32_t est = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < SWPS_ADMIT_DEPTH; j++) {
      const uint32_t v = cells[admit_cell(seed, width, j, key)];
      est = v < est ? v : est;
    }
    f = (1ULL << 32) | (est >= min_count ? 1u : 0u);
  }
  flags[u] = f;
}

// inc = the inclusive scan of flags: the admitted key u is number (uint32)inc[u] - 1
__global__ __launch_bounds__(256) void k_admit_compact(const uint64_t *__restrict__ uniq,
                                                       const uint64_t *__restrict__ flags,
                                                       const uint64_t *__restrict__ inc, uint64_t nu,
                                                       uint64_t *__restrict__ adm_keys, uint32_t *__restrict__ adm_idx) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nu || !(flags[u] & 1)) return;
  const uint32_t i = (uint32_t)inc[u] - 1;
  adm_keys[i] = uniq[u];
  adm_idx[i] = (uint32_t)u;
}

__global__ __launch_bounds__(256) void k_admit_rows(const uint32_t *__restrict__ adm_idx,
                                                    const uint32_t *__restrict__ adm_rows, uint64_t na,
                                                    uint32_t *__restrict__ row_u) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < na) row_u[adm_idx[i]] = adm_rows[i];
}

// The gated insert of the distinct keys uniq[nu] (first-occurrence order, count[u] non-padding
// occurrences each): row_u[u] = the key's row, kNoRow for a refused key.  Keys the shard holds are
// untouched by the gate; the admitted list goes through table_find_or_insert exactly as swps_pull
// of that list would (init rule, growth bound, SWPS_E_OOM latch), and the return value is that
// call's.  One host read (the tested and admitted counts) beside the insert's own.
int admit_insert(swps_table *t, const uint64_t *uniq, const uint32_t *count, uint64_t nu, uint32_t *row_u,
                 hipStream_t s) {
  if (nu == 0) return SWPS_OK;
  if (nu >= (1ULL << 31)) return fail(SWPS_E_UNSUPPORTED, "2^31 or more distinct keys in one gated lookup");
  SWPS_TRY(table_probe(t, uniq, nu, row_u, s));
  SWPS_TRY(t->adm_buf.ensure(nu * 32));
  uint64_t *flags = t->adm_buf.as<uint64_t>(), *inc = flags + nu, *adm_keys = inc + nu;
  uint32_t *adm_idx = (uint32_t *)(adm_keys + nu), *adm_rows = adm_idx + nu;
  uint32_t *cells = t->adm_cells.as<uint32_t>();
  k_admit_add<<<nblk(nu), 256, 0, s>>>(uniq, count, row_u, nu, cells, t->adm_width, t->cfg.seed, t->adm_min);
  SWPS_HIP(hipGetLastError());
  k_admit_test<<<nblk(nu), 256, 0, s>>>(uniq, row_u, nu, cells, t->adm_width, t->cfg.seed, t->adm_min, flags);
  SWPS_HIP(hipGetLastError());
  SWPS_TRY(inclusive_scan(flags, inc, nu, t->adm_scan, s));
  k_admit_compact<<<nblk(nu), 256, 0, s>>>(uniq, flags, inc, nu, adm_keys, adm_idx);
  SWPS_HIP(hipGetLastError());
  uint64_t total = 0;
  SWPS_HIP(hipMemcpyAsync(&total, inc + (nu - 1), 8, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  const uint64_t tested = total >> 32, na = total & 0xFFFFFFFFULL;
  t->adm_stat[0] += tested;
  t->adm_stat[1] += na;
  t->adm_stat[2] += tested - na;
  if (na == 0) return SWPS_OK;
  // a refusal before the insert kernel ran (a failed growth) must leave no stale row index behind
  SWPS_HIP(hipMemsetAsync(adm_rows, 0xFF, na * 4, s));
  const int rc = table_find_or_insert(t, adm_keys, na, adm_rows, s);
  const std::string msg = rc != SWPS_OK ? swps_last_error() : "";
  k_admit_rows<<<nblk(na), 256, 0, s>>>(adm_idx, adm_rows, na, row_u);
  SWPS_HIP(hipGetLastError());
  return rc != SWPS_OK ? fail(rc, msg) : SWPS_OK;
}

}  // namespace

#pragma clang diagnostic pop
