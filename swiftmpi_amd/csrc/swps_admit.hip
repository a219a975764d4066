// Admission by count on the HBM shard: the count-min sketch's life cycle.
//
// swps_table_set_admission allocates SWPS_ADMIT_DEPTH x width u32 cells beside the shard; the
// inserting lookups (swps_dup.hip, swps_bag.hip) gate their new keys on it through the helper of
// swps_admit.h.  The sketch is not part of the rows: growth, erase, save / restore and the snapshot
// checksum never see it; swps_admission_cells / _load are how a caller checkpoints it.
#include "swps_internal.h"

using namespace swps;

namespace {

// every cell >>= shift (1..31)
__global__ __launch_bounds__(256) void k_admit_decay(uint32_t *__restrict__ cells, uint64_t n, int shift) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) cells[i] = cells[i] >> shift;
}

int check_on(const swps_table *t) {
  if (!t) return fail(SWPS_E_CFG, "null table");
  if (t->adm_min <= 1) return fail(SWPS_E_STATE, "admission is off (swps_table_set_admission with min_count > 1 first)");
  return SWPS_OK;
}

}  // namespace

extern "C" {

int swps_table_set_admission(swps_table *t, uint32_t min_count, uint64_t width) {
  const bool on = min_count > 1;
  if (on && (width < (1ULL << 6) || width > (1ULL << 30) || (width & (width - 1))))
    return fail(SWPS_E_CFG, "admission width " + std::to_string(width) + " is not a power of two in [2^6, 2^30]");
  if (!t) return fail(SWPS_E_CFG, "null table");
  if (on && t->comm)
    return fail(SWPS_E_UNSUPPORTED, "swps_table_set_admission on a routed table (swps_table_route): the counts would "
                                    "have to travel with the routed pull");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  SWPS_HIP(hipDeviceSynchronize());  // async calls may have used caller streams
  t->adm_min = 0;
  t->adm_width = 0;
  t->adm_stat[0] = t->adm_stat[1] = t->adm_stat[2] = 0;
  t->adm_cells.release();
  if (!on) return SWPS_OK;
  const size_t bytes = (size_t)SWPS_ADMIT_DEPTH * width * 4;
  SWPS_TRY(t->adm_cells.alloc_exact(bytes));
  if (hipMemset(t->adm_cells.p, 0, bytes) != hipSuccess) {
    t->adm_cells.release();
    return fail(SWPS_E_HIP, "hipMemset of the admission sketch failed");
  }
  SWPS_HIP(hipDeviceSynchronize());
  t->adm_min = min_count;
  t->adm_width = width;
  return SWPS_OK;
}

int swps_admission_info(swps_table *t, uint64_t *out6) {
  if (!t || !out6) return fail(SWPS_E_CFG, "null argument");
  out6[0] = t->adm_min;
  out6[1] = t->adm_width;
  out6[2] = SWPS_ADMIT_DEPTH;
  out6[3] = t->adm_stat[0];
  out6[4] = t->adm_stat[1];
  out6[5] = t->adm_stat[2];
  return SWPS_OK;
}

int swps_admission_decay(swps_table *t, int32_t shift) {
  if (shift < 1 || shift > 32) return fail(SWPS_E_CFG, "admission decay shift must be 1..32 (32 clears)");
  SWPS_TRY(check_on(t));
  SWPS_HIP(hipSetDevice(t->cfg.device));
  SWPS_HIP(hipDeviceSynchronize());
  const uint64_t n = (uint64_t)SWPS_ADMIT_DEPTH * t->adm_width;
  if (shift == 32) {
    SWPS_HIP(hipMemsetAsync(t->adm_cells.p, 0, n * 4, t->stream));
  } else {
    k_admit_decay<<<nblk(n), 256, 0, t->stream>>>(t->adm_cells.as<uint32_t>(), n, shift);
    SWPS_HIP(hipGetLastError());
  }
  SWPS_HIP(hipStreamSynchronize(t->stream));
  return SWPS_OK;
}

int swps_admission_cells(swps_table *t, uint32_t *cells, uint64_t cap, uint64_t *n) {
  SWPS_TRY(check_on(t));
  const uint64_t m = (uint64_t)SWPS_ADMIT_DEPTH * t->adm_width;
  if (n) *n = m;
  if (!cells || cap < m) return fail(SWPS_E_CFG, "the admission sketch holds " + std::to_string(m) + " cells");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  SWPS_HIP(hipDeviceSynchronize());
  SWPS_HIP(hipMemcpy(cells, t->adm_cells.p, m * 4, hipMemcpyDeviceToHost));
  return SWPS_OK;
}

int swps_admission_load(swps_table *t, const uint32_t *cells, uint64_t n) {
  SWPS_TRY(check_on(t));
  const uint64_t m = (uint64_t)SWPS_ADMIT_DEPTH * t->adm_width;
  if (!cells || n != m) return fail(SWPS_E_CFG, "the admission sketch holds " + std::to_string(m) + " cells");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  SWPS_HIP(hipDeviceSynchronize());
  SWPS_HIP(hipMemcpy(t->adm_cells.p, cells, m * 4, hipMemcpyHostToDevice));
  return SWPS_OK;
}

}  // extern "C"
