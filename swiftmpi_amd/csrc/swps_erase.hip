// Removing keys from the HBM shard: swps_erase, swps_prune.
//
// The reference's dense_hash_map shards are never erased from (parameter/sparsetable.h has no
// erase), so this is an extension.  Four stream-ordered stages on the dense row store:
//   mark   dead[r] = 1 for the rows to remove (the listed keys' rows, or a scan of the AdaGrad
//          accumulators against a threshold);
//   plan   an inclusive prefix sum of dead gives the survivor count M and, per row, its place
//          among the HOLES (dead rows < M) or the MOVERS (live rows >= M), both ascending;
//   copy   the k-th mover's row and row_key go into the k-th hole: sources >= M > destinations,
//          so the copy is in place and race-free, and at most min(#dead, M) rows move;
//   index  the slot arrays are refilled with 0xFF and the M rows re-inserted (table_rebuild_index).
// No tombstones: the table has no spare key value (0 and 2^64 - 2 are legal keys), and a tombstone
// in slot_row would change k_find_or_insert, which every training step runs.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "swps_internal.h"
#include "swps_scan.h"

using namespace swps;

namespace {

struct DeadToCount {
  __host__ __device__ uint32_t operator()(uint8_t d) const { return d ? 1u : 0u; }
};

// the listed keys' rows (kNoRow: a key the shard lacks, or ~0) -> dead flags; the same row may be
// listed many times: the store is idempotent
__global__ __launch_bounds__(256) void k_erase_mark(const uint32_t *__restrict__ rows_idx, uint64_t n, uint32_t nrows,
                                                    uint8_t *__restrict__ dead) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = rows_idx[i];
  if (r < nrows) dead[r] = 1;
}

// swps_prune's mark, W2V rows: one wave per row over the accumulator half [2D, 4D) of the row.
// A row is cold when every element is <= thr.  Each lane keeps "saw an element that is not <= thr"
// (a NaN element is such an element, so the row is kept); the wave ORs the flags.  That is the
// running max and NaN flag of the row reduced across the wave, with no max ever formed: exact and
// order-free.  V: uint4 lanes when the half starts and ends on 16 B, else one element per lane.
template <typename T, bool V>
__global__ __launch_bounds__(256) void k_prune_mark_w2v(const T *__restrict__ rows, uint32_t nrows, int D, double thr,
                                                        uint8_t *__restrict__ dead) {
  const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= nrows) return;
  const T *acc = rows + w * 4 * (uint64_t)D + 2 * (uint64_t)D;
  bool hot = false;
  if (V) {
    constexpr int E = 16 / sizeof(T);
    struct alignas(16) P {
      T v[E];
    };
    const int nv = 2 * D / E;
    for (int c = lane; c < nv; c += 64) {
      const P p = ((const P *)acc)[c];
#pragma unroll
      for (int k = 0; k < E; k++) hot |= !((double)p.v[k] <= thr);
    }
  } else {
    for (int e = lane; e < 2 * D; e += 64) hot |= !((double)acc[e] <= thr);
  }
  const bool any_hot = __ballot(hot) != 0;
  if (lane == 0) dead[w] = any_hot ? 0 : 1;
}

// LR rows [w | grad2sum]: one thread per row
template <typename T>
__global__ __launch_bounds__(256) void k_prune_mark_lr(const T *__restrict__ rows, uint32_t nrows, double thr,
                                                       uint8_t *__restrict__ dead) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  dead[r] = (double)rows[2 * r + 1] <= thr ? 1 : 0;
}

// scan[r] = dead rows in [0, r].  Row r < M that is dead is hole number scan[r] - 1; row r >= M
// that lives is mover number (live rows in [M, r]) - 1.
__global__ __launch_bounds__(256) void k_erase_plan(const uint8_t *__restrict__ dead, const uint32_t *__restrict__ scan,
                                                    uint32_t nrows, uint32_t M, uint32_t *__restrict__ src,
                                                    uint32_t *__restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows) return;
  const uint32_t r = (uint32_t)i;
  const bool d = dead[r] != 0;
  if (r < M) {
    if (d) dst[scan[r] - 1] = r;
  } else if (!d) {
    const uint32_t below = M ? scan[M - 1] : 0u;  // the holes: as many as there are movers
    src[(r - M + 1) - (scan[r] - below) - 1] = r;
  }
}

// one wave per move: row src[k] -> row dst[k] (16-B, 4-B or byte lanes by row width), row_key too.
// The launch covers an upper bound of the moves (min(#dead, M), known on the host); the count
// itself, scan[M - 1], is read here so the host needs no second sync for it.
__global__ __launch_bounds__(256) void k_erase_move(const uint32_t *__restrict__ src, const uint32_t *__restrict__ dst,
                                                    const uint32_t *__restrict__ scan, uint32_t M, uint64_t bound,
                                                    char *__restrict__ rows, uint64_t rb,
                                                    uint64_t *__restrict__ row_key) {
  const uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const uint32_t H = M ? scan[M - 1] : 0u;
  if (k >= bound || k >= H) return;
  const uint32_t s = src[k], d = dst[k];
  const char *from = rows + (uint64_t)s * rb;
  char *to = rows + (uint64_t)d * rb;
  if (rb % 16 == 0) {
    for (uint64_t c = lane; c < rb / 16; c += 64) ((uint4 *)to)[c] = ((const uint4 *)from)[c];
  } else if (rb % 4 == 0) {
    for (uint64_t c = lane; c < rb / 4; c += 64) ((uint32_t *)to)[c] = ((const uint32_t *)from)[c];
  } else {
    for (uint64_t c = lane; c < rb; c += 64) to[c] = from[c];
  }
  if (lane == 0) row_key[d] = row_key[s];
}

// Before the mark: the table must be free of contexts; every async call has retired; the real row
// count (clamped as table_move clamps it) sizes a zeroed dead array.
int erase_begin(swps_table *t, uint32_t *cnt, uint32_t *nrows, hipStream_t s) {
  if (t->pins)
    return fail(SWPS_E_STATE, "an app context holds this table's row indices (from its init to its destroy): no "
                              "key can be removed meanwhile");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  SWPS_HIP(hipDeviceSynchronize());  // async calls may have used caller streams
  SWPS_HIP(hipMemcpy(cnt, t->counters.p, 4, hipMemcpyDeviceToHost));
  const uint64_t N = std::min<uint64_t>(*cnt, t->cfg.capacity);
  if (N >= (1ULL << 31)) return fail(SWPS_E_UNSUPPORTED, "erase on a shard of 2^31 rows or more");
  *nrows = (uint32_t)N;
  SWPS_TRY(t->er_dead.ensure(std::max<uint64_t>(N, 1)));
  if (N) SWPS_HIP(hipMemsetAsync(t->er_dead.p, 0, N, s));
  return SWPS_OK;
}

// plan, copy, index and the host state, from the dead flags of rows [0, N)
int erase_commit(swps_table *t, uint32_t cnt, uint32_t N, uint64_t *erased, hipStream_t s) {
  uint32_t ndead = 0;
  uint32_t *scan = nullptr;
  if (N) {
    SWPS_TRY(t->er_scan.ensure((uint64_t)N * 4));
    scan = t->er_scan.as<uint32_t>();
    hipcub::TransformInputIterator<uint32_t, DeadToCount, const uint8_t *> in(t->er_dead.as<const uint8_t>(),
                                                                              DeadToCount());
    SWPS_TRY(inclusive_scan(in, scan, N, t->er_tmp, s));
    SWPS_HIP(hipMemcpyAsync(&ndead, scan + (N - 1), 4, hipMemcpyDeviceToHost, s));
    SWPS_HIP(hipStreamSynchronize(s));  // the call's one wait for its own work before the commit
  }
  if (erased) *erased = ndead;
  const uint32_t M = N - ndead;
  if (ndead == 0 && cnt == N) {  // nothing to remove and no overflow to repair: the table is as it was
    t->host_nrows = N;
    t->rows_bound = N;
    t->ins_pending = t->ins_mixed = false;
    return SWPS_OK;
  }
  const uint64_t bound = std::min<uint32_t>(ndead, M);
  if (bound) {
    SWPS_TRY(t->er_src.ensure(bound * 4));
    SWPS_TRY(t->er_dst.ensure(bound * 4));
    k_erase_plan<<<nblk(N), 256, 0, s>>>(t->er_dead.as<const uint8_t>(), scan, N, M, t->er_src.as<uint32_t>(),
                                         t->er_dst.as<uint32_t>());
    SWPS_HIP(hipGetLastError());
    k_erase_move<<<nblk(bound * 64), 256, 0, s>>>(t->er_src.as<uint32_t>(), t->er_dst.as<uint32_t>(), scan, M, bound,
                                                  t->rows.as<char>(), (uint64_t)t->row_elems * t->esize,
                                                  t->row_key.as<uint64_t>());
    SWPS_HIP(hipGetLastError());
  }
  SWPS_HIP(hipMemcpyAsync(t->counters.p, &M, 4, hipMemcpyHostToDevice, s));
  SWPS_TRY(table_rebuild_index(t, M, s));
  SWPS_HIP(hipStreamSynchronize(s));  // M outlives its copy; the caller may use any stream next
  t->host_nrows = M;
  t->rows_bound = M;
  t->ins_pending = t->ins_mixed = false;
  return SWPS_OK;
}

}  // namespace

namespace swps {

int table_erase_keys(swps_table *t, const uint64_t *d_keys, uint64_t n, uint64_t *erased, hipStream_t s) {
  if (erased) *erased = 0;
  if (n >= (1ULL << 32)) return fail(SWPS_E_UNSUPPORTED, "more than 2^32 keys in one erase");
  uint32_t cnt = 0, N = 0;
  SWPS_TRY(erase_begin(t, &cnt, &N, s));
  if (n && N) {
    SWPS_TRY(t->er_rows.ensure(n * 4));
    SWPS_TRY(table_probe(t, d_keys, n, t->er_rows.as<uint32_t>(), s));
    k_erase_mark<<<nblk(n), 256, 0, s>>>(t->er_rows.as<uint32_t>(), n, N, t->er_dead.as<uint8_t>());
    SWPS_HIP(hipGetLastError());
  }
  return erase_commit(t, cnt, N, erased, s);
}

}  // namespace swps

extern "C" {

int swps_erase(swps_table *t, const uint64_t *d_keys, uint64_t n, uint64_t *erased) {
  if (!t || (n && !d_keys)) return fail(SWPS_E_CFG, "null argument");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  if (t->comm) return routed_erase(t, d_keys, n, erased, t->stream);
  return table_erase_keys(t, d_keys, n, erased, t->stream);
}

int swps_erase_h(swps_table *t, const uint64_t *keys, uint64_t n, uint64_t *erased) {
  if (!t || (n && !keys)) return fail(SWPS_E_CFG, "null argument");
  if (t->comm) return fail(SWPS_E_UNSUPPORTED, "swps_erase_h on a routed table");
  if (n >= (1ULL << 32)) return fail(SWPS_E_UNSUPPORTED, "more than 2^32 keys in one erase");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  DevMem dk;
  SWPS_TRY(dk.ensure(std::max<uint64_t>(n, 1) * 8));
  if (n) SWPS_HIP(hipMemcpy(dk.p, keys, n * 8, hipMemcpyHostToDevice));
  return table_erase_keys(t, dk.as<uint64_t>(), n, erased, t->stream);  // syncs before dk goes out of scope
}

int swps_prune(swps_table *t, double max_g2, uint64_t *erased) {
  if (!t) return fail(SWPS_E_CFG, "null table");
  if (erased) *erased = 0;
  if (max_g2 != max_g2) return fail(SWPS_E_CFG, "max_g2 is NaN");
  if (t->cfg.push_rule != SWPS_PUSH_ADAGRAD)
    return fail(SWPS_E_UNSUPPORTED, "swps_prune reads the AdaGrad accumulators: an SWPS_PUSH_SGD table never "
                                    "writes them");
  hipStream_t s = t->stream;
  uint32_t cnt = 0, N = 0;
  SWPS_TRY(erase_begin(t, &cnt, &N, s));
  if (N) {
    uint8_t *dead = t->er_dead.as<uint8_t>();
    const int D = t->cfg.dim;
    if (t->cfg.layout == SWPS_LAYOUT_W2V) {
      const unsigned nb = nblk((uint64_t)N * 64);
      if (t->cfg.dtype == SWPS_F64)  // 16 D bytes in front of the half, 16 D bytes of it
        k_prune_mark_w2v<double, true><<<nb, 256, 0, s>>>(t->rows.as<double>(), N, D, max_g2, dead);
      else if (D % 2 == 0)  // 8 D bytes in front of the half, 8 D bytes of it
        k_prune_mark_w2v<float, true><<<nb, 256, 0, s>>>(t->rows.as<float>(), N, D, max_g2, dead);
      else
        k_prune_mark_w2v<float, false><<<nb, 256, 0, s>>>(t->rows.as<float>(), N, D, max_g2, dead);
    } else if (t->cfg.dtype == SWPS_F64) {
      k_prune_mark_lr<double><<<nblk(N), 256, 0, s>>>(t->rows.as<double>(), N, max_g2, dead);
    } else {
      k_prune_mark_lr<float><<<nblk(N), 256, 0, s>>>(t->rows.as<float>(), N, max_g2, dead);
    }
    SWPS_HIP(hipGetLastError());
  }
  return erase_commit(t, cnt, N, erased, s);
}

}  // extern "C"
