// Pooled lookups on the HBM shard: one row per BAG of ids.
//
// swps_lookup_bag sums (or averages) the pull values of a bag's members in fp64 in the order fixed
// by include/swps.h and writes one row per bag; swps_push_bag gives every distinct key one step of
// the push rule with the terms its occurrences inherit from their bags' gradient rows.  Neither
// materialises a [n][elems] tensor: the forward reads the rows of the shard (or the routed pull's
// buffer) through the coalesce's maps, the backward is the (run, chunk) reduce of swps_dup.h with
// BagGrads as its gradient source.
//
// Bags are CSR offsets over positions; a bag longer than SWPS_DUP_CHUNK positions is cut into
// (bag, chunk) items by POSITION, so the items follow from the offsets alone (no key is read).
// No kernel here waits on another thread: every dependency is a kernel boundary.
#include "swps_dup.h"
#include "swps_admit.h"

using namespace swps;

namespace {

constexpr uint32_t kAbsentRow = 0xFFFFFFFEu;  // a member without a row (insert = 0): a zero row that counts
constexpr uint32_t kNoBag = 0xFFFFFFFFu;
constexpr int kInFlight = 4;  // row loads issued before the adds that consume them

// ---- offsets ------------------------------------------------------------------------------------
// first[0] = the first bag whose offsets break the CSR contract (first != 0, a decrease, last != n);
// first[0] was set to kNoBag
__global__ __launch_bounds__(256) void k_bag_check(const uint64_t *__restrict__ off, uint64_t nbags, uint64_t n,
                                                   uint32_t *first) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b > nbags) return;
  bool bad = false;
  if (b == 0 && off[0] != 0) bad = true;
  if (b < nbags && off[b + 1] < off[b]) bad = true;
  if (b == nbags && off[nbags] != n) bad = true;
  if (bad) atomicMin(first, (uint32_t)(b < nbags ? b : nbags - 1));
}

// chunks of the bags longer than one chunk of positions (0 for the others, and for offsets that
// k_bag_check refuses: nothing is launched from them)
__global__ __launch_bounds__(256) void k_bag_nchunk(const uint64_t *__restrict__ off, uint64_t nbags,
                                                    uint32_t *__restrict__ nchunk) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nbags) return;
  const uint64_t lo = off[b], hi = off[b + 1];
  uint32_t c = 0;
  if (hi > lo && hi - lo > kChunk && hi - lo < (1ULL << 32)) c = (uint32_t)((hi - lo + kChunk - 1) / kChunk);
  nchunk[b] = c;
}

// rowp[p]: the row a position reads: kNoRow for padding (not a member), kAbsentRow for a key without a
// row, else row_u[inv[p]] (row_u == nullptr: inv[p], a row of the routed pull's buffer)
__global__ __launch_bounds__(256) void k_bag_rows(const uint32_t *__restrict__ inv,
                                                  const uint32_t *__restrict__ row_u, uint64_t n,
                                                  uint32_t *__restrict__ rowp) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t u = inv[p];
  uint32_t r = kNoRow;
  if (u != kNoIdx) {
    r = row_u ? row_u[u] : u;
    if (r == kNoRow) r = kAbsentRow;
  }
  rowp[p] = r;
}

// bag_of[p] = the bag of position p (the last b with off[b] <= p: empty bags are stepped over);
// mcount[b] (zeroed; may be null) += 1 per member
__global__ __launch_bounds__(256) void k_bag_of(const uint64_t *__restrict__ off, uint64_t nbags,
                                                const uint64_t *__restrict__ keys, uint64_t n,
                                                uint32_t *__restrict__ bag_of, uint32_t *mcount) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  uint64_t lo = 0, hi = nbags;  // off[lo] <= p < off[hi]
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  bag_of[p] = (uint32_t)lo;
  if (mcount && keys[p] != kEmptyKey) atomicAdd(mcount + lo, 1u);
}

// ---- forward --------------------------------------------------------------------------------------
// One member's term joins the chain: the first member starts it (not 0.0 + term).
template <typename T, int E>
__device__ __forceinline__ void bag_add(double (&acc)[E], uint32_t &m, uint32_t r, const Pack<T, E> &x, bool weighted,
                                        double wp) {
  if (r == kNoRow) return;
#pragma unroll
  for (int k = 0; k < E; k++) {
    double v = r == kAbsentRow ? 0.0 : (double)x.v[k];
    if (weighted) v = v * wp;
    acc[k] = m ? acc[k] + v : v;
  }
  m++;
}

// The chain of elements [c*E, c*E + E) over positions [a, b) in ascending position; returns the
// member count.  The adds are a fixed chain but the loads are not ordered: kInFlight rows are
// requested before the first of their adds.  No branch around a load: padding and absent keys
// load row 0 and the value is selected.
template <typename T, int E, bool WAVE>
__device__ __forceinline__ uint32_t bag_chain(const T *__restrict__ rows, uint64_t RS,
                                              const uint32_t *__restrict__ rowp, const double *__restrict__ w,
                                              uint64_t a, uint64_t b, int c, double (&acc)[E]) {
  using PT = Pack<T, E>;
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < E; k++) acc[k] = 0.0;
  uint64_t p = a;
  for (; p + kInFlight <= b; p += kInFlight) {
    uint32_t r[kInFlight];
    double wp[kInFlight];
    PT x[kInFlight];
#pragma unroll
    for (int i = 0; i < kInFlight; i++) {
      r[i] = rowp[p + i];
      if (WAVE) r[i] = __builtin_amdgcn_readfirstlane(r[i]);
      wp[i] = w ? w[p + i] : 1.0;
    }
#pragma unroll
    for (int i = 0; i < kInFlight; i++)
      x[i] = *(const PT *)(rows + (uint64_t)(r[i] < kAbsentRow ? r[i] : 0) * RS + (uint64_t)c * E);
#pragma unroll
    for (int i = 0; i < kInFlight; i++) bag_add<T, E>(acc, m, r[i], x[i], w != nullptr, wp[i]);
  }
  for (; p < b; p++) {
    uint32_t r = rowp[p];
    if (WAVE) r = __builtin_amdgcn_readfirstlane(r);
    const PT x = *(const PT *)(rows + (uint64_t)(r < kAbsentRow ? r : 0) * RS + (uint64_t)c * E);
    bag_add<T, E>(acc, m, r, x, w != nullptr, w ? w[p] : 1.0);
  }
  return m;
}

// mean, the one cast to the table dtype, the store; m = 0: +0.0 and no division
template <typename T, int E>
__device__ __forceinline__ void bag_store(T *__restrict__ out, int c, double (&acc)[E], uint32_t m, int mode) {
  Pack<T, E> o;
#pragma unroll
  for (int k = 0; k < E; k++) {
    double v = acc[k];
    if (m == 0)
      v = 0.0;
    else if (mode == SWPS_BAG_MEAN)
      v = v / (double)m;
    o.v[k] = (T)v;
  }
  ((Pack<T, E> *)out)[c] = o;
}

// Bags of at most one chunk of positions: one wave per bag, lanes across the PV packs of the pull
// value (WAVE), or one thread per bag (narrow values: LR); accumulators in registers, one store.
template <typename T, int E, bool WAVE>
__global__ __launch_bounds__(256) void k_bag_short(const uint64_t *__restrict__ off, uint64_t nbags,
                                                   const uint32_t *__restrict__ rowp,
                                                   const double *__restrict__ w, const T *__restrict__ rows,
                                                   uint64_t RS, int PV, T *__restrict__ out, int mode) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t bag = WAVE ? tid >> 6 : tid;
  const int lane = WAVE ? (int)(threadIdx.x & 63) : 0;
  if (bag >= nbags) return;
  const uint64_t a = off[bag], b = off[bag + 1];
  if (b - a > kChunk) return;  // the (bag, chunk) items take it
  for (int c = lane; c < PV; c += WAVE ? 64 : 1) {
    double acc[E];
    const uint32_t m = bag_chain<T, E, WAVE>(rows, RS, rowp, w, a, b, c, acc);
    bag_store<T, E>(out + bag * (uint64_t)PV * E, c, acc, m, mode);
  }
}

// Longer bags, pass 1: one wave (thread) per (bag, chunk) item writes the chunk's fp64 partial and
// its member count.
template <typename T, int E, bool WAVE>
__global__ __launch_bounds__(256) void k_bag_partial(const uint32_t *__restrict__ item_bag,
                                                     const uint32_t *__restrict__ item_chunk, uint64_t nitems,
                                                     const uint64_t *__restrict__ off,
                                                     const uint32_t *__restrict__ rowp,
                                                     const double *__restrict__ w, const T *__restrict__ rows,
                                                     uint64_t RS, int PV, double *__restrict__ partial,
                                                     uint32_t *__restrict__ cnt) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t it = WAVE ? tid >> 6 : tid;
  const int lane = WAVE ? (int)(threadIdx.x & 63) : 0;
  if (it >= nitems) return;
  const uint32_t bag = item_bag[it];
  const uint64_t a = off[bag] + (uint64_t)item_chunk[it] * kChunk;
  const uint64_t e = off[bag + 1];
  const uint64_t b = a + kChunk < e ? a + kChunk : e;
  uint32_t m = 0;
  for (int c = lane; c < PV; c += WAVE ? 64 : 1) {
    double acc[E];
    m = bag_chain<T, E, WAVE>(rows, RS, rowp, w, a, b, c, acc);
    store_g<E>(partial + it * (uint64_t)PV * E, c, acc);
  }
  if (lane == 0) cnt[it] = m;  // PV >= 1: lane 0 ran the chain
}

// pass 2 (after pass 1 has completed: a kernel boundary): the wave of a bag's first item chains the
// non-empty partials in chunk order, from the first, and finishes as k_bag_short does
template <typename T, int E, bool WAVE>
__global__ __launch_bounds__(256) void k_bag_long(const uint32_t *__restrict__ item_bag,
                                                  const uint32_t *__restrict__ item_chunk, uint64_t nitems,
                                                  const uint64_t *__restrict__ off,
                                                  const double *__restrict__ partial,
                                                  const uint32_t *__restrict__ cnt, int PV, T *__restrict__ out,
                                                  int mode) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t it = WAVE ? tid >> 6 : tid;
  const int lane = WAVE ? (int)(threadIdx.x & 63) : 0;
  if (it >= nitems || item_chunk[it] != 0) return;
  const uint32_t bag = item_bag[it];
  const uint32_t nc = (uint32_t)((off[bag + 1] - off[bag] + kChunk - 1) / kChunk);
  using PD = Pack<double, E>;
  for (int c = lane; c < PV; c += WAVE ? 64 : 1) {
    double acc[E];
#pragma unroll
    for (int k = 0; k < E; k++) acc[k] = 0.0;
    uint32_t m = 0;
    for (uint32_t q = 0; q < nc; q++) {
      const uint32_t mq = cnt[it + q];
      if (!mq) continue;  // a chunk without members is skipped
      const PD p = ((const PD *)(partial + (it + q) * (uint64_t)PV * E))[c];
#pragma unroll
      for (int k = 0; k < E; k++) acc[k] = m ? acc[k] + p.v[k] : p.v[k];
      m += mq;
    }
    bag_store<T, E>(out + bag * (uint64_t)PV * E, c, acc, m, mode);
  }
}

// ---- host side ------------------------------------------------------------------------------------
// words of swps_table::dup[B_BAG]: a header, three per bag, one per position
struct BagScratch {
  uint32_t *head = nullptr;    // [0] the first bad bag, [1] the (bag, chunk) item count
  uint32_t *nchunk = nullptr;  // [nbags]
  uint32_t *cinc = nullptr;    // [nbags]
  uint32_t *mcount = nullptr;  // [nbags]
  uint32_t *pos = nullptr;     // [n]: rowp (forward) / bag_of (backward)
  uint64_t nitems = 0;
};

int bag_scratch(swps_table *t, uint64_t n, uint64_t nbags, BagScratch &B) {
  SWPS_TRY(t->dup[B_BAG].ensure((8 + 3 * nbags + n) * 4));
  B.head = t->dup[B_BAG].as<uint32_t>();
  B.nchunk = B.head + 8;
  B.cinc = B.nchunk + nbags;
  B.mcount = B.cinc + nbags;
  B.pos = B.mcount + nbags;
  return SWPS_OK;
}

// The offsets' check and the chunk counts of the long bags, queued on s; `rd` names the two words
// the caller's one host read has to bring along (nbags > 0).
int bag_prepare(swps_table *t, const uint64_t *d_off, uint64_t n, uint64_t nbags, BagScratch &B, uint32_t (&h)[2],
                HostRead &rd, hipStream_t s) {
  SWPS_HIP(hipMemsetAsync(B.head, 0xFF, 4, s));
  k_bag_check<<<nblk(nbags + 1), 256, 0, s>>>(d_off, nbags, n, B.head);
  SWPS_HIP(hipGetLastError());
  k_bag_nchunk<<<nblk(nbags), 256, 0, s>>>(d_off, nbags, B.nchunk);
  SWPS_HIP(hipGetLastError());
  SWPS_TRY(scan_u32(t, B.nchunk, B.cinc, nbags, s));
  SWPS_HIP(hipMemcpyAsync(B.head + 1, B.cinc + (nbags - 1), 4, hipMemcpyDeviceToDevice, s));
  h[0] = h[1] = 0;
  rd.d = B.head;
  rd.h = h;
  rd.words = 2;
  return SWPS_OK;
}

int bag_verdict(const uint32_t (&h)[2], BagScratch &B) {
  if (h[0] != kNoBag)
    return fail(SWPS_E_CFG, "bag offsets are not CSR (first 0, never decreasing, last n): first bad bag " +
                                std::to_string(h[0]));
  B.nitems = h[1];
  return SWPS_OK;
}

// coalesce + the bags' preparation with ONE host read; n == 0 reads the two words by itself
int bag_runs(swps_table *t, const uint64_t *d_keys, uint64_t n, const uint64_t *d_off, uint64_t nbags, bool items,
             BagScratch &B, Runs &R, hipStream_t s) {
  SWPS_TRY(bag_scratch(t, n, nbags, B));
  uint32_t h[2];
  HostRead rd;
  SWPS_TRY(bag_prepare(t, d_off, n, nbags, B, h, rd, s));
  if (n) {
    SWPS_TRY(sorted_runs(t, d_keys, n, s, items, R, &rd));
  } else {
    SWPS_HIP(hipMemcpyAsync(rd.h, rd.d, 8, hipMemcpyDeviceToHost, s));
    SWPS_HIP(hipStreamSynchronize(s));
  }
  return bag_verdict(h, B);
}

template <typename T, int E, bool WAVE>
int launch_bags(swps_table *t, const uint64_t *d_off, uint64_t nbags, const BagScratch &B, const double *w,
                const void *src, uint64_t RS, int PV, void *out, int mode, hipStream_t s) {
  const uint64_t per = WAVE ? 64 : 1;
  k_bag_short<T, E, WAVE><<<nblk(nbags * per), 256, 0, s>>>(d_off, nbags, B.pos, w, (const T *)src, RS, PV, (T *)out,
                                                           mode);
  SWPS_HIP(hipGetLastError());
  if (B.nitems) {
    const uint64_t ni = B.nitems;
    uint32_t *item_bag = t->dup[B_BAG_ITEMS].as<uint32_t>(), *item_chunk = item_bag + ni, *cnt = item_chunk + ni;
    double *partial = t->dup[B_BAG_PART].as<double>();
    k_dup_items<<<nblk(nbags), 256, 0, s>>>(B.nchunk, B.cinc, nbags, item_bag, item_chunk);
    SWPS_HIP(hipGetLastError());
    k_bag_partial<T, E, WAVE><<<nblk(ni * per), 256, 0, s>>>(item_bag, item_chunk, ni, d_off, B.pos, w,
                                                            (const T *)src, RS, PV, partial, cnt);
    SWPS_HIP(hipGetLastError());
    k_bag_long<T, E, WAVE><<<nblk(ni * per), 256, 0, s>>>(item_bag, item_chunk, ni, d_off, partial, cnt, PV, (T *)out,
                                                         mode);
    SWPS_HIP(hipGetLastError());
  }
  return SWPS_OK;
}

// out[b] = the pooled pull value of bag b from rows of row_bytes at src, B.pos = rowp.  Lanes run
// across 16-B packs when row stride, pull bytes and both bases allow, else scalar lanes (the rule
// of gather()); narrow values (LR) one thread per bag / item
int pool_bags(swps_table *t, const uint64_t *d_off, uint64_t nbags, const BagScratch &B, const double *w,
              const void *src, size_t row_bytes, void *out, int mode, hipStream_t s) {
  if (B.nitems) {
    SWPS_TRY(t->dup[B_BAG_ITEMS].ensure(B.nitems * 12));
    SWPS_TRY(t->dup[B_BAG_PART].ensure(B.nitems * (uint64_t)t->pull_elems * 8));
  }
  const size_t cb = (size_t)t->pull_elems * t->esize;
  const bool f64 = t->cfg.dtype == SWPS_F64;
  const int P = t->pull_elems;
  if (P <= 4 && cb < 16) {
    if (f64) return launch_bags<double, 1, false>(t, d_off, nbags, B, w, src, row_bytes / 8, P, out, mode, s);
    return launch_bags<float, 1, false>(t, d_off, nbags, B, w, src, row_bytes / 4, P, out, mode, s);
  }
  if (row_bytes % 16 == 0 && cb % 16 == 0 && aligned16(src) && aligned16(out)) {
    if (f64) return launch_bags<double, 2, true>(t, d_off, nbags, B, w, src, row_bytes / 8, P / 2, out, mode, s);
    return launch_bags<float, 4, true>(t, d_off, nbags, B, w, src, row_bytes / 4, P / 4, out, mode, s);
  }
  if (f64) return launch_bags<double, 1, true>(t, d_off, nbags, B, w, src, row_bytes / 8, P, out, mode, s);
  return launch_bags<float, 1, true>(t, d_off, nbags, B, w, src, row_bytes / 4, P, out, mode, s);
}

int check_bag_args(const swps_table *t, const void *keys, uint64_t n, const void *off, uint64_t nbags,
                   const void *weights, int32_t mode, const void *io) {
  if (mode != SWPS_BAG_SUM && mode != SWPS_BAG_MEAN) return fail(SWPS_E_CFG, "unknown bag mode");
  if (!t || (n && !keys) || (nbags && (!off || !io))) return fail(SWPS_E_CFG, "null argument");
  if (weights && mode == SWPS_BAG_MEAN) return fail(SWPS_E_CFG, "per-position weights with SWPS_BAG_MEAN");
  return SWPS_OK;
}

int check_bag_sizes(uint64_t n, uint64_t nbags) {
  SWPS_TRY(check_n(n));
  if (nbags >= (1ULL << 32)) return fail(SWPS_E_UNSUPPORTED, "2^32 or more bags in one call (bag indices are 32-bit)");
  if (nbags == 0 && n != 0) return fail(SWPS_E_CFG, "keys without bags (nbags == 0, n != 0)");
  return SWPS_OK;
}

int check_bag_push(const swps_table *t, int32_t gdtype) {
  if (t->cfg.layout == SWPS_LAYOUT_LR && gdtype != SWPS_F32)
    return fail(SWPS_E_CFG, "an LR table takes fp32 gradients (gdtype SWPS_F32)");
  return SWPS_OK;
}

// host arrays -> device staging of the _h forms (on the table's stream)
int stage_bag(swps_table *t, const uint64_t *keys, uint64_t n, const uint64_t *off, uint64_t nbags,
              const double *weights, DevMem &dk, DevMem &doff, DevMem &dw) {
  SWPS_TRY(dk.ensure(n * 8));
  SWPS_TRY(doff.ensure((nbags + 1) * 8));
  if (n) SWPS_HIP(hipMemcpyAsync(dk.p, keys, n * 8, hipMemcpyHostToDevice, t->stream));
  if (nbags) SWPS_HIP(hipMemcpyAsync(doff.p, off, (nbags + 1) * 8, hipMemcpyHostToDevice, t->stream));
  if (weights) {
    SWPS_TRY(dw.ensure(n * 8));
    if (n) SWPS_HIP(hipMemcpyAsync(dw.p, weights, n * 8, hipMemcpyHostToDevice, t->stream));
  }
  return SWPS_OK;
}

}  // namespace

extern "C" {

int swps_lookup_bag(swps_table *t, const uint64_t *d_keys, uint64_t n, const uint64_t *d_offsets, uint64_t nbags,
                    const double *d_weights, int32_t mode, int32_t insert, void *d_out, void *stream) {
  if (insert != 0 && insert != 1) return fail(SWPS_E_CFG, "insert must be 0 or 1");
  SWPS_TRY(check_bag_args(t, d_keys, n, d_offsets, nbags, d_weights, mode, d_out));
  SWPS_TRY(check_bag_sizes(n, nbags));
  if (t->comm && !insert) return fail(SWPS_E_UNSUPPORTED, "swps_lookup_bag without insert on a routed table");
  if (nbags == 0 && !t->comm) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : t->stream;
  BagScratch B;
  Runs R;
  uint64_t *uniq = nullptr;
  uint32_t *inv = nullptr, *count = nullptr;
  const bool gated = insert && !t->comm && t->adm_min > 1;  // admission by count
  if (nbags) SWPS_TRY(bag_runs(t, d_keys, n, d_offsets, nbags, false, B, R, s));  // refuses bad offsets here
  if (n) {
    SWPS_TRY(t->dup[B_UNIQ].ensure((R.nu + 1) * 8));
    SWPS_TRY(t->dup[B_INV].ensure(n * 4));
    uniq = t->dup[B_UNIQ].as<uint64_t>();
    inv = t->dup[B_INV].as<uint32_t>();
    if (gated) {
      SWPS_TRY(t->adm_cnt.ensure((R.nu + 1) * 4));
      count = t->adm_cnt.as<uint32_t>();
    }
    SWPS_TRY(rank_runs(t, R, uniq, inv, count, s));
  }
  if (t->comm) {  // collective: the routed pull of the distinct keys, pooled through inv
    const size_t cb = (size_t)t->pull_elems * t->esize;
    SWPS_TRY(t->dup[B_VALS].ensure((R.nu + 1) * cb));
    SWPS_TRY(routed_pull(t, uniq, R.nu, t->dup[B_VALS].p, s));
    if (nbags) {
      if (n) {
        k_bag_rows<<<nblk(n), 256, 0, s>>>(inv, nullptr, n, B.pos);
        SWPS_HIP(hipGetLastError());
      }
      SWPS_TRY(pool_bags(t, d_offsets, nbags, B, d_weights, t->dup[B_VALS].p, cb, d_out, mode, s));
    }
    return table_check_error(t, s);
  }
  int rc = SWPS_OK;
  std::string msg;
  if (n) {
    SWPS_TRY(t->dup[B_ROWS].ensure((R.nu + 1) * 4));
    uint32_t *row_u = t->dup[B_ROWS].as<uint32_t>();
    if (insert) {
      // exactly swps_lookup's insert of the distinct list; a failure (table full) still leaves the
      // found keys' rows, and the keys without one pool as zero rows; gated: the admitted keys only,
      // a refused key is such a zero row
      rc = gated ? admit_insert(t, uniq, count, R.nu, row_u, s) : table_find_or_insert(t, uniq, R.nu, row_u, s);
      if (rc != SWPS_OK && rc != SWPS_E_OOM && rc != SWPS_E_BADKEY) return rc;
      if (rc != SWPS_OK) msg = swps_last_error();
    } else {
      SWPS_TRY(table_probe(t, uniq, R.nu, row_u, s));
    }
    k_bag_rows<<<nblk(n), 256, 0, s>>>(inv, row_u, n, B.pos);
    SWPS_HIP(hipGetLastError());
  }
  SWPS_TRY(pool_bags(t, d_offsets, nbags, B, d_weights, t->rows.p, (size_t)t->row_elems * t->esize, d_out, mode, s));
  const int rc2 = table_check_error(t, s);
  if (rc != SWPS_OK) return fail(rc, msg);
  return rc2;
}

int swps_push_bag(swps_table *t, const uint64_t *d_keys, uint64_t n, const uint64_t *d_offsets, uint64_t nbags,
                  const double *d_weights, int32_t mode, const void *d_bag_grads, int32_t gdtype, double scale,
                  void *stream) {
  if (gdtype != SWPS_F32 && gdtype != SWPS_F64) return fail(SWPS_E_CFG, "gdtype must be SWPS_F32 or SWPS_F64");
  SWPS_TRY(check_bag_args(t, d_keys, n, d_offsets, nbags, d_weights, mode, d_bag_grads));
  SWPS_TRY(check_bag_push(t, gdtype));
  SWPS_TRY(check_bag_sizes(n, nbags));
  if (nbags == 0 && !t->comm) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : t->stream;
  BagScratch B;
  Runs R;
  uint64_t *rkeys = nullptr;
  BagArgs bag;
  if (nbags) SWPS_TRY(bag_runs(t, d_keys, n, d_offsets, nbags, true, B, R, s));  // refuses bad offsets here
  if (n) {
    SWPS_TRY(t->dup[B_UNIQ].ensure((R.nu + 1) * 8));
    rkeys = t->dup[B_UNIQ].as<uint64_t>();  // the distinct keys in key order, as in swps_push_dup
    if (R.nu) {
      k_dup_run_keys<<<nblk(R.nu), 256, 0, s>>>(R.ks, R.run_start, R.nu, rkeys);
      SWPS_HIP(hipGetLastError());
    }
    const bool mean = mode == SWPS_BAG_MEAN;
    if (mean) SWPS_HIP(hipMemsetAsync(B.mcount, 0, nbags * 4, s));
    k_bag_of<<<nblk(n), 256, 0, s>>>(d_offsets, nbags, d_keys, n, B.pos, mean ? B.mcount : nullptr);
    SWPS_HIP(hipGetLastError());
    bag.bag_of = B.pos;
    bag.w = d_weights;
    bag.m = mean ? B.mcount : nullptr;
  }
  if (t->comm) {  // collective: one reduced gradient per distinct key, then the routed push
    const size_t gb = (size_t)t->push_elems * (t->cfg.layout == SWPS_LAYOUT_W2V ? 8 : 4);
    SWPS_TRY(t->dup[B_VALS].ensure((R.nu + 1) * gb));
    if (R.nu)
      SWPS_TRY((reduce_runs<false, true>(t, R, d_bag_grads, gdtype, nullptr, t->dup[B_VALS].p, SWPS_REDUCE_SUM, scale, s,
                                         &bag)));
    SWPS_TRY(routed_push(t, rkeys, R.nu, t->dup[B_VALS].p, s));
    return table_check_error(t, s);
  }
  if (R.nu) {
    SWPS_TRY(t->dup[B_ROWS].ensure(R.nu * 4));
    uint32_t *row_r = t->dup[B_ROWS].as<uint32_t>();
    // an unknown key: latched, its run skipped; with admission on it is a refused id's gradient
    // and only skipped
    if (t->adm_min > 1)
      SWPS_TRY(table_probe(t, rkeys, R.nu, row_r, s));
    else
      SWPS_TRY(table_lookup(t, rkeys, R.nu, row_r, s));
    SWPS_TRY((reduce_runs<true, true>(t, R, d_bag_grads, gdtype, row_r, nullptr, SWPS_REDUCE_SUM, scale, s, &bag)));
  }
  return table_check_error(t, s);
}

int swps_lookup_bag_h(swps_table *t, const uint64_t *keys, uint64_t n, const uint64_t *offsets, uint64_t nbags,
                      const double *weights, int32_t mode, int32_t insert, void *out) {
  if (insert != 0 && insert != 1) return fail(SWPS_E_CFG, "insert must be 0 or 1");
  SWPS_TRY(check_bag_args(t, keys, n, offsets, nbags, weights, mode, out));
  SWPS_TRY(check_bag_sizes(n, nbags));
  if (nbags == 0 && !t->comm) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  const uint64_t m = nbags * (uint64_t)t->pull_elems;
  DevMem dk, doff, dw, dv;
  SWPS_TRY(stage_bag(t, keys, n, offsets, nbags, weights, dk, doff, dw));
  SWPS_TRY(dv.ensure(m * t->esize));
  const int rc = swps_lookup_bag(t, dk.as<uint64_t>(), n, doff.as<uint64_t>(), nbags, weights ? dw.as<double>() : nullptr,
                                 mode, insert, dv.p, nullptr);  // syncs
  if (rc != SWPS_OK && rc != SWPS_E_OOM && rc != SWPS_E_BADKEY) return rc;
  const std::string msg = rc != SWPS_OK ? swps_last_error() : "";
  const bool w2v = t->cfg.layout == SWPS_LAYOUT_W2V;
  const size_t out_es = w2v ? 8 : 4;
  if (t->esize == out_es) {
    if (m) SWPS_HIP(hipMemcpy(out, dv.p, m * out_es, hipMemcpyDeviceToHost));
  } else {
    std::vector<char> tmp(m * t->esize);
    if (m) SWPS_HIP(hipMemcpy(tmp.data(), dv.p, tmp.size(), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < m; i++) {
      if (w2v)
        ((double *)out)[i] = (double)((float *)tmp.data())[i];
      else
        ((float *)out)[i] = (float)((double *)tmp.data())[i];
    }
  }
  return rc != SWPS_OK ? fail(rc, msg) : SWPS_OK;
}

int swps_push_bag_h(swps_table *t, const uint64_t *keys, uint64_t n, const uint64_t *offsets, uint64_t nbags,
                    const double *weights, int32_t mode, const void *bag_grads, double scale) {
  SWPS_TRY(check_bag_args(t, keys, n, offsets, nbags, weights, mode, bag_grads));
  SWPS_TRY(check_bag_sizes(n, nbags));
  if (nbags == 0 && !t->comm) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  const bool w2v = t->cfg.layout == SWPS_LAYOUT_W2V;
  const size_t gb = nbags * (uint64_t)t->push_elems * (w2v ? 8 : 4);
  DevMem dk, doff, dw, dg;
  SWPS_TRY(stage_bag(t, keys, n, offsets, nbags, weights, dk, doff, dw));
  SWPS_TRY(dg.ensure(gb));
  if (gb) SWPS_HIP(hipMemcpyAsync(dg.p, bag_grads, gb, hipMemcpyHostToDevice, t->stream));
  return swps_push_bag(t, dk.as<uint64_t>(), n, doff.as<uint64_t>(), nbags, weights ? dw.as<double>() : nullptr, mode,
                       dg.p, w2v ? SWPS_F64 : SWPS_F32, scale, nullptr);  // syncs
}

}  // extern "C"
