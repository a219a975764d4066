// The coalesce, the gather and the (run, chunk) reduce of the repeated-key calls:
// kernels and host helpers shared by swps_dup.hip and swps_bag.hip (§14).  Everything has internal
// linkage (an anonymous namespace): each unit carries the instantiations it launches.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "swps_internal.h"
#include "swps_sort.h"

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"

namespace {
using namespace swps;

constexpr uint32_t kNoIdx = 0xFFFFFFFFu;  // d_inv of a padding position
constexpr uint32_t kChunk = SWPS_DUP_CHUNK;

template <typename T, int E> struct alignas(sizeof(T) * E) Pack {
  T v[E];
};

// ---- coalesce ---------------------------------------------------------------------------------
// ks / ps: the (key, position) pairs sorted by key (stable: ascending position within a run; the
// padding key ~0 is the largest u64 and sorts last).
__global__ __launch_bounds__(256) void k_dup_flags(const uint64_t *__restrict__ ks, uint64_t n,
                                                   uint32_t *__restrict__ flags) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint64_t k = ks[j];
  flags[j] = (k != kEmptyKey && (j == 0 || ks[j - 1] != k)) ? 1u : 0u;
}

// inc = inclusive scan of the head flags: the run of sorted entry j is inc[j] - 1, the distinct
// count is inc[n - 1].  run_start[r] = first sorted entry of run r, run_start[nu] = the number of
// non-padding entries; head_pos[r] = the position of the run's first occurrence.
__global__ __launch_bounds__(256) void k_dup_heads(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ ps,
                                                   const uint32_t *__restrict__ flags,
                                                   const uint32_t *__restrict__ inc, uint64_t n,
                                                   uint32_t *__restrict__ run_start, uint32_t *__restrict__ head_pos) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  if (flags[j]) {
    run_start[inc[j] - 1] = (uint32_t)j;
    head_pos[inc[j] - 1] = ps[j];
  }
  if (ks[j] != kEmptyKey && (j == n - 1 || ks[j + 1] == kEmptyKey)) run_start[inc[j]] = (uint32_t)(j + 1);
}

// chunks of the runs longer than one chunk (0 for the others): the (run, chunk) items
__global__ __launch_bounds__(256) void k_dup_nchunk(const uint32_t *__restrict__ run_start,
                                                    const uint32_t *__restrict__ inc, uint64_t n,
                                                    uint32_t *__restrict__ nchunk) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  uint32_t c = 0;
  if (r < inc[n - 1]) {
    const uint32_t m = run_start[r + 1] - run_start[r];
    if (m > kChunk) c = (m + kChunk - 1) / kChunk;
  }
  nchunk[r] = c;
}

__global__ __launch_bounds__(256) void k_dup_items(const uint32_t *__restrict__ nchunk,
                                                   const uint32_t *__restrict__ cinc, uint64_t nu,
                                                   uint32_t *__restrict__ item_run, uint32_t *__restrict__ item_chunk) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nu) return;
  const uint32_t nc = nchunk[r];
  if (!nc) return;
  const uint32_t o = cinc[r] - nc;
  for (uint32_t c = 0; c < nc; c++) {
    item_run[o + c] = (uint32_t)r;
    item_chunk[o + c] = c;
  }
}

// perm[u] = the sorted run whose first occurrence is the u-th earliest
__global__ __launch_bounds__(256) void k_dup_rank(const uint32_t *__restrict__ perm, uint64_t nu,
                                                  const uint32_t *__restrict__ run_start,
                                                  const uint64_t *__restrict__ ks, uint32_t *__restrict__ rank_of,
                                                  uint64_t *__restrict__ uniq, uint32_t *__restrict__ count) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nu) return;
  const uint32_t r = perm[u];
  rank_of[r] = (uint32_t)u;
  if (uniq) uniq[u] = ks[run_start[r]];
  if (count) count[u] = run_start[r + 1] - run_start[r];
}

__global__ __launch_bounds__(256) void k_dup_inv(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ ps,
                                                 const uint32_t *__restrict__ inc,
                                                 const uint32_t *__restrict__ rank_of, uint64_t n,
                                                 uint32_t *__restrict__ inv) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  inv[ps[j]] = ks[j] == kEmptyKey ? kNoIdx : rank_of[inc[j] - 1];
}

__global__ __launch_bounds__(256) void k_dup_run_keys(const uint64_t *__restrict__ ks,
                                                      const uint32_t *__restrict__ run_start, uint64_t nu,
                                                      uint64_t *__restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < nu) out[r] = ks[run_start[r]];
}

// ---- gather (lookup) ----------------------------------------------------------------------------
template <typename V> __device__ __forceinline__ V zero_of() {
  V z;
  __builtin_memset(&z, 0, sizeof(V));
  return z;
}

// out[i] = the first PV elements of src row row_u[inv[i]] (row_u == nullptr: row inv[i]); a padding
// position or a missing row reads as zero.  WAVE: one wave per position, lanes across the row;
// else one thread per position (narrow rows).  pad_flag: the table's error word, latched with the
// empty-key bit by a padding position (an inserting lookup refuses ~0 as swps_pull does).
template <typename V, bool WAVE>
__global__ __launch_bounds__(256) void k_dup_gather(const uint32_t *__restrict__ inv,
                                                    const uint32_t *__restrict__ row_u, uint64_t n,
                                                    const V *__restrict__ src, uint64_t RV, int PV,
                                                    V *__restrict__ out, uint8_t *__restrict__ found,
                                                    uint32_t *pad_flag) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i = WAVE ? tid >> 6 : tid;
  const int lane = WAVE ? (int)(threadIdx.x & 63) : 0;
  if (i >= n) return;
  const uint32_t u = inv[i];
  uint32_t r = kNoRow;
  if (u != kNoIdx) r = row_u ? row_u[u] : u;
  if (lane == 0) {
    if (u == kNoIdx && pad_flag) atomicOr(pad_flag, 4u);
    if (found) found[i] = r != kNoRow ? 1 : 0;
  }
  const V *row = src + (uint64_t)(r == kNoRow ? 0 : r) * RV;
  for (int e = lane; e < PV; e += WAVE ? 64 : 1) out[i * PV + e] = r == kNoRow ? zero_of<V>() : row[e];
}

// ---- reduce + push --------------------------------------------------------------------------------
// Gradient sources: the fp64 term of position p, elements [c*E, c*E + E) (LR: the one element).
// RowGrads: grads[p], one row per position (swps_push_dup).
template <typename G> struct RowGrads {
  using elem = G;
  const G *__restrict__ g;
  const void *base() const { return g; }
  template <int E> __device__ __forceinline__ void term(uint32_t p, int P, int c, double (&v)[E]) const {
    const Pack<G, E> x = *(const Pack<G, E> *)(g + (uint64_t)p * P + (uint64_t)c * E);
#pragma unroll
    for (int k = 0; k < E; k++) v[k] = (double)x.v[k];
  }
  __device__ __forceinline__ double term1(uint32_t p) const { return (double)g[p]; }
};

// BagGrads: the row of the position's bag, G[bag_of[p]], times w[p] (w != null) or divided by the
// bag's member count (m != null): one IEEE operation per element (swps_push_bag); the [n][P]
// expansion is never materialised
template <typename G> struct BagGrads {
  using elem = G;
  const G *__restrict__ g;
  const uint32_t *__restrict__ bag_of;
  const double *__restrict__ w;
  const uint32_t *__restrict__ m;
  const void *base() const { return g; }
  template <int E> __device__ __forceinline__ void term(uint32_t p, int P, int c, double (&v)[E]) const {
    const uint32_t b = bag_of[p];
    const Pack<G, E> x = *(const Pack<G, E> *)(g + (uint64_t)b * P + (uint64_t)c * E);
#pragma unroll
    for (int k = 0; k < E; k++) v[k] = (double)x.v[k];
    if (w) {
      const double wp = w[p];
#pragma unroll
      for (int k = 0; k < E; k++) v[k] = v[k] * wp;
    } else if (m) {
      const double mb = (double)m[b];
#pragma unroll
      for (int k = 0; k < E; k++) v[k] = v[k] / mb;
    }
  }
  __device__ __forceinline__ double term1(uint32_t p) const {
    const uint32_t b = bag_of[p];
    const double v = (double)g[b];
    return w ? v * w[p] : m ? v / (double)m[b] : v;
  }
};

// The sum of elements [c*E, c*E + E) of the source's terms at sorted entries [a, b): a sequential
// fp64 chain in entry (= position) order that starts from the first entry's value.
template <typename S, int E>
__device__ __forceinline__ void chain_grads(const S &src, const uint32_t *__restrict__ ps, uint64_t a, uint64_t b,
                                            int P, int c, double (&acc)[E]) {
  src.template term<E>(ps[a], P, c, acc);
#pragma unroll 4
  for (uint64_t j = a + 1; j < b; j++) {
    double v[E];
    src.template term<E>(ps[j], P, c, v);
#pragma unroll
    for (int k = 0; k < E; k++) acc[k] = acc[k] + v[k];
  }
}

template <int E> __device__ __forceinline__ void finish_sum(double (&g)[E], uint32_t m, int reduce, double scale) {
#pragma unroll
  for (int k = 0; k < E; k++) {
    if (reduce == SWPS_REDUCE_MEAN) g[k] = g[k] / (double)m;
    g[k] = g[k] * scale;
  }
}

// one step of k_push_w2v on elements [c*E, c*E + E) of [h | v] (x) and [h2 | v2] (x2 = x + P)
template <typename T, int E>
__device__ __forceinline__ void apply_w2v(T *__restrict__ row, int P, int c, const double (&g)[E], double lr,
                                          double fudge, int rule) {
  using PT = Pack<T, E>;
  PT x = ((PT *)row)[c];
  if (rule == SWPS_PUSH_SGD) {
#pragma unroll
    for (int k = 0; k < E; k++) x.v[k] = (T)((double)x.v[k] + g[k] * lr);
    ((PT *)row)[c] = x;
    return;
  }
  PT x2 = ((PT *)(row + P))[c];
#pragma unroll
  for (int k = 0; k < E; k++) {
    const double a = g[k];
    const double x2n = (double)x2.v[k] + a * a;
    x.v[k] = (T)((double)x.v[k] + (a * lr) / sqrt(x2n + fudge));
    x2.v[k] = (T)x2n;
  }
  ((PT *)(row + P))[c] = x2;
  ((PT *)row)[c] = x;
}

template <int E> __device__ __forceinline__ void store_g(double *__restrict__ out, int c, const double (&g)[E]) {
  Pack<double, E> p;
#pragma unroll
  for (int k = 0; k < E; k++) p.v[k] = g[k];
  ((Pack<double, E> *)out)[c] = p;
}

// Runs of at most one chunk: one wave per run, lanes across the element packs; the run is summed
// in registers in position order, then the rule is applied and the row written once (APPLY), or the
// reduced gradient is stored to out[r][P] (the routed form).
template <typename T, typename S, int E, bool APPLY>
__global__ __launch_bounds__(256) void k_dup_short(const uint32_t *__restrict__ run_start, uint64_t nu,
                                                   const uint32_t *__restrict__ ps, const S grads,
                                                   const uint32_t *__restrict__ row_r, T *__restrict__ rows,
                                                   double *__restrict__ out, int P, double lr, double fudge,
                                                   int rule, int reduce, double scale) {
  const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (r >= nu) return;
  const uint32_t a = run_start[r], b = run_start[r + 1];
  if (b - a > kChunk) return;  // the (run, chunk) items take it
  T *row = nullptr;
  if (APPLY) {
    const uint32_t ri = row_r[r];
    if (ri == kNoRow) return;  // the lookup latched the unknown key
    row = rows + (uint64_t)ri * 2 * P;
  }
  for (int c = lane; c < P / E; c += 64) {
    double g[E];
    chain_grads<S, E>(grads, ps, a, b, P, c, g);
    finish_sum<E>(g, b - a, reduce, scale);
    if (APPLY)
      apply_w2v<T, E>(row, P, c, g, lr, fudge, rule);
    else
      store_g<E>(out + r * P, c, g);
  }
}

// Longer runs, pass 1: one wave per (run, chunk) item writes the chunk's fp64 partial sum.
template <typename S, int E>
__global__ __launch_bounds__(256) void k_dup_partial(const uint32_t *__restrict__ item_run,
                                                     const uint32_t *__restrict__ item_chunk, uint64_t nitems,
                                                     const uint32_t *__restrict__ run_start,
                                                     const uint32_t *__restrict__ ps, const S grads,
                                                     double *__restrict__ partial, int P) {
  const uint64_t it = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (it >= nitems) return;
  const uint32_t r = item_run[it];
  const uint64_t a = (uint64_t)run_start[r] + (uint64_t)item_chunk[it] * kChunk;
  const uint64_t e = run_start[r + 1];
  const uint64_t b = a + kChunk < e ? a + kChunk : e;
  for (int c = lane; c < P / E; c += 64) {
    double g[E];
    chain_grads<S, E>(grads, ps, a, b, P, c, g);
    store_g<E>(partial + it * P, c, g);
  }
}

// pass 2 (after pass 1 has completed: a kernel boundary): the wave of a run's first item chains the
// run's partials in chunk order, from the first, and applies the rule / stores the gradient
template <typename T, int E, bool APPLY>
__global__ __launch_bounds__(256) void k_dup_long(const uint32_t *__restrict__ item_run,
                                                  const uint32_t *__restrict__ item_chunk, uint64_t nitems,
                                                  const uint32_t *__restrict__ run_start,
                                                  const double *__restrict__ partial,
                                                  const uint32_t *__restrict__ row_r, T *__restrict__ rows,
                                                  double *__restrict__ out, int P, double lr, double fudge, int rule,
                                                  int reduce, double scale) {
  const uint64_t it = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (it >= nitems || item_chunk[it] != 0) return;
  const uint32_t r = item_run[it];
  const uint32_t m = run_start[r + 1] - run_start[r];
  const uint32_t nc = (m + kChunk - 1) / kChunk;
  T *row = nullptr;
  if (APPLY) {
    const uint32_t ri = row_r[r];
    if (ri == kNoRow) return;
    row = rows + (uint64_t)ri * 2 * P;
  }
  using PD = Pack<double, E>;
  for (int c = lane; c < P / E; c += 64) {
    double g[E];
    PD p = ((const PD *)(partial + it * P))[c];
#pragma unroll
    for (int k = 0; k < E; k++) g[k] = p.v[k];
#pragma unroll 4
    for (uint32_t q = 1; q < nc; q++) {
      p = ((const PD *)(partial + (it + q) * P))[c];
#pragma unroll
      for (int k = 0; k < E; k++) g[k] = g[k] + p.v[k];
    }
    finish_sum<E>(g, m, reduce, scale);
    if (APPLY)
      apply_w2v<T, E>(row, P, c, g, lr, fudge, rule);
    else
      store_g<E>(out + (uint64_t)r * P, c, g);
  }
}

// ---- LR rows (one fp32 gradient per occurrence): threads instead of waves, the same chunk rule ----
template <typename S>
__device__ __forceinline__ double chain_lr(const S &grads, const uint32_t *__restrict__ ps, uint64_t a, uint64_t b) {
  double acc = grads.term1(ps[a]);
#pragma unroll 4
  for (uint64_t j = a + 1; j < b; j++) acc = acc + grads.term1(ps[j]);
  return acc;
}

// one step of k_push_lr with the gradient (float)g, or the gradient stored for the routed push
template <typename T, bool APPLY>
__device__ __forceinline__ void finish_lr(double g, uint32_t m, int reduce, double scale, uint32_t r,
                                          const uint32_t *__restrict__ row_r, T *__restrict__ rows,
                                          float *__restrict__ out, T lr, T fudge, int rule) {
  if (reduce == SWPS_REDUCE_MEAN) g = g / (double)m;
  g = g * scale;
  const float gf = (float)g;
  if (!APPLY) {
    out[r] = gf;
    return;
  }
  const uint32_t ri = row_r[r];
  if (ri == kNoRow) return;
  const T mg = (T)gf;
  T *row = rows + (uint64_t)ri * 2;
  if (rule == SWPS_PUSH_SGD) {
    row[0] = row[0] + lr * mg;
    return;
  }
  T g2 = row[1] + mg * mg;
  row[1] = g2;
  T step = lr * mg;
  row[0] = row[0] + step / (T)sqrt(g2 + fudge);
}

template <typename T, typename S, bool APPLY>
__global__ __launch_bounds__(256) void k_dup_lr_short(const uint32_t *__restrict__ run_start, uint64_t nu,
                                                      const uint32_t *__restrict__ ps, const S grads,
                                                      const uint32_t *__restrict__ row_r, T *__restrict__ rows,
                                                      float *__restrict__ out, T lr, T fudge, int rule, int reduce,
                                                      double scale) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nu) return;
  const uint32_t a = run_start[r], b = run_start[r + 1];
  if (b - a > kChunk) return;
  finish_lr<T, APPLY>(chain_lr(grads, ps, a, b), b - a, reduce, scale, (uint32_t)r, row_r, rows, out, lr, fudge,
                      rule);
}

template <typename S>
__global__ __launch_bounds__(256) void k_dup_lr_partial(const uint32_t *__restrict__ item_run,
                                                        const uint32_t *__restrict__ item_chunk, uint64_t nitems,
                                                        const uint32_t *__restrict__ run_start,
                                                        const uint32_t *__restrict__ ps, const S grads,
                                                        double *__restrict__ partial) {
  const uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems) return;
  const uint32_t r = item_run[it];
  const uint64_t a = (uint64_t)run_start[r] + (uint64_t)item_chunk[it] * kChunk;
  const uint64_t e = run_start[r + 1];
  partial[it] = chain_lr(grads, ps, a, a + kChunk < e ? a + kChunk : e);
}

template <typename T, bool APPLY>
__global__ __launch_bounds__(256) void k_dup_lr_long(const uint32_t *__restrict__ item_run,
                                                     const uint32_t *__restrict__ item_chunk, uint64_t nitems,
                                                     const uint32_t *__restrict__ run_start,
                                                     const double *__restrict__ partial,
                                                     const uint32_t *__restrict__ row_r, T *__restrict__ rows,
                                                     float *__restrict__ out, T lr, T fudge, int rule, int reduce,
                                                     double scale) {
  const uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nitems || item_chunk[it] != 0) return;
  const uint32_t r = item_run[it];
  const uint32_t m = run_start[r + 1] - run_start[r];
  const uint32_t nc = (m + kChunk - 1) / kChunk;
  double g = partial[it];
  for (uint32_t q = 1; q < nc; q++) g = g + partial[it + q];
  finish_lr<T, APPLY>(g, m, reduce, scale, r, row_r, rows, out, lr, fudge, rule);
}

// ---- host side ------------------------------------------------------------------------------------
// buffers of swps_table::dup
enum {
  B_KS = 0, B_U32, B_SORT, B_SCAN, B_RANK, B_UNIQ, B_INV, B_ROWS, B_ITEMS, B_PART, B_VALS,
  // the pooled calls (swps_bag.hip): per-bag / per-position words, the (bag, chunk) items, their partials
  B_BAG, B_BAG_ITEMS, B_BAG_PART
};
static_assert(B_BAG_PART < kDupBufs, "swps_table::dup is too small");

struct Runs {
  uint64_t n = 0, nu = 0, nitems = 0;
  uint64_t *ks = nullptr;  // [n] sorted keys
  uint32_t *ps = nullptr, *flags = nullptr, *inc = nullptr, *run_start = nullptr, *head_pos = nullptr,
           *nchunk = nullptr, *cinc = nullptr;
};

int scan_u32(swps_table *t, const uint32_t *in, uint32_t *out, uint64_t n, hipStream_t s) {
  size_t b = 0;
  SWPS_HIP(rocprim::inclusive_scan(nullptr, b, in, out, (size_t)n, rocprim::plus<uint32_t>(), s));
  SWPS_TRY(t->dup[B_SCAN].ensure(b));
  b = t->dup[B_SCAN].bytes;
  SWPS_HIP(rocprim::inclusive_scan(t->dup[B_SCAN].p, b, in, out, (size_t)n, rocprim::plus<uint32_t>(), s));
  return SWPS_OK;
}

// The runs of d_keys[n] (n > 0) in key order and, with `items`, the chunk counts of the long runs;
// reads the distinct count (and the item count) on the host: one stream synchronisation, which
// also brings `extra` (device words the caller queued on s before this call) to the host.
struct HostRead {
  const uint32_t *d = nullptr;
  uint32_t *h = nullptr;
  int words = 0;
};

int sorted_runs(swps_table *t, const uint64_t *d_keys, uint64_t n, hipStream_t s, bool items, Runs &R,
                const HostRead *extra = nullptr) {
  R.n = n;
  SWPS_TRY(t->dup[B_KS].ensure(n * 8));
  SWPS_TRY(t->dup[B_U32].ensure((7 * n + 8) * 4));
  R.ks = t->dup[B_KS].as<uint64_t>();
  uint32_t *u = t->dup[B_U32].as<uint32_t>();
  R.ps = u;
  R.flags = u + n;
  R.inc = u + 2 * n;
  R.head_pos = u + 3 * n;
  R.nchunk = u + 4 * n;
  R.cinc = u + 5 * n;
  R.run_start = u + 6 * n;  // [n + 1]
  SWPS_TRY(sort_pairs_iota(t->dup[B_SORT], d_keys, R.ks, R.ps, n, 64, s));
  k_dup_flags<<<nblk(n), 256, 0, s>>>(R.ks, n, R.flags);
  SWPS_HIP(hipGetLastError());
  SWPS_TRY(scan_u32(t, R.flags, R.inc, n, s));
  k_dup_heads<<<nblk(n), 256, 0, s>>>(R.ks, R.ps, R.flags, R.inc, n, R.run_start, R.head_pos);
  SWPS_HIP(hipGetLastError());
  uint32_t h[2] = {0, 0};
  if (items) {
    k_dup_nchunk<<<nblk(n), 256, 0, s>>>(R.run_start, R.inc, n, R.nchunk);
    SWPS_HIP(hipGetLastError());
    SWPS_TRY(scan_u32(t, R.nchunk, R.cinc, n, s));
    SWPS_HIP(hipMemcpyAsync(&h[1], R.cinc + (n - 1), 4, hipMemcpyDeviceToHost, s));
  }
  SWPS_HIP(hipMemcpyAsync(&h[0], R.inc + (n - 1), 4, hipMemcpyDeviceToHost, s));
  if (extra) SWPS_HIP(hipMemcpyAsync(extra->h, extra->d, (size_t)extra->words * 4, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  R.nu = h[0];
  R.nitems = h[1];
  return SWPS_OK;
}

// first-occurrence order: uniq / inv / count (any may be null) from the runs
int rank_runs(swps_table *t, const Runs &R, uint64_t *uniq, uint32_t *inv, uint32_t *count, hipStream_t s) {
  const uint64_t n = R.n, nu = R.nu;
  SWPS_TRY(t->dup[B_RANK].ensure((3 * nu + 4) * 4));
  uint32_t *head_s = t->dup[B_RANK].as<uint32_t>(), *perm = head_s + nu, *rank_of = perm + nu;
  if (nu) {
    int bits = 1;
    while (bits < 32 && (1ULL << bits) < n) bits++;
    SWPS_TRY(sort_pairs_iota(t->dup[B_SORT], R.head_pos, head_s, perm, nu, bits, s));
    k_dup_rank<<<nblk(nu), 256, 0, s>>>(perm, nu, R.run_start, R.ks, rank_of, uniq, count);
    SWPS_HIP(hipGetLastError());
  }
  if (inv) {
    k_dup_inv<<<nblk(n), 256, 0, s>>>(R.ks, R.ps, R.inc, rank_of, n, inv);
    SWPS_HIP(hipGetLastError());
  }
  return SWPS_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// out[i] = src row (row_u ? row_u[inv[i]] : inv[i]), the first pull_elems elements of rows of
// row_bytes; 16-B lanes when strides, width and both bases allow, else scalar lanes; narrow rows
// (LR) one thread per position
int gather(swps_table *t, const uint32_t *inv, const uint32_t *row_u, uint64_t n, const void *src, size_t row_bytes,
           void *out, uint8_t *found, uint32_t *pad_flag, hipStream_t s) {
  const size_t cb = (size_t)t->pull_elems * t->esize;
  const bool f64 = t->cfg.dtype == SWPS_F64;
  if (t->pull_elems <= 4 && cb < 16) {
    if (f64)
      k_dup_gather<double, false><<<nblk(n), 256, 0, s>>>(inv, row_u, n, (const double *)src, row_bytes / 8,
                                                          t->pull_elems, (double *)out, found, pad_flag);
    else
      k_dup_gather<float, false><<<nblk(n), 256, 0, s>>>(inv, row_u, n, (const float *)src, row_bytes / 4,
                                                         t->pull_elems, (float *)out, found, pad_flag);
  } else if (row_bytes % 16 == 0 && cb % 16 == 0 && aligned16(src) && aligned16(out)) {
    k_dup_gather<uint4, true><<<nblk(n * 64), 256, 0, s>>>(inv, row_u, n, (const uint4 *)src, row_bytes / 16,
                                                           (int)(cb / 16), (uint4 *)out, found, pad_flag);
  } else if (f64) {
    k_dup_gather<double, true><<<nblk(n * 64), 256, 0, s>>>(inv, row_u, n, (const double *)src, row_bytes / 8,
                                                            t->pull_elems, (double *)out, found, pad_flag);
  } else {
    k_dup_gather<float, true><<<nblk(n * 64), 256, 0, s>>>(inv, row_u, n, (const float *)src, row_bytes / 4,
                                                           t->pull_elems, (float *)out, found, pad_flag);
  }
  SWPS_HIP(hipGetLastError());
  return SWPS_OK;
}

template <typename T, typename S, int E, bool APPLY>
int launch_w2v(swps_table *t, const Runs &R, const S &grads, const uint32_t *row_r, double *out,
               const uint32_t *item_run, const uint32_t *item_chunk, double *partial, int reduce, double scale,
               hipStream_t s) {
  const int P = t->push_elems, rule = t->cfg.push_rule;
  const double lr = (double)t->cfg.learning_rate, fudge = (double)t->cfg.fudge;
  T *rows = APPLY ? t->rows.as<T>() : nullptr;
  k_dup_short<T, S, E, APPLY><<<nblk(R.nu * 64), 256, 0, s>>>(R.run_start, R.nu, R.ps, grads, row_r, rows, out, P, lr,
                                                              fudge, rule, reduce, scale);
  SWPS_HIP(hipGetLastError());
  if (R.nitems) {
    k_dup_partial<S, E><<<nblk(R.nitems * 64), 256, 0, s>>>(item_run, item_chunk, R.nitems, R.run_start, R.ps, grads,
                                                            partial, P);
    SWPS_HIP(hipGetLastError());
    k_dup_long<T, E, APPLY><<<nblk(R.nitems * 64), 256, 0, s>>>(item_run, item_chunk, R.nitems, R.run_start, partial,
                                                                row_r, rows, out, P, lr, fudge, rule, reduce, scale);
    SWPS_HIP(hipGetLastError());
  }
  return SWPS_OK;
}

template <typename T, typename S, bool APPLY>
int launch_w2v_e(swps_table *t, const Runs &R, const S &grads, const uint32_t *row_r, double *out,
                 const uint32_t *item_run, const uint32_t *item_chunk, double *partial, int reduce, double scale,
                 hipStream_t s) {
  constexpr int E = 16 / sizeof(typename S::elem);  // 16-B lanes on the gradients, the widest stream
  if (t->push_elems % E == 0 && aligned16(grads.base()))
    return launch_w2v<T, S, E, APPLY>(t, R, grads, row_r, out, item_run, item_chunk, partial, reduce, scale, s);
  return launch_w2v<T, S, 1, APPLY>(t, R, grads, row_r, out, item_run, item_chunk, partial, reduce, scale, s);
}

template <typename T, typename S, bool APPLY>
int launch_lr(swps_table *t, const Runs &R, const S &grads, const uint32_t *row_r, float *out,
              const uint32_t *item_run, const uint32_t *item_chunk, double *partial, int reduce, double scale,
              hipStream_t s) {
  const T lr = (T)t->cfg.learning_rate, fudge = (T)t->cfg.fudge;
  const int rule = t->cfg.push_rule;
  T *rows = APPLY ? t->rows.as<T>() : nullptr;
  k_dup_lr_short<T, S, APPLY><<<nblk(R.nu), 256, 0, s>>>(R.run_start, R.nu, R.ps, grads, row_r, rows, out, lr, fudge,
                                                         rule, reduce, scale);
  SWPS_HIP(hipGetLastError());
  if (R.nitems) {
    k_dup_lr_partial<S><<<nblk(R.nitems), 256, 0, s>>>(item_run, item_chunk, R.nitems, R.run_start, R.ps, grads,
                                                       partial);
    SWPS_HIP(hipGetLastError());
    k_dup_lr_long<T, APPLY><<<nblk(R.nitems), 256, 0, s>>>(item_run, item_chunk, R.nitems, R.run_start, partial, row_r,
                                                           rows, out, lr, fudge, rule, reduce, scale);
    SWPS_HIP(hipGetLastError());
  }
  return SWPS_OK;
}

// what BagGrads needs beside the [nbags][push elems] gradient (swps_push_bag)
struct BagArgs {
  const uint32_t *bag_of = nullptr;
  const double *w = nullptr;
  const uint32_t *m = nullptr;
};

template <typename G, bool BAG> auto grad_source(const void *grads, const BagArgs *bag) {
  if constexpr (BAG)
    return BagGrads<G>{(const G *)grads, bag->bag_of, bag->w, bag->m};
  else
    return RowGrads<G>{(const G *)grads};
}

// The runs' reduced gradients applied to rows row_r (APPLY) or stored to `out` ([nu][push elems],
// fp64 for W2V, fp32 for LR: the wire types of the routed push).  BAG: grads is [nbags][push
// elems] and a position's term is derived from its bag's row (BagGrads), else [n][push elems]
template <bool APPLY, bool BAG = false>
int reduce_runs(swps_table *t, const Runs &R, const void *grads, int gdtype, const uint32_t *row_r, void *out,
                int reduce, double scale, hipStream_t s, const BagArgs *bag = nullptr) {
  uint32_t *item_run = nullptr, *item_chunk = nullptr;
  double *partial = nullptr;
  if (R.nitems) {
    SWPS_TRY(t->dup[B_ITEMS].ensure(R.nitems * 8));
    SWPS_TRY(t->dup[B_PART].ensure(R.nitems * (uint64_t)t->push_elems * 8));
    item_run = t->dup[B_ITEMS].as<uint32_t>();
    item_chunk = item_run + R.nitems;
    partial = t->dup[B_PART].as<double>();
    k_dup_items<<<nblk(R.nu), 256, 0, s>>>(R.nchunk, R.cinc, R.nu, item_run, item_chunk);
    SWPS_HIP(hipGetLastError());
  }
  const bool f64 = t->cfg.dtype == SWPS_F64;
  if (t->cfg.layout == SWPS_LAYOUT_LR) {
    auto src = grad_source<float, BAG>(grads, bag);
    using S = decltype(src);
    if (f64)
      return launch_lr<double, S, APPLY>(t, R, src, row_r, (float *)out, item_run, item_chunk, partial, reduce, scale,
                                         s);
    return launch_lr<float, S, APPLY>(t, R, src, row_r, (float *)out, item_run, item_chunk, partial, reduce, scale, s);
  }
  if (gdtype == SWPS_F64) {
    auto src = grad_source<double, BAG>(grads, bag);
    using S = decltype(src);
    if (f64)
      return launch_w2v_e<double, S, APPLY>(t, R, src, row_r, (double *)out, item_run, item_chunk, partial, reduce,
                                            scale, s);
    return launch_w2v_e<float, S, APPLY>(t, R, src, row_r, (double *)out, item_run, item_chunk, partial, reduce, scale,
                                         s);
  }
  auto src = grad_source<float, BAG>(grads, bag);
  using S = decltype(src);
  if (f64)
    return launch_w2v_e<double, S, APPLY>(t, R, src, row_r, (double *)out, item_run, item_chunk, partial, reduce,
                                          scale, s);
  return launch_w2v_e<float, S, APPLY>(t, R, src, row_r, (double *)out, item_run, item_chunk, partial, reduce, scale,
                                       s);
}

int check_n(uint64_t n) {
  if (n >= (1ULL << 32)) return fail(SWPS_E_UNSUPPORTED, "2^32 or more keys in one call (positions are 32-bit)");
  return SWPS_OK;
}

}  // namespace

#pragma clang diagnostic pop
