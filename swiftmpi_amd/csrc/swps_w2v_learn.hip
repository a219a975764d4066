// word2vec minibatch learn (swps_w2v_ctx.h): everything that reads or writes
// parameters — the pull (or the install of the owners' values), the forward
// (learn_instance's position body), the chunked segmented gradient sums and
// the push (mean + AdaGrad, or the sharded learner's mean gradients) — in the
// four precisions (fp64, fp32 rows with fp64 intermediates, fast fp32, and
// the BFP rows of swps_w2v_bfp.h), then the step dispatch (learn_batch: one
// function per stage), the overlapped single-GPU driver and the whole-vocab
// initialisers.
#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>

#include "swps_rand.h"
#include "swps_w2v_ctx.h"
#include "swps_wave.h"

using namespace swps;

namespace {

template <typename T> struct V16;
template <> struct V16<float> {
  using V = float4;
  static constexpr int E = 4;
};
template <> struct V16<double> {
  using V = double2;
  static constexpr int E = 2;
};


// cache <- table rows (h, v) for the listed vids; local[vid] = u when set_local
template <typename T>
__global__ __launch_bounds__(256) void k_pull(const int32_t *__restrict__ K, uint32_t U,
                                              const uint32_t *__restrict__ vid_row, const T *__restrict__ rows,
                                              int D, T *__restrict__ cache_h, T *__restrict__ cache_v,
                                              int32_t *__restrict__ local, int set_local, int cs) {
  using V = typename V16<T>::V;
  constexpr int E = V16<T>::E;
  const int lane = threadIdx.x & 63;
  const int NC = D / E;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < U; u += (uint64_t)gridDim.x * 4) {
    const int32_t vid = K ? K[u] : (int32_t)u;
    const V *src = (const V *)(rows + (uint64_t)vid_row[vid] * 4 * D);
    V *dh = (V *)(cache_h + (uint64_t)vid * cs);  // cs: the cache row stride (swps_w2v::cs)
    V *dv = (V *)(cache_v + (uint64_t)vid * cs);
    for (int c = lane; c < cs / E; c += 64) {  // the pad too (zeros): whole-line stores
      const bool in = c < NC;
      dh[c] = in ? src[c] : V{};
      dv[c] = in ? src[NC + c] : V{};
    }
    if (set_local && lane == 0) local[vid] = (int32_t)u;
  }
}

// Chunk ci = elements [E*ci, E*ci+E) of a D-element row, held by one lane as
// one register chunk and converted to / from fp64.  16 B of the table type per
// lane; when fp32 rows carry fp64 intermediates (E = 4 doubles) the row is
// stored as two planes [D/2 | D/2] of double2 so every load/store instruction
// of a wave is contiguous.
template <typename X, int E> struct Chk;
template <> struct Chk<float, 4> {
  using R = float4;
  static __device__ __forceinline__ R ld(const float *row, int ci, int) { return ((const float4 *)row)[ci]; }
  static __device__ __forceinline__ double at(const R &r, int k) { return (double)((const float *)&r)[k]; }
  static __device__ __forceinline__ void st(float *row, int ci, int, const double (&v)[4]) {
    ((float4 *)row)[ci] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  }
};
template <> struct Chk<double, 4> {
  struct R {
    double2 a, b;
  };
  static __device__ __forceinline__ R ld(const double *row, int ci, int D) {
    R r;
    r.a = ((const double2 *)row)[ci];
    r.b = ((const double2 *)(row + D / 2))[ci];
    return r;
  }
  static __device__ __forceinline__ double at(const R &r, int k) { return ((const double *)&r)[k]; }
  static __device__ __forceinline__ void st(double *row, int ci, int D, const double (&v)[4]) {
    ((double2 *)row)[ci] = make_double2(v[0], v[1]);
    ((double2 *)(row + D / 2))[ci] = make_double2(v[2], v[3]);
  }
};
template <> struct Chk<double, 2> {
  using R = double2;
  static __device__ __forceinline__ R ld(const double *row, int ci, int) { return ((const double2 *)row)[ci]; }
  static __device__ __forceinline__ double at(const R &r, int k) { return ((const double *)&r)[k]; }
  static __device__ __forceinline__ void st(double *row, int ci, int, const double (&v)[2]) {
    ((double2 *)row)[ci] = make_double2(v[0], v[1]);
  }
};

template <typename T, typename A> struct FwdArgs {
  const int32_t *rec;
  int P;
  const T *cache_h, *cache_v;
  const T *tab;  // the table's rows [cap][4D]: source of rows tagged kTabRow (single-GPU direct reads)
  const float *exptab;
  int D, W, N;
  float alpha;
  A *neu1, *neu1e;
  float *pg;
  int xcd;  // 1: XCD-contiguous block order (xcd_block)
  int ld;   // neu1/neu1e row stride in elements (D rounded up to 128 B: whole cache lines per row)
  int cs;   // worker-cache row stride in elements (the same rounding)
  int full;  // k_forward_t: neu1/neu1e stores cover the row pad (zeros): whole lines (SWPS_FULL_LINES)
  int rowg;  // k_forward_b: N + 1 = g goes into the neu1 row's pad and pg is not written; 0 = pg (bfp_row_g)
};

// Source row of a forward slot: a record entry tagged kTabRow is a row index
// into the table (the batch's pulled keys: the table row IS the value the
// pull would have copied — the push of this batch has not run yet); any other
// entry >= 0 is a vid into the worker cache (stale rows of keys outside the
// batch key set, global_pull_access.h:88-97).
template <typename T, typename A>
__device__ __forceinline__ const T *slot_row(const FwdArgs<T, A> &a, int32_t e, bool ctx) {
  if (e & kTabRow) return a.tab + (uint64_t)(e & ~kTabRow) * 4 * a.D + (ctx ? a.D : 0);
  return (ctx ? a.cache_v : a.cache_h) + (uint64_t)e * a.cs;
}

// Blocks are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md
// §Workgroup dispatch: b and b+8 share one).  Renumber so each XCD walks one
// contiguous range of positions: neighbouring kept positions share most of
// their context rows (the window slides by one token), so those rows are
// re-read from the XCD's own L2 instead of crossing to HBM/MALL.  A bijection
// on [0, G) for any G; speed only, never correctness.
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t G) {
  const uint32_t q = G >> 3, r = G & 7, x = b & 7, i = b >> 3;
  return x * q + min(x, r) + i;
}

// One wave per kept position (the body of learn_instance's position loop,
// word2vec_global.h:663-718).  Context v rows are loaded in groups of G slots
// whose loads are issued together and summed into neu1 in slot order; then
// the targets, up to 8 at a time: their h rows, the 8 per-lane partial dots
// with neu1 (fp64) reduced together (wave_sum8), g from the exp table, and
// neu1e += g*h.  Writes neu1, neu1e (gradient sources) and g.
template <typename T, typename A, int NCH, int G>
__global__ __launch_bounds__(256) void k_forward_b8(FwdArgs<T, A> a) {
  constexpr int E = V16<T>::E;
  using CT = Chk<T, E>;
  using CA = Chk<A, E>;
  const int lane = threadIdx.x & 63;
  const uint32_t blk = a.xcd ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x;
  const int p = __builtin_amdgcn_readfirstlane((int)(blk * 4 + (threadIdx.x >> 6)));
  if (p >= a.P) return;
  const int D = a.D, W = a.W, N = a.N, NC = D / E;
  const int S = 2 * W + N + 1;  // slots: contexts then targets
  const int32_t *r = a.rec + (uint64_t)p * (S + 1);
  double acc[NCH][E], ne[NCH][E];
#pragma unroll
  for (int c = 0; c < NCH; c++)
#pragma unroll
    for (int k = 0; k < E; k++) {
      acc[c][k] = 0.0;
      ne[c][k] = 0.0;
    }
  // Slots in groups of G whose row loads are issued together: context slots
  // (v rows) add into neu1 in slot order; target slots (h rows) of the group
  // then get their per-lane partial dots with the finished neu1, reduced
  // together (wave_sum8), g from the exp table, and neu1e += g*h.
  static_assert(G == 8, "wave_sum8 reduces eight targets");
  for (int s0 = 0; s0 < S; s0 += G) {
    typename CT::R rows[G][NCH];
    int32_t vid[G];
#pragma unroll
    for (int q = 0; q < G; q++) {
      const int slot = s0 + q;
      vid[q] = slot < S ? r[1 + slot] : -1;
      if (vid[q] >= 0) {
        const T *src = slot_row(a, vid[q], slot < 2 * W);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
          const int ci = lane + c * 64;
          if (ci < NC) rows[q][c] = CT::ld(src, ci, D);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < G; q++) {
      if (s0 + q >= 2 * W || vid[q] < 0) continue;
#pragma unroll
      for (int c = 0; c < NCH; c++)
        if (lane + c * 64 < NC)
#pragma unroll
          for (int k = 0; k < E; k++) acc[c][k] += CT::at(rows[q][c], k);
    }
    if (s0 + G <= 2 * W) continue;  // no target in this group
    double part[G];
    uint32_t tmask = 0;  // wave-uniform: target slots of this group that are present
#pragma unroll
    for (int q = 0; q < G; q++) {
      double pq = 0.0;
      if (s0 + q >= 2 * W && vid[q] >= 0) {
        tmask |= 1u << q;
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (lane + c * 64 < NC)
#pragma unroll
            for (int k = 0; k < E; k++) {
              const double prod = acc[c][k] * CT::at(rows[q][c], k);
              pq += prod;
            }
      }
      part[q] = pq;
    }
    const double tot = wave_sum8(part, lane);
    // lanes 8q..8q+7 hold slot s0+q's dot: g per learn_instance (word2vec_global.h:693-701)
    const int d = s0 + (lane >> 3) - 2 * W;
    float f = 0;
    f += tot;
    const int label = d == 0 ? 1 : 0;
    float g;
    if (f > 6)
      g = (label - 1) * a.alpha;
    else if (f < -6)
      g = (label - 0) * a.alpha;
    else
      g = (label - a.exptab[(int)((f + 6) * (1000 / 6 / 2))]) * a.alpha;
#pragma unroll
    for (int q = 0; q < G; q++) {
      if (!((tmask >> q) & 1)) continue;
      const float gq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g), 8 * q));
#pragma unroll
      for (int c = 0; c < NCH; c++)
        if (lane + c * 64 < NC)
#pragma unroll
          for (int k = 0; k < E; k++) {
            const double prod = (double)gq * CT::at(rows[q][c], k);
            ne[c][k] += prod;
          }
    }
    if ((lane & 7) == 0 && d >= 0 && d <= N) a.pg[(uint64_t)p * (N + 1) + d] = (tmask >> (lane >> 3)) & 1 ? g : 0.f;
  }
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    const int ci = lane + c * 64;
    if (ci < NC) {
      CA::st(a.neu1 + (uint64_t)p * a.ld, ci, D, acc[c]);
      CA::st(a.neu1e + (uint64_t)p * a.ld, ci, D, ne[c]);
    }
  }
}

// The form with one wave reduction per target: faster than k_forward_b8 with
// fp32 intermediates (4.3 vs 6.4 ms per 5M-token batch, same box), slower with
// fp64 ones — launch_forward picks per mode.
template <typename T, typename A, int NCH, int G>
__global__ __launch_bounds__(256) void k_forward(FwdArgs<T, A> a) {
  constexpr int E = V16<T>::E;
  using CT = Chk<T, E>;
  using CA = Chk<A, E>;
  const int lane = threadIdx.x & 63;
  const uint32_t blk = a.xcd ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x;
  const int p = __builtin_amdgcn_readfirstlane((int)(blk * 4 + (threadIdx.x >> 6)));
  if (p >= a.P) return;
  const int D = a.D, W = a.W, N = a.N, NC = D / E;
  const int S = 2 * W + N + 1;  // slots: contexts then targets
  const int32_t *r = a.rec + (uint64_t)p * (S + 1);
  double acc[NCH][E], ne[NCH][E];
#pragma unroll
  for (int c = 0; c < NCH; c++)
#pragma unroll
    for (int k = 0; k < E; k++) {
      acc[c][k] = 0.0;
      ne[c][k] = 0.0;
    }
  float gk = 0.f;
  for (int s0 = 0; s0 < S; s0 += G) {
    typename CT::R rows[G][NCH];
    int32_t vid[G];
#pragma unroll
    for (int q = 0; q < G; q++) {
      const int slot = s0 + q;
      vid[q] = slot < S ? r[1 + slot] : -1;
      if (vid[q] >= 0) {
        const T *src = slot_row(a, vid[q], slot < 2 * W);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
          const int ci = lane + c * 64;
          if (ci < NC) rows[q][c] = CT::ld(src, ci, D);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < G; q++) {
      const int slot = s0 + q;
      if (vid[q] < 0) continue;
      if (slot < 2 * W) {
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (lane + c * 64 < NC)
#pragma unroll
            for (int k = 0; k < E; k++) acc[c][k] += CT::at(rows[q][c], k);
      } else {
        const int d = slot - 2 * W;
        double part = 0.0;
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (lane + c * 64 < NC)
#pragma unroll
            for (int k = 0; k < E; k++) {
              const double prod = acc[c][k] * CT::at(rows[q][c], k);
              part += prod;
            }
        part = wave_sum_pl(part);
        float f = 0;
        f += part;
        const int label = d == 0 ? 1 : 0;
        float g;
        if (f > 6)
          g = (label - 1) * a.alpha;
        else if (f < -6)
          g = (label - 0) * a.alpha;
        else
          g = (label - a.exptab[(int)((f + 6) * (1000 / 6 / 2))]) * a.alpha;
#pragma unroll
        for (int c = 0; c < NCH; c++)
          if (lane + c * 64 < NC)
#pragma unroll
            for (int k = 0; k < E; k++) {
              const double prod = (double)g * CT::at(rows[q][c], k);
              ne[c][k] += prod;
            }
        if (lane == d) gk = g;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    const int ci = lane + c * 64;
    if (ci < NC) {
      CA::st(a.neu1 + (uint64_t)p * a.ld, ci, D, acc[c]);
      CA::st(a.neu1e + (uint64_t)p * a.ld, ci, D, ne[c]);
    }
  }
  if (lane <= N) a.pg[(uint64_t)p * (N + 1) + lane] = gk;
}

// Fast mode (fp32 rows, fp32 intermediates) when D = 256*NCH + tail with
// 0 < tail <= 64 (D = 300: one float4 chunk + a 44-lane float tail): a lane's
// slice of a row is NCH float4 + one float, 5 registers per row at D = 300
// instead of the 8 two whole float4 chunks take, so more rows are in flight
// per CU.  Same memory layout (natural element order) as the chunked form.
template <int NCH> struct FSlice {
  float4 v[NCH];
  float t;
  __device__ __forceinline__ void ld(const float *row, int lane, bool tl) {
#pragma unroll
    for (int c = 0; c < NCH; c++) v[c] = ((const float4 *)row)[lane + c * 64];
    t = row[256 * NCH + (tl ? lane : 0)];  // lanes past the tail load a valid duplicate: no branch
  }
  __device__ __forceinline__ void st(float *row, int lane, bool tl) const {
#pragma unroll
    for (int c = 0; c < NCH; c++) ((float4 *)row)[lane + c * 64] = v[c];
    if (tl) row[256 * NCH + lane] = t;
  }
  // the same into a row of ld >= D elements whose pad (elements D..ld) is written as zeros:
  // whole-line stores (a partial last line is a masked write that HBM completes as a
  // read-modify-write of its ECC word; measured on the cache rows: pull 0.19 -> 0.16 ms)
  __device__ __forceinline__ void st_full(float *row, int lane, bool tl, int ld) const {
#pragma unroll
    for (int c = 0; c < NCH; c++) ((float4 *)row)[lane + c * 64] = v[c];
    if (256 * NCH + lane < ld) row[256 * NCH + lane] = tl ? t : 0.f;
  }
};
template <int NCH> struct FAcc {
  double v[NCH][4];
  double t;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
      for (int k = 0; k < 4; k++) v[c][k] = 0.0;
    t = 0.0;
  }
  __device__ __forceinline__ void add(const FSlice<NCH> &r, bool tl) {
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      v[c][0] += (double)r.v[c].x;
      v[c][1] += (double)r.v[c].y;
      v[c][2] += (double)r.v[c].z;
      v[c][3] += (double)r.v[c].w;
    }
    t += (double)r.t;  // garbage past the tail is never stored nor dotted
  }
  __device__ __forceinline__ void axpy(double g, const FSlice<NCH> &r, bool tl) {
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const double p0 = g * (double)r.v[c].x, p1 = g * (double)r.v[c].y, p2 = g * (double)r.v[c].z,
                   p3 = g * (double)r.v[c].w;
      v[c][0] += p0;
      v[c][1] += p1;
      v[c][2] += p2;
      v[c][3] += p3;
    }
    const double p = g * (double)r.t;
    t += p;
  }
  __device__ __forceinline__ double dot(const FSlice<NCH> &r, bool tl) const {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const double p0 = v[c][0] * (double)r.v[c].x, p1 = v[c][1] * (double)r.v[c].y,
                   p2 = v[c][2] * (double)r.v[c].z, p3 = v[c][3] * (double)r.v[c].w;
      s += p0;
      s += p1;
      s += p2;
      s += p3;
    }
    const double p = t * (double)r.t;
    s += tl ? p : 0.0;
    return s;
  }
  __device__ __forceinline__ void st(float *row, int lane, bool tl) const {
#pragma unroll
    for (int c = 0; c < NCH; c++)
      ((float4 *)row)[lane + c * 64] = make_float4((float)v[c][0], (float)v[c][1], (float)v[c][2], (float)v[c][3]);
    if (tl) row[256 * NCH + lane] = (float)t;
  }
  __device__ __forceinline__ void st_full(float *row, int lane, bool tl, int ld) const {  // FSlice::st_full
#pragma unroll
    for (int c = 0; c < NCH; c++)
      ((float4 *)row)[lane + c * 64] = make_float4((float)v[c][0], (float)v[c][1], (float)v[c][2], (float)v[c][3]);
    if (256 * NCH + lane < ld) row[256 * NCH + lane] = tl ? (float)t : 0.f;
  }
};

// k_forward (fast mode) on FSlice rows.
template <int NCH, int G, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void k_forward_t(FwdArgs<float, float> a) {
  const int lane = threadIdx.x & 63;
  const uint32_t blk = a.xcd ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x;
  const int p = __builtin_amdgcn_readfirstlane((int)(blk * 4 + (threadIdx.x >> 6)));
  if (p >= a.P) return;
  const int D = a.D, W = a.W, N = a.N;
  const bool tl = 256 * NCH + lane < D;
  const int S = 2 * W + N + 1;  // slots: contexts then targets
  const int32_t *r = a.rec + (uint64_t)p * (S + 1);
  FAcc<NCH> acc, ne;
  acc.zero();
  ne.zero();
  float gk = 0.f;
  for (int s0 = 0; s0 < S; s0 += G) {
    FSlice<NCH> rows[G];
    int32_t vid[G];
#pragma unroll
    for (int q = 0; q < G; q++) {
      const int slot = s0 + q;
      vid[q] = __builtin_amdgcn_readfirstlane(slot < S ? r[1 + slot] : -1);
      if (vid[q] >= 0) rows[q].ld(slot_row(a, vid[q], slot < 2 * W), lane, tl);
    }
#pragma unroll
    for (int q = 0; q < G; q++) {
      const int slot = s0 + q;
      if (vid[q] < 0) continue;
      if (slot < 2 * W) {
        acc.add(rows[q], tl);
      } else {
        const int d = slot - 2 * W;
        const double part = wave_sum_pl(acc.dot(rows[q], tl));
        float f = 0;
        f += part;
        const int label = d == 0 ? 1 : 0;
        float g;
        if (f > 6)
          g = (label - 1) * a.alpha;
        else if (f < -6)
          g = (label - 0) * a.alpha;
        else
          g = (label - a.exptab[(int)((f + 6) * (1000 / 6 / 2))]) * a.alpha;
        ne.axpy((double)g, rows[q], tl);
        if (lane == d) gk = g;
      }
    }
  }
  acc.st_full(a.neu1 + (uint64_t)p * a.ld, lane, tl, a.full ? a.ld : a.D);
  ne.st_full(a.neu1e + (uint64_t)p * a.ld, lane, tl, a.full ? a.ld : a.D);
  if (lane <= N) a.pg[(uint64_t)p * (N + 1) + lane] = gk;
}

template <typename A> struct GatherArgs {
  const uint4 *desc;
  const uint32_t *ioff, *vals;
  uint32_t U;
  const A *neu1, *neu1e;
  const float *pg;
  uint64_t HOFF;
  uint32_t P;
  int D;
  A *partial;
  int ld;  // neu1/neu1e row stride (FwdArgs::ld)
  const uint32_t *lead;  // hot-group leaders (k_item_desc): [0] = count, then items
  uint32_t max_items;    // capacity of desc / partial: a bound on ioff[2U] every reader clamps to
  const uint32_t *multi;  // k_gather_t: only these items ([0] = count; the multi-chunk runs'), or null = all
  uint32_t SH, SV;        // record slots per position: N+1 (h records), 2W (v records)
  const uint32_t *order;  // k_gather: all items in this order ([1..]: the multi-item sort's output), or null
};

// One wave per chunk of <= 128 records of one (key, kind): the fp64 sum, in
// record (= position) order, of g*neu1[p] (h records: accu_h(g*neu1),
// word2vec_global.h:705) or neu1e[p] (v records: accu_v(neu1e), :716).
// Record indices and g are loaded for the whole chunk up front; rows are
// fetched UNR at a time.
template <typename T, typename A, int NCH, int UNR>
__global__ __launch_bounds__(256) void k_gather(GatherArgs<A> a) {
  constexpr int E = V16<T>::E;
  using CA = Chk<A, E>;
  const int lane = threadIdx.x & 63;
  const int NC = a.D / E;
  const uint32_t NI = min(a.ioff[2 * a.U], a.max_items);
  for (uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6); q < NI; q += gridDim.x * 4) {
    // the multi-chunk items first, in first-record position order (Infinity-Cache reuse), then the rest
    const uint32_t item = a.order ? __builtin_amdgcn_readfirstlane(a.order[1 + q]) : q;
    const uint4 d = a.desc[__builtin_amdgcn_readfirstlane(item)];
    const uint32_t s = d.x, e = d.y & 0x7FFFFFFFu, kind = d.y >> 31, n = e - s;
    uint32_t p0 = 0, p1 = 0;
    float g0 = 1.f, g1 = 1.f;
    // records are position-major: index = p*SH + d (h), HOFF + p*SV + j (v)
    if (lane < (int)n) {
      const uint32_t pi = a.vals[s + lane];
      if (kind == 0) {
        p0 = pi / a.SH;
        g0 = a.pg[pi];
      } else {
        p0 = (uint32_t)(pi - a.HOFF) / a.SV;
      }
    }
    if (lane + 64 < (int)n) {
      const uint32_t pi = a.vals[s + 64 + lane];
      if (kind == 0) {
        p1 = pi / a.SH;
        g1 = a.pg[pi];
      } else {
        p1 = (uint32_t)(pi - a.HOFF) / a.SV;
      }
    }
    const A *base = kind == 0 ? a.neu1 : a.neu1e;
    double acc[NCH][E];
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
      for (int k = 0; k < E; k++) acc[c][k] = 0.0;
    for (uint32_t r0 = 0; r0 < n; r0 += UNR) {
      typename CA::R rv[UNR][NCH];
      double gg[UNR];
#pragma unroll
      for (int q = 0; q < UNR; q++) {
        const uint32_t idx = min(r0 + q, n - 1);
        const uint32_t pr = idx < 64 ? __shfl(p0, (int)idx, 64) : __shfl(p1, (int)(idx - 64), 64);
        gg[q] = (double)(idx < 64 ? __shfl(g0, (int)idx, 64) : __shfl(g1, (int)(idx - 64), 64));
        const A *src = base + (uint64_t)pr * a.ld;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
          const int ci = lane + c * 64;
          if (ci < NC) rv[q][c] = CA::ld(src, ci, a.D);
        }
      }
#pragma unroll
      for (int q = 0; q < UNR; q++) {
        if (r0 + q < n) {
#pragma unroll
          for (int c = 0; c < NCH; c++)
            if (lane + c * 64 < NC)
#pragma unroll
              for (int k = 0; k < E; k++) {
                if (kind == 0) {
                  const double prod = gg[q] * CA::at(rv[q][c], k);
                  acc[c][k] += prod;
                } else {
                  acc[c][k] += CA::at(rv[q][c], k);
                }
              }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const int ci = lane + c * 64;
      if (ci < NC) CA::st(a.partial + (uint64_t)item * a.D, ci, a.D, acc[c]);
    }
  }
}

// Record info of one gather item: position and g of its records 0..127
// (lanes hold records lane and 64+lane).
struct ItemRecs {
  uint32_t p0, p1;
  float g0, g1;
};
__device__ __forceinline__ uint4 uniform4(uint4 d) {  // wave-uniform value: keep its branches scalar
  return make_uint4(__builtin_amdgcn_readfirstlane(d.x), __builtin_amdgcn_readfirstlane(d.y),
                    __builtin_amdgcn_readfirstlane(d.z), __builtin_amdgcn_readfirstlane(d.w));
}

// pg == nullptr: g rides in the neu1 rows (swps_w2v_bfp.h) and an h record's g word is its slot
// d = index % SH, as an integer
__device__ __forceinline__ ItemRecs run_recs(const uint32_t *vals, const float *pg, uint32_t SH, uint32_t SV,
                                             uint64_t HOFF, uint32_t s, uint32_t n, uint32_t kind, int lane) {
  ItemRecs r{0, 0, 1.f, 1.f};
  // records are position-major: index = p*SH + d (h), HOFF + p*SV + j (v)
  if (lane < (int)n) {
    const uint32_t pi = vals[s + lane];
    if (kind == 0) {
      r.p0 = pi / SH;
      r.g0 = pg ? pg[pi] : __int_as_float((int)(pi % SH));
    } else {
      r.p0 = (uint32_t)(pi - HOFF) / SV;
    }
  }
  if (lane + 64 < (int)n) {
    const uint32_t pi = vals[s + 64 + lane];
    if (kind == 0) {
      r.p1 = pi / SH;
      r.g1 = pg ? pg[pi] : __int_as_float((int)(pi % SH));
    } else {
      r.p1 = (uint32_t)(pi - HOFF) / SV;
    }
  }
  return r;
}

__device__ __forceinline__ ItemRecs item_recs(const GatherArgs<float> &a, uint4 d, int lane) {
  const uint32_t s = d.x, e = d.y & 0x7FFFFFFFu, kind = d.y >> 31, n = e - s;
  return run_recs(a.vals, a.pg, a.SH, a.SV, a.HOFF, s, n, kind, lane);
}

// k_gather (fast mode) on FSlice rows, software-pipelined across items: most
// items are short (Zipf tail keys: a few records), so the next item's
// descriptor and record info are fetched while this item's rows are in flight
// instead of after them (desc -> vals -> pg -> rows was four dependent
// memory round trips per item).
template <int NCH, int UNR>
__global__ __launch_bounds__(256) void k_gather_t(GatherArgs<float> a) {
  const int lane = threadIdx.x & 63;
  const bool tl = 256 * NCH + lane < a.D;
  const uint32_t NI = min(a.multi ? a.multi[0] : a.ioff[2 * a.U], a.max_items);
  const uint32_t stride = gridDim.x * 4;
  uint32_t qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= NI) return;
  // the multi-chunk items only (fused push), or every item in multi-first position order, or item order
  const uint32_t *list = a.multi ? a.multi : a.order;
  auto item_at = [&](uint32_t q) { return list ? list[1 + __builtin_amdgcn_readfirstlane(q)] : q; };
  uint32_t item = __builtin_amdgcn_readfirstlane(item_at(qi));
  uint4 d = uniform4(a.desc[item]);
  ItemRecs ri = item_recs(a, d, lane);
  for (;;) {
    const uint32_t qn = qi + stride;
    const bool more = qn < NI;
    const uint32_t nx = more ? __builtin_amdgcn_readfirstlane(item_at(qn)) : 0;
    const uint4 dn = uniform4(more ? a.desc[nx] : make_uint4(0, 0x80000000u, 0, 0));
    const uint32_t s = d.x, e = d.y & 0x7FFFFFFFu, kind = d.y >> 31, n = e - s;
    const float *base = kind == 0 ? a.neu1 : a.neu1e;
    FAcc<NCH> acc;
    acc.zero();
    ItemRecs rn;
    for (uint32_t r0 = 0; r0 < n; r0 += UNR) {
      FSlice<NCH> rv[UNR];
      double gg[UNR];
#pragma unroll
      for (int q = 0; q < UNR; q++) {
        const uint32_t idx = min(r0 + q, n - 1);
        // idx is wave-uniform: read the record's position and g with v_readlane (scalar results)
        const uint32_t pr = idx < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)ri.p0, (int)idx)
                                     : (uint32_t)__builtin_amdgcn_readlane((int)ri.p1, (int)(idx - 64));
        gg[q] = (double)__int_as_float(idx < 64 ? __builtin_amdgcn_readlane(__float_as_int(ri.g0), (int)idx)
                                                : __builtin_amdgcn_readlane(__float_as_int(ri.g1), (int)(idx - 64)));
        rv[q].ld(base + (uint64_t)pr * a.ld, lane, tl);
      }
      if (r0 == 0) rn = item_recs(a, dn, lane);  // next item's record info, behind this item's first rows
#pragma unroll
      for (int q = 0; q < UNR; q++) {
        if (r0 + q < n) {
          if (kind == 0)
            acc.axpy(gg[q], rv[q], tl);
          else
            acc.add(rv[q], tl);
        }
      }
    }
    if (n == 0) rn = item_recs(a, dn, lane);
    acc.st(a.partial + (uint64_t)item * a.D, lane, tl);
    if (!more) break;
    qi = qn;
    item = nx;
    d = dn;
    ri = rn;
  }
}

constexpr uint32_t kGroup = 16;  // hot keys: partials are pre-summed in groups of 16
// k_combine: a stride loop over the leader list k_item_desc collected
constexpr unsigned kCombineGrid = 1024;

// Hot (key, kind) runs with more than kGroup chunks: each group leader sums
// its group's partials in chunk order into its own slot (second level).
template <typename T, typename A, int NCH>
__global__ __launch_bounds__(256) void k_combine(GatherArgs<A> a) {
  constexpr int E = V16<T>::E;
  using CA = Chk<A, E>;
  const int lane = threadIdx.x & 63;
  const int NC = a.D / E;
  const uint32_t NL = min(a.lead[0], a.max_items / 8 + 1);
  for (uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6); q < NL; q += gridDim.x * 4) {
    const uint32_t item = a.lead[1 + __builtin_amdgcn_readfirstlane(q)];
    const uint4 d = a.desc[__builtin_amdgcn_readfirstlane(item)];
    const uint32_t j = d.z;
    const uint32_t i1 = a.ioff[j + 1];
    const uint32_t end = min(item + kGroup, i1);
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const int ci = lane + c * 64;
      if (ci >= NC) continue;
      typename CA::R rv[kGroup];
#pragma unroll
      for (uint32_t q2 = 0; q2 < kGroup; q2++) rv[q2] = CA::ld(a.partial + (uint64_t)min(item + q2, end - 1) * a.D, ci, a.D);
      double sum[E];
#pragma unroll
      for (int kk = 0; kk < E; kk++) sum[kk] = 0.0;
#pragma unroll
      for (uint32_t q2 = 0; q2 < kGroup; q2++)
        if (item + q2 < end)
#pragma unroll
          for (int kk = 0; kk < E; kk++) sum[kk] += CA::at(rv[q2], kk);
      CA::st(a.partial + (uint64_t)item * a.D, ci, a.D, sum);
    }
  }
}

constexpr int kMaxSplitOwners = 64;
template <typename T, typename A> struct PushArgs {
  const int32_t *K;
  uint32_t U;
  const uint32_t *vid_row, *seg, *ioff;
  const A *partial;
  T *rows;
  int32_t *local;
  int D;
  double lr, fudge;
  A *grads;  // TO_GRADS: mean gradients [U][2D] in the intermediate type (the push request payload)
  T *cache_h, *cache_v;  // direct table reads (single GPU): every pushed key's pre-update h, v rows go to
  int cs;                // the worker cache (the value its pull would have left there), row stride cs
  // k_push_thp: the sorted records and the forward's rows, to sum single-chunk runs in place
  const uint32_t *vals;
  const float *pg;
  const A *neu1, *neu1e;
  uint64_t HOFF;
  uint32_t P;
  int ld;
  const uint32_t *krow;  // k_push_thp: shard row per batch key (k_batch_setup)
  uint32_t SH, SV;       // record slots per position (GatherArgs)
  int full;              // cache-row stores cover the pad too (zeros): SWPS_FULL_LINES
  // k_push_thp<TO_GRADS> in two passes (sharded learner, world > 1): pass 1 = the first
  // ohalf[r] keys of every owner r's key range [obnd[r], obnd[r+1]) (K is grouped by owner),
  // pass 2 = the rest; 0 = every key.  Their all-to-alls then overlap pass 2.
  uint32_t group;  // runs of more than `group` partials read k_combine's group leaders (kGroup), else all
  int gpass;
  uint32_t nown;
  uint32_t obnd[kMaxSplitOwners + 1], ohalf[kMaxSplitOwners];
};

// Mean gradient (word2vec_global.h:122-134) + AdaGrad ascent
// (word2vec_global.h:176-185) per key, fp64 math; one wave per key.
// TO_GRADS: stop at the mean and write the push payload (sharded mode: the
// owner GPU applies AdaGrad, see swps_w2v_serve_push).
template <typename T, typename A, int NCH, bool TO_GRADS>
__global__ __launch_bounds__(256) void k_push(PushArgs<T, A> a) {
  constexpr int E = V16<T>::E;
  using CT = Chk<T, E>;
  using CA = Chk<A, E>;
  constexpr int PU = 8;
  const int lane = threadIdx.x & 63;
  const int D = a.D, NC = D / E;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < a.U; u += (uint64_t)gridDim.x * 4) {
    const int32_t vid = a.K[u];
    if (lane == 0) a.local[vid] = -1;
    const uint32_t hc = a.seg[1 * a.U + u] - a.seg[0 * a.U + u];
    const uint32_t vc = a.seg[3 * a.U + u] - a.seg[2 * a.U + u];
    if (hc == 0 && vc == 0 && !TO_GRADS && !a.cache_h) continue;
    T *row = TO_GRADS ? nullptr : a.rows + (uint64_t)a.vid_row[vid] * 4 * D;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const int ci = lane + c * 64;
      if (ci >= NC) continue;
      for (int half = 0; half < 2; half++) {
        const uint32_t cnt = half ? vc : hc;
        if (!TO_GRADS && a.cache_h) {  // the pulled (pre-update) value stays in the worker cache
          using V = typename V16<T>::V;
          ((V *)((half ? a.cache_v : a.cache_h) + (uint64_t)vid * a.cs))[ci] = ((const V *)(row + half * D))[ci];
        }
        if (cnt == 0) {
          if (TO_GRADS)
#pragma unroll
            for (int k = 0; k < E; k++) a.grads[u * 2 * D + half * D + ci * E + k] = (A)0;
          continue;
        }
        const uint32_t i0 = a.ioff[2 * u + half], i1 = a.ioff[2 * u + half + 1];
        const uint32_t stride = (i1 - i0) > a.group ? kGroup : 1;
        double sum[E];
#pragma unroll
        for (int k = 0; k < E; k++) sum[k] = 0.0;
        for (uint32_t it0 = i0; it0 < i1; it0 += PU * stride) {
          typename CA::R pv[PU];
#pragma unroll
          for (int q = 0; q < PU; q++) {
            const uint32_t it = min(it0 + q * stride, i1 - 1);
            pv[q] = CA::ld(a.partial + (uint64_t)it * D, ci, D);
          }
#pragma unroll
          for (int q = 0; q < PU; q++)
            if (it0 + q * stride < i1)
#pragma unroll
              for (int k = 0; k < E; k++) sum[k] += CA::at(pv[q], k);
        }
        if (TO_GRADS) {
#pragma unroll
          for (int k = 0; k < E; k++) a.grads[u * 2 * D + half * D + ci * E + k] = (A)(sum[k] / (double)cnt);
          continue;
        }
        T *w = row + half * D, *w2 = row + (2 + half) * D;
        const typename CT::R wr = CT::ld(w, ci, D), w2r = CT::ld(w2, ci, D);
        double wn[E], w2n[E];
#pragma unroll
        for (int k = 0; k < E; k++) {
          const double g = (double)(A)(sum[k] / (double)cnt);  // the mean in the push payload's type
          const double gsq = g * g;
          const double acc2 = CT::at(w2r, k) + gsq;
          const double step = (g * a.lr) / sqrt(acc2 + a.fudge);
          w2n[k] = acc2;
          wn[k] = CT::at(wr, k) + step;
        }
        CT::st(w2, ci, D, w2n);
        CT::st(w, ci, D, wn);
      }
    }
  }
}

// k_push (fast mode, fp32 rows and partials, single GPU) on FSlice rows: both
// halves' first partial and their w / w2 rows are loaded together before any
// arithmetic (k_push walks chunk x half with a dependent load -> store round
// trip each, and its second 64-lane chunk keeps 11 lanes busy at D = 300).
// Same per-element arithmetic and partial order as k_push: bit-identical.
template <int NCH>
__global__ __launch_bounds__(256) void k_push_t(PushArgs<float, float> a) {
  constexpr int PU = 8;
  const int lane = threadIdx.x & 63;
  const int D = a.D;
  const bool tl = 256 * NCH + lane < D;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < a.U; u += (uint64_t)gridDim.x * 4) {
    const int32_t vid = a.K[u];
    if (lane == 0) a.local[vid] = -1;
    const uint32_t s0 = a.seg[0 * a.U + u], s1 = a.seg[1 * a.U + u], s2 = a.seg[2 * a.U + u], s3 = a.seg[3 * a.U + u];
    const uint32_t cnt[2] = {s1 - s0, s3 - s2};
    if (cnt[0] == 0 && cnt[1] == 0 && !a.cache_h) continue;
    float *row = a.rows + (uint64_t)a.vid_row[vid] * 4 * D;
    uint32_t i0[2], i1[2];
    FSlice<NCH> wr[2], w2r[2], pf[2];
#pragma unroll
    for (int half = 0; half < 2; half++) {
      i0[half] = a.ioff[2 * u + half];
      i1[half] = a.ioff[2 * u + half + 1];
      if (cnt[half] || a.cache_h) wr[half].ld(row + half * D, lane, tl);
      if (cnt[half]) {
        pf[half].ld(a.partial + (uint64_t)i0[half] * D, lane, tl);
        w2r[half].ld(row + (2 + half) * D, lane, tl);
      }
    }
    if (a.cache_h) {  // the pulled (pre-update) value stays in the worker cache
      wr[0].st_full(a.cache_h + (uint64_t)vid * a.cs, lane, tl, a.full ? a.cs : D);
      wr[1].st_full(a.cache_v + (uint64_t)vid * a.cs, lane, tl, a.full ? a.cs : D);
    }
#pragma unroll
    for (int half = 0; half < 2; half++) {
      if (cnt[half] == 0) continue;
      FAcc<NCH> acc;
      acc.zero();
      acc.add(pf[half], tl);
      const uint32_t stride = (i1[half] - i0[half]) > a.group ? kGroup : 1;
      for (uint32_t it0 = i0[half] + stride; it0 < i1[half]; it0 += PU * stride) {
        FSlice<NCH> pv[PU];
#pragma unroll
        for (int q = 0; q < PU; q++)
          pv[q].ld(a.partial + (uint64_t)min(it0 + q * stride, i1[half] - 1) * D, lane, tl);
#pragma unroll
        for (int q = 0; q < PU; q++)
          if (it0 + q * stride < i1[half]) acc.add(pv[q], tl);
      }
      const double inv = (double)cnt[half];
      float *w = row + half * D, *w2 = row + (2 + half) * D;
      auto upd = [&](double sum, float wv, float w2v, float &wo, float &w2o) {
        const double g = (double)(float)(sum / inv);  // the mean in the push payload's type
        const double acc2 = (double)w2v + g * g;
        const double step = (g * a.lr) / sqrt(acc2 + a.fudge);
        w2o = (float)acc2;
        wo = (float)((double)wv + step);
      };
#pragma unroll
      for (int c = 0; c < NCH; c++) {
        float4 wo, w2o;
        upd(acc.v[c][0], wr[half].v[c].x, w2r[half].v[c].x, wo.x, w2o.x);
        upd(acc.v[c][1], wr[half].v[c].y, w2r[half].v[c].y, wo.y, w2o.y);
        upd(acc.v[c][2], wr[half].v[c].z, w2r[half].v[c].z, wo.z, w2o.z);
        upd(acc.v[c][3], wr[half].v[c].w, w2r[half].v[c].w, wo.w, w2o.w);
        ((float4 *)w2)[lane + c * 64] = w2o;
        ((float4 *)w)[lane + c * 64] = wo;
      }
      if (tl) {
        float wo, w2o;
        upd(acc.t, wr[half].t, w2r[half].t, wo, w2o);
        w2[256 * NCH + lane] = w2o;
        w[256 * NCH + lane] = wo;
      }
    }
  }
}

// k_push_t with the gather of single-chunk runs folded in, one wave per
// (key, half).  A (key, kind) run of at most kChunk records is summed here,
// straight from the forward's neu1 / neu1e rows: the same fp64 sum in record
// order, rounded to the fp32 partial k_gather_t would have stored, so
// k_gather_t only runs the multi-chunk items and the single-chunk partials
// are never written nor re-read.  The h half (h, h2sum: the target records'
// g*neu1 sums) and the v half (v, v2sum: the context records' neu1e sums) of
// a key's AdaGrad update touch disjoint elements, so they are independent
// items: half the live registers per wave and twice the waves.  Items are
// software-pipelined like k_gather_t's: a wave walks a stride of them; the
// next item's bounds / key / shard row are loaded at the top and its record
// info right behind this item's row loads, so the per-item chain (bounds ->
// records -> g -> rows, key -> shard row -> w rows) overlaps the previous
// item's traffic.  Same per-element arithmetic and partial order as
// k_gather_t + k_combine + k_push_t: bit-identical.
struct PHead {
  uint32_t s0, s1, i0, i1;
  int32_t vid;
  uint32_t row;
};
// TO_GRADS (sharded learner): stop at the mean and write the push payload
// [U][h|v] (fp32), zeros for an empty half, as k_push<..., true> does; the
// owner applies AdaGrad (swps_w2v_serve_push).
// MODE 0: every (key, half); 1: all but the multi-chunk halves (they wait for k_gather_t's
// partials while this runs beside it, on another stream); 2: only the multi-chunk halves.
template <int NCH, int UNR, bool TO_GRADS = false, int MODE = 0>
__global__ __launch_bounds__(256) void k_push_thp(PushArgs<float, float> a) {
  constexpr int PU = 8;
  const int lane = threadIdx.x & 63;
  const int D = a.D;
  const bool tl = 256 * NCH + lane < D;
  const uint64_t n2 = 2ull * a.U;
  const uint64_t stride = (uint64_t)gridDim.x * 4;
  uint64_t uh = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (uh >= n2) return;
  auto head = [&](uint64_t x) {
    const uint64_t u = x >> 1;
    const int half = (int)(x & 1);
    PHead h;
    h.s0 = __builtin_amdgcn_readfirstlane(a.seg[(2 * half) * a.U + u]);
    h.s1 = __builtin_amdgcn_readfirstlane(a.seg[(2 * half + 1) * a.U + u]);
    h.i0 = __builtin_amdgcn_readfirstlane(a.ioff[2 * u + half]);
    h.i1 = __builtin_amdgcn_readfirstlane(a.ioff[2 * u + half + 1]);
    h.vid = __builtin_amdgcn_readfirstlane(a.K[u]);
    h.row = TO_GRADS ? 0u : __builtin_amdgcn_readfirstlane(a.krow[u]);
    return h;
  };
  PHead h = head(uh);
  ItemRecs ri{0, 0, 1.f, 1.f};
  if (h.s1 > h.s0 && h.i1 - h.i0 == 1) ri = run_recs(a.vals, a.pg, a.SH, a.SV, a.HOFF, h.s0, h.s1 - h.s0, (int)(uh & 1), lane);
  for (;;) {
    const uint64_t nx = uh + stride;
    const bool more = nx < n2;
    PHead hn{0, 0, 0, 0, 0, 0};
    if (more) hn = head(nx);
    const int half = (int)(uh & 1);
    const bool multi = h.i1 - h.i0 > 1;
    bool other = (MODE == 1 && multi) || (MODE == 2 && !multi);
    // the key's local slot is freed by its half-0 item in pass 1 even when pass 2 pushes that half
    // (pass 2 never frees one): every key of the batch leaves the map, as in MODE 0
    if (MODE == 1 && multi && lane == 0 && half == 0) a.local[h.vid] = -1;
    if (TO_GRADS && a.gpass) {  // the key's owner range: its first ohalf keys go in pass 1
      const uint32_t u = (uint32_t)(uh >> 1);
      uint32_t r = 0;
      while (r + 1 < a.nown && a.obnd[r + 1] <= u) r++;
      const bool first = u - a.obnd[r] < a.ohalf[r];
      other = other || (first != (a.gpass == 1));
    }
    if (other) {  // the other pass's item
      if (more && hn.s1 > hn.s0 && hn.i1 - hn.i0 == 1 && MODE != 2)
        ri = run_recs(a.vals, a.pg, a.SH, a.SV, a.HOFF, hn.s0, hn.s1 - hn.s0, (int)(nx & 1), lane);
      if (!more) break;
      uh = nx;
      h = hn;
      continue;
    }
    if (lane == 0 && half == 0 && MODE != 2) a.local[h.vid] = -1;
    const uint32_t cnt = h.s1 - h.s0;
    const bool one = h.i1 - h.i0 == 1;
    float *row = TO_GRADS ? nullptr : a.rows + (uint64_t)h.row * 4 * D;
    float *gout = TO_GRADS ? a.grads + ((uh >> 1) * 2 + half) * (uint64_t)D : nullptr;
    FSlice<NCH> wr, w2r, pf;
    ItemRecs rn{0, 0, 1.f, 1.f};
    bool rn_done = false;
    auto next_recs = [&]() {
      if (more && hn.s1 > hn.s0 && hn.i1 - hn.i0 == 1)
        rn = run_recs(a.vals, a.pg, a.SH, a.SV, a.HOFF, hn.s0, hn.s1 - hn.s0, (int)(nx & 1), lane);
      rn_done = true;
    };
    if (!TO_GRADS) {
      if (cnt || a.cache_h) wr.ld(row + half * D, lane, tl);
      if (cnt) w2r.ld(row + (2 + half) * D, lane, tl);
    }
    if (cnt && !one) pf.ld(a.partial + (uint64_t)h.i0 * D, lane, tl);
    if (!TO_GRADS && a.cache_h)  // the pre-update value, pad as zeros (whole lines)
      wr.st_full((half ? a.cache_v : a.cache_h) + (uint64_t)h.vid * a.cs, lane, tl, a.full ? a.cs : D);
    if (TO_GRADS && cnt == 0) {  // an empty half: zero mean
      FSlice<NCH> z;
#pragma unroll
      for (int c = 0; c < NCH; c++) z.v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      z.t = 0.f;
      z.st(gout, lane, tl);
    }
    if (cnt) {
      FAcc<NCH> acc;
      acc.zero();
      if (one) {
        const float *base = half == 0 ? a.neu1 : a.neu1e;
        FAcc<NCH> c;
        c.zero();
        for (uint32_t r0 = 0; r0 < cnt; r0 += UNR) {
          FSlice<NCH> rv[UNR];
          float gf[UNR];
#pragma unroll
          for (int q = 0; q < UNR; q++) {
            const uint32_t idx = min(r0 + q, cnt - 1);
            const uint32_t pr = idx < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)ri.p0, (int)idx)
                                         : (uint32_t)__builtin_amdgcn_readlane((int)ri.p1, (int)(idx - 64));
            gf[q] = __int_as_float(idx < 64 ? __builtin_amdgcn_readlane(__float_as_int(ri.g0), (int)idx)
                                            : __builtin_amdgcn_readlane(__float_as_int(ri.g1), (int)(idx - 64)));
            rv[q].ld(base + (uint64_t)pr * a.ld, lane, tl);
          }
          if (r0 == 0) next_recs();  // behind this item's first rows
#pragma unroll
          for (int q = 0; q < UNR; q++) {
            if (r0 + q < cnt) {
              if (half == 0)
                c.axpy((double)gf[q], rv[q], tl);
              else
                c.add(rv[q], tl);
            }
          }
        }
#pragma unroll
        for (int cc = 0; cc < NCH; cc++)
#pragma unroll
          for (int k = 0; k < 4; k++) acc.v[cc][k] = (double)(float)c.v[cc][k];  // the fp32 partial
        acc.t = (double)(float)c.t;
      } else {
        next_recs();
        acc.add(pf, tl);
        const uint32_t st = (h.i1 - h.i0) > a.group ? kGroup : 1;
        for (uint32_t it0 = h.i0 + st; it0 < h.i1; it0 += PU * st) {
          FSlice<NCH> pv[PU];
#pragma unroll
          for (int q = 0; q < PU; q++) pv[q].ld(a.partial + (uint64_t)min(it0 + q * st, h.i1 - 1) * D, lane, tl);
#pragma unroll
          for (int q = 0; q < PU; q++)
            if (it0 + q * st < h.i1) acc.add(pv[q], tl);
        }
      }
      const double inv = (double)cnt;
      if (TO_GRADS) {  // the mean in the push payload's type
        FSlice<NCH> m;
#pragma unroll
        for (int c = 0; c < NCH; c++)
          m.v[c] = make_float4((float)(acc.v[c][0] / inv), (float)(acc.v[c][1] / inv), (float)(acc.v[c][2] / inv),
                               (float)(acc.v[c][3] / inv));
        m.t = (float)(acc.t / inv);
        m.st(gout, lane, tl);
      } else {
        float *w = row + half * D, *w2 = row + (2 + half) * D;
        auto upd = [&](double sum, float wv, float w2v, float &wo, float &w2o) {
          const double g = (double)(float)(sum / inv);  // the mean in the push payload's type
          const double acc2 = (double)w2v + g * g;
          const double step = (g * a.lr) / sqrt(acc2 + a.fudge);
          w2o = (float)acc2;
          wo = (float)((double)wv + step);
        };
#pragma unroll
        for (int c = 0; c < NCH; c++) {
          float4 wo, w2o;
          upd(acc.v[c][0], wr.v[c].x, w2r.v[c].x, wo.x, w2o.x);
          upd(acc.v[c][1], wr.v[c].y, w2r.v[c].y, wo.y, w2o.y);
          upd(acc.v[c][2], wr.v[c].z, w2r.v[c].z, wo.z, w2o.z);
          upd(acc.v[c][3], wr.v[c].w, w2r.v[c].w, wo.w, w2o.w);
          ((float4 *)w2)[lane + c * 64] = w2o;
          ((float4 *)w)[lane + c * 64] = wo;
        }
        if (tl) {
          float wo, w2o;
          upd(acc.t, wr.t, w2r.t, wo, w2o);
          w2[256 * NCH + lane] = w2o;
          w[256 * NCH + lane] = wo;
        }
      }
    }
    if (!rn_done) next_recs();
    if (!more) break;
    uh = nx;
    h = hn;
    ri = rn;
  }
}

}  // namespace

#include "swps_w2v_bfp.h"

namespace {

#define SWPS_BFP_SHAPES(code, F, RB) \
  switch (code) {                     \
    case 1: F(0, 1, RB); break;       \
    case 2: F(0, 2, RB); break;       \
    case 10: F(1, 0, RB); break;      \
    case 11: F(1, 1, RB); break;      \
    case 12: F(1, 2, RB); break;      \
    default: F(2, 0, RB); break;      \
  }
// every (NCH, NT, RB) instantiation of F for context w's dim and residual bytes
#define SWPS_BFP_DISPATCH(w, F)                    \
  do {                                             \
    if ((w)->bfp_rb)                               \
      SWPS_BFP_SHAPES(bfp_shape((w)->D), F, 1)     \
    else                                           \
      SWPS_BFP_SHAPES(bfp_shape((w)->D), F, 0)     \
  } while (0)

// requester side of a sharded pull: the owners' pull values [U][h|v] (K order)
// into the worker cache (global_pull_access.h:88-97: params[key] = val)
// srow != nullptr (world 1, the pull read in place): value u is the table row srow[u] of vals
// (the shard rows, [h | v | h2 | v2]: its first 2D elements)
template <typename T>
__global__ __launch_bounds__(256) void k_install(const int32_t *__restrict__ K, uint32_t U, const T *__restrict__ vals,
                                                 int D, T *__restrict__ cache_h, T *__restrict__ cache_v,
                                                 int32_t *__restrict__ local, int set_local, int cs,
                                                 const uint32_t *__restrict__ srow = nullptr) {
  using V = typename V16<T>::V;
  constexpr int E = V16<T>::E;
  const int lane = threadIdx.x & 63;
  const int NC = D / E;
  for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < U; u += (uint64_t)gridDim.x * 4) {
    const int32_t vid = K[u];
    // a key the shard holds no row for (full table: table_copy_pull's zero row) installs zeros
    const uint32_t sr = srow ? srow[u] : 0u;
    const bool have = !srow || sr != kNoRow;
    const V *src = (const V *)(vals + (srow ? (uint64_t)(have ? sr : 0u) * 4 : u * 2) * D);
    V *dh = (V *)(cache_h + (uint64_t)vid * cs);  // cs: the cache row stride (swps_w2v::cs)
    V *dv = (V *)(cache_v + (uint64_t)vid * cs);
    for (int c = lane; c < cs / E; c += 64) {  // the pad too (zeros): whole-line stores
      const bool in = have && c < NC;
      dh[c] = in ? src[c] : V{};
      dv[c] = in ? src[NC + c] : V{};
    }
    if (set_local && lane == 0) local[vid] = (int32_t)u;
  }
}

// k_install of a split pull's part (ShardDriver early / late values): value i belongs to the
// batch's key pos[i] (K order) — the same rows written as by k_install of the assembled values
template <typename T>
__global__ __launch_bounds__(256) void k_install_idx(const int32_t *__restrict__ K, const uint32_t *__restrict__ pos,
                                                     uint32_t n, const T *__restrict__ vals, int D,
                                                     T *__restrict__ cache_h, T *__restrict__ cache_v, int cs) {
  using V = typename V16<T>::V;
  constexpr int E = V16<T>::E;
  const int lane = threadIdx.x & 63;
  const int NC = D / E;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * 4) {
    const int32_t vid = K[pos[i]];
    const V *src = (const V *)(vals + i * 2 * D);
    V *dh = (V *)(cache_h + (uint64_t)vid * cs);
    V *dv = (V *)(cache_v + (uint64_t)vid * cs);
    for (int c = lane; c < cs / E; c += 64) {
      const bool in = c < NC;
      dh[c] = in ? src[c] : V{};
      dv[c] = in ? src[NC + c] : V{};
    }
  }
}

// Vec::randInit (vec1.h:229-232) for every vocab key on the GPU: rand() is
// glibc's additive generator o[i] = o[i-31] + o[i-3] (mod 2^32, output o >> 1;
// GlibcRand in swps_host.cpp), linear in its state, so output m is
// sum_j a_j o[3+j] with sum_j a_j x^j = x^(m-3) mod (x^31 - x^28 - 1):
// every thread jumps to its own run of outputs (square-and-multiply on
// 31-coefficient polynomials) and then steps the recurrence.  Output k
// (after `skip` earlier calls) is element k % 2D of key k / 2D's [h | v],
// (rand()/(float)RAND_MAX - 0.5) / D, written straight into the table row.
template <typename T>
__global__ __launch_bounds__(64) void k_rand_init(const uint32_t *__restrict__ base, uint64_t first, uint64_t total,
                                                   int D, const uint32_t *__restrict__ vid_row, T *__restrict__ rows) {
  const uint64_t k0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kRandRun;
  if (k0 >= total) return;
  // o[m] for the 31 values before output k0: m = first + k0 - 31 + d, d = 0..30
  uint32_t ring[31];
  glibc_ring_at(base, first + k0 - 31, ring);
  const uint64_t k1 = min(total, k0 + kRandRun);
  int h = 0;  // ring[h] = o[i-31], ring[(h+28)%31] = o[i-3]
  for (uint64_t k = k0; k < k1; k++) {
    const int h28 = h + 28 >= 31 ? h + 28 - 31 : h + 28;
    const uint32_t v = ring[h] + ring[h28];
    ring[h] = v;
    h = h + 1 == 31 ? 0 : h + 1;
    const float f = (float)(int32_t)(v >> 1) / (float)2147483647;
    const uint64_t key = k / (2 * (uint64_t)D), el = k % (2 * (uint64_t)D);
    rows[(uint64_t)vid_row[key] * 4 * D + el] = (T)(((double)f - 0.5) / (double)(size_t)D);
  }
}

template <typename T>
__global__ void k_zero_sums(const uint32_t *__restrict__ vid_row, uint64_t V, int D, T *__restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * 2 * (uint64_t)D) return;
  const uint64_t key = i / (2 * (uint64_t)D), el = i % (2 * (uint64_t)D);
  rows[(uint64_t)vid_row[key] * 4 * D + 2 * D + el] = (T)0;
}

// ---- the step: one function per stage, each picking its kernel once ----------------------

// F(NCH) for the chunked kernels (k_forward, k_gather, k_combine, k_push): NCH 16-byte chunks per lane
#define SWPS_NCH_DISPATCH(nch, F) \
  switch (nch) {                  \
    case 1: F(1); break;          \
    case 2: F(2); break;          \
    case 3: F(3); break;          \
    default: F(4); break;         \
  }
// F(NCH) for the FSlice kernels (k_forward_t, k_gather_t, k_push_t): D = 256*NCH + tail, 0 < tail <= 64
#define SWPS_TAIL_DISPATCH(D, F) \
  do {                           \
    if ((D) < 512)               \
      F(1);                      \
    else if ((D) < 768)          \
      F(2);                      \
    else                         \
      F(3);                      \
  } while (0)

template <typename T, typename A>
constexpr bool kFast = std::is_same<T, float>::value && std::is_same<A, float>::value;  // fp32 rows and intermediates

// the row form a step's kernels work on
enum Rows { kChunked, kTail, kBfp };  // Chk chunks (any precision), FSlice (fast mode), BFP rows (swps_w2v_bfp.h)
template <typename T, typename A> Rows rows_of(const swps_w2v *w) {
  if (!kFast<T, A>) return kChunked;
  return w->bfp ? kBfp : w->tail ? kTail : kChunked;
}
// neu1 / neu1e row stride in elements of A (FwdArgs::ld)
template <typename A> int inter_ld(const swps_w2v *w) {
  return w->bfp ? bfp_ld(w->D, w->bfp_rb) : row_ld(w->D, sizeof(A), w->row_pad);
}
// N + 1 when the step's g rides in the neu1 rows (BFP modes, where the row pad holds it), else 0: the
// forward, the gather and the push all read it — pg is then neither written nor read.  By default
// from 65536 keys per batch: below, pg stays in L2 and its gather is the faster of the two (same
// box, B = 100 lines, per launch: gather 33.0 -> 39.3 us, push 165.6 -> 172.6 us with g in the row)
inline int row_g(const swps_w2v *w, uint32_t U) {
  return w->bfp && (w->row_g > 0 || (w->row_g < 0 && U >= 65536)) ? bfp_row_g(w->D, w->bfp_rb, w->N) : 0;
}
// at most max_items / kGroup leaders, 4 per block
inline bool use_combine(const swps_w2v *w, uint64_t M) {
  return w->combine == 1 || (w->combine == 2 && M >= w->combine_min);
}
inline unsigned combine_grid(uint64_t max_items) {
  return (unsigned)std::min<uint64_t>(kCombineGrid, max_items / kGroup / 4 + 1);
}

// How a step sums and pushes its gradients, decided once (the gather and the push both read it).
struct SumPlan {
  bool fused_ip = false;  // the push sums the single-chunk runs itself (k_push_thp / k_push_b), AdaGrad in place
  bool fused_g = false;   // ... and stops at the mean gradients (the sharded learner)
  // small batches: the multi-chunk gather (latency-bound, a few hundred items) runs on a side stream
  // beside the push of every other (key, half); the multi-chunk halves are pushed after it
  bool split = false;
  bool fused() const { return fused_ip || fused_g; }
};
template <typename T, typename A> SumPlan sum_plan(const swps_w2v *w, const swps_w2v::Prepped &pb, bool to_grads) {
  SumPlan pl;
  const bool fast_tail = kFast<T, A> && w->tail && w->fused_push && w->D < 512 && pb.sorted && !w->bfp;
  const bool sp = kFast<T, A> && w->bfp;
  pl.fused_ip = !to_grads && ((fast_tail && w->push_t) || sp);
  pl.fused_g = to_grads && (fast_tail || sp);
  pl.split = !sp && pl.fused() && (w->split_push > 0 || (w->split_push < 0 && pb.U < 65536));
  return pl;
}

// ---- pull (global_pull_access.h:28-107 + server.h:129-154) ----
// Single GPU: no copy — the forward reads the batch's keys straight from
// the table rows (k_records tagged them kTabRow) and the push leaves their
// pre-update values in the worker cache, which is exactly the state the
// reference's pull leaves behind.  Sharded: install the owners' values.
template <typename T> int install_pulled(swps_w2v *w, const int32_t *K, uint32_t U, const void *d_vals) {
  hipStream_t s = w->s;
  const int D = w->D;
  hipEvent_t e = w->timer.begin(s);
  if (w->parts.n[0] + w->parts.n[1] == U) {  // a split pull: the early and the late values
    for (int q = 0; q < 2; q++)
      if (w->parts.n[q])
        k_install_idx<T><<<nblk((uint64_t)w->parts.n[q] * 64), 256, 0, s>>>(
            K, w->parts.pos[q], (uint32_t)w->parts.n[q], (const T *)w->parts.vals[q], D, w->d_cache_h.as<T>(),
            w->d_cache_v.as<T>(), w->cs);
  } else if (w->pull_rows) {  // world 1: straight from the shard rows the serve looked up
    k_install<T><<<nblk((uint64_t)U * 64), 256, 0, s>>>(K, U, w->t->rows.as<T>(), D, w->d_cache_h.as<T>(),
                                                        w->d_cache_v.as<T>(), w->d_local.as<int32_t>(), 0, w->cs,
                                                        w->pull_rows);
  } else {
    k_install<T><<<nblk((uint64_t)U * 64), 256, 0, s>>>(K, U, (const T *)d_vals, D, w->d_cache_h.as<T>(),
                                                        w->d_cache_v.as<T>(), w->d_local.as<int32_t>(), 0, w->cs);
  }
  w->pull_rows = nullptr;
  w->parts = swps_w2v::Parts{};
  SWPS_HIP(hipGetLastError());
  w->timer.end(KT_PULL, e, s);
  return SWPS_OK;
}

// ---- forward (learn_instance) ----
template <typename T, typename A> int forward(swps_w2v *w, const swps_w2v::Prepped &pb) {
  hipStream_t s = w->s;
  const int D = w->D;
  const uint64_t P = pb.P;
  const int ld = inter_ld<A>(w);
  SWPS_TRY(w->d_neu1.ensure(P * ld * sizeof(A)));
  SWPS_TRY(w->d_neu1e.ensure(P * ld * sizeof(A)));
  SWPS_TRY(w->d_pg.ensure(pb.HOFF * 4));
  FwdArgs<T, A> fa{w->d_rec.as<int32_t>(), (int)P, w->d_cache_h.as<T>(), w->d_cache_v.as<T>(), w->t->rows.as<T>(),
                   w->d_exptab.as<float>(), D, w->W, w->N, w->cfg.alpha, w->d_neu1.as<A>(), w->d_neu1e.as<A>(),
                   w->d_pg.as<float>(), w->xcd_order, ld, w->cs, w->full_lines, row_g(w, pb.U)};
  const unsigned grid = nblk(P * 64);
  const Rows rows = rows_of<T, A>(w);
  hipEvent_t ef = w->timer.begin(s);
  if constexpr (kFast<T, A>) {
    if (rows == kBfp) {
#define SWPS_F(a_, b_, r_) k_forward_b<a_, b_, r_, 4><<<grid, 256, 0, s>>>(fa)
      SWPS_BFP_DISPATCH(w, SWPS_F);
#undef SWPS_F
    }
    if (rows == kTail) {  // NCH = 1: G = 4 rows in flight, occupancy 7 (A/B: G = 2..8)
#define SWPS_F(n_) k_forward_t<n_, (n_) == 1 ? 4 : 8, 1><<<grid, 256, 0, s>>>(fa)
      SWPS_TAIL_DISPATCH(D, SWPS_F);
#undef SWPS_F
    }
  }
  if (rows == kChunked) {  // fp64 intermediates: the batched target reduction wins
#define SWPS_F(n_)                                           \
  if (sizeof(A) == 8)                                        \
    k_forward_b8<T, A, n_, 8><<<grid, 256, 0, s>>>(fa);      \
  else                                                       \
    k_forward<T, A, n_, 8><<<grid, 256, 0, s>>>(fa)
    SWPS_NCH_DISPATCH(w->NCH, SWPS_F);
#undef SWPS_F
  }
  SWPS_HIP(hipGetLastError());
  w->timer.end(KT_FWD, ef, s);
  return SWPS_OK;
}

// ---- chunked segmented gradient sums, on stream gs ----
template <typename T, typename A>
int gradient_sums(swps_w2v *w, const swps_w2v::Prepped &pb, const SumPlan &pl, hipStream_t gs) {
  Timer &tm = w->timer;
  const int D = w->D;
  const bool fused = pl.fused();
  SWPS_TRY(w->d_partial.ensure(pb.max_items * D * (w->bfp ? 8 : sizeof(A))));
  GatherArgs<A> ga{w->d_desc.as<uint4>(), w->d_ioff.as<uint32_t>(), w->d_pvals_s.as<uint32_t>(), pb.U,
                   w->d_neu1.as<A>(), w->d_neu1e.as<A>(), row_g(w, pb.U) ? nullptr : w->d_pg.as<float>(), pb.HOFF,
                   (uint32_t)pb.P, D, w->d_partial.as<A>(), inter_ld<A>(w), w->d_lead.as<uint32_t>(),
                   (uint32_t)pb.max_items, fused ? w->d_multi.as<uint32_t>() : nullptr, (uint32_t)(w->N + 1),
                   (uint32_t)(2 * w->W), !fused && pb.msorted ? w->d_multi.as<uint32_t>() : nullptr};
  // multi-chunk items: at most M / chm full chunks plus one partial chunk per run of > kChunk records
  const uint64_t gitems =
      fused ? std::min<uint64_t>(pb.max_items, pb.M / multi_chunk(w, pb.P) + pb.M / kChunk + 1) : pb.max_items;
  const unsigned ggrid = (unsigned)std::min<uint64_t>(nblk(gitems * 64), (uint64_t)w->gather_grid);
  const unsigned cgrid = use_combine(w, pb.M) ? combine_grid(pb.max_items) : 0;  // 0: no second level
  const Rows rows = rows_of<T, A>(w);
  hipEvent_t eg = tm.begin(gs);
  if constexpr (kFast<T, A>) {
    if (rows == kBfp) {  // profiled: the kernels' own start / end stamps
      double *part = w->d_partial.as<double>();
      hipEvent_t gb = tm.ext(), ge = tm.ext();
#define SWPS_F(a_, b_, r_)                                                                                         \
  hipExtLaunchKernelGGL(k_gather_b<a_, b_, r_, 8>, dim3(ggrid), dim3(256), 0, gs, gb, cgrid ? (hipEvent_t) nullptr : ge, \
                        0, ga, part)
      SWPS_BFP_DISPATCH(w, SWPS_F);
#undef SWPS_F
      if (cgrid)
        hipExtLaunchKernelGGL(k_combine_b, dim3(cgrid), dim3(256), 0, gs, (hipEvent_t) nullptr, ge, 0, ga, part);
      if (gb) {
        tm.ext_end(KT_GATHER, gb, ge);
        tm.drop(eg);
        eg = nullptr;
      }
    }
    if (rows == kTail) {
#define SWPS_F(n_) k_gather_t<n_, 8><<<ggrid, 256, 0, gs>>>(ga)
      SWPS_TAIL_DISPATCH(D, SWPS_F);
#undef SWPS_F
    }
  }
  if (rows == kChunked) {
    constexpr int UNR = sizeof(A) * V16<T>::E > 16 ? 4 : 8;
#define SWPS_F(n_) k_gather<T, A, n_, UNR><<<ggrid, 256, 0, gs>>>(ga)
    SWPS_NCH_DISPATCH(w->NCH, SWPS_F);
#undef SWPS_F
  }
  if (cgrid && rows != kBfp) {  // second level over the partials: layout-independent
#define SWPS_F(n_) k_combine<T, A, n_><<<cgrid, 256, 0, gs>>>(ga)
    SWPS_NCH_DISPATCH(w->NCH, SWPS_F);
#undef SWPS_F
  }
  SWPS_HIP(hipGetLastError());
  tm.end(KT_GATHER, eg, gs);
  if (pl.split) SWPS_HIP(hipEventRecord(w->ev_gat, gs));
  w->st_pairs += pb.M;
  w->st_sums++;
  w->st_fused += pl.fused_ip;
  w->st_fused_g += pl.fused_g;
  return SWPS_OK;
}

// The sharded learner's mean gradients at world > 1 go out in two passes, each owner's first half
// of keys first: the driver sends those gradients (ev_half) while the second pass runs.  launch(pa)
// issues one pass over pa (PushArgs::gpass: 0 = every key).
template <typename Launch> int push_grads(swps_w2v *w, uint64_t bi, PushArgs<float, float> &pa, Launch launch) {
  const int world = w->world;
  if (!(w->split_grads && world > 1 && world <= kMaxSplitOwners)) {
    launch(pa);
    return SWPS_OK;
  }
  if (!w->ev_half) SWPS_HIP(hipEventCreateWithFlags(&w->ev_half, hipEventDisableTiming));
  pa.nown = (uint32_t)world;
  uint32_t acc = 0;
  for (int r = 0; r < world; r++) {
    const uint64_t c = w->bcounts[bi * world + r];
    pa.obnd[r] = acc;
    pa.ohalf[r] = (uint32_t)(c / 2);
    acc += (uint32_t)c;
  }
  pa.obnd[world] = acc;
  pa.gpass = 1;
  launch(pa);
  SWPS_HIP(hipEventRecord(w->ev_half, w->s));
  pa.gpass = 2;
  launch(pa);
  w->half_ready = true;
  return SWPS_OK;
}

// ---- push: mean + AdaGrad (also clears the local index map) ----
template <typename T, typename A>
int push(swps_w2v *w, const swps_w2v::Prepped &pb, const SumPlan &pl, const int32_t *K, const void *d_vals,
         A *d_grads) {
  hipStream_t s = w->s;
  Timer &tm = w->timer;
  const int D = w->D;
  const uint32_t U = pb.U;
  PushArgs<T, A> pa{K, U, w->d_vid_row.as<uint32_t>(), w->d_seg.as<uint32_t>(), w->d_ioff.as<uint32_t>(),
                    w->d_partial.as<A>(), w->t->rows.as<T>(), w->d_local.as<int32_t>(), D,
                    (double)w->t->cfg.learning_rate, (double)w->t->cfg.fudge, d_grads,
                    d_vals ? nullptr : w->d_cache_h.as<T>(), d_vals ? nullptr : w->d_cache_v.as<T>(), w->cs,
                    w->d_pvals_s.as<uint32_t>(), row_g(w, pb.U) ? nullptr : w->d_pg.as<float>(), w->d_neu1.as<A>(),
                    w->d_neu1e.as<A>(), pb.HOFF, (uint32_t)pb.P, inter_ld<A>(w), w->d_krow.as<uint32_t>(),
                    (uint32_t)(w->N + 1), (uint32_t)(2 * w->W), w->full_lines,
                    use_combine(w, pb.M) ? kGroup : 0xFFFFFFFFu};
  // one wave per key for k_push / k_push_t; the (key, half) kernels (k_push_thp, k_push_b) walk a
  // capped grid: small batches are latency-bound — several items per wave, and the idle CUs run the
  // prep stream (A/B at B = 100 lines: 2048 blocks 0.317 ms/step, 4096 0.323, one item per wave
  // 0.331); large ones want every item in flight
  const unsigned kgrid = nblk((uint64_t)U * 64);
  const unsigned pgrid = (unsigned)std::min<uint64_t>(nblk((uint64_t)U * 128),
                                                      w->push_grid ? w->push_grid : (U < 65536 ? 2048 : ~0u));
  const Rows rows = rows_of<T, A>(w);
  bool done = false;
  hipEvent_t ep = tm.begin(s);
  if constexpr (kFast<T, A>) {
    if (rows == kBfp && !d_grads) {  // in-place AdaGrad; profiled: the kernel's own start / end stamps
      const double *part = w->d_partial.as<double>();
      // D = 257..320, bfp32: 134 -> 128 VGPRs (2 spilled) for 4 waves per SIMD; small batches only
      // (same-box A/B: B = 100 2.87e8 -> 3.06e8 words/s, B = 5000 -0.1 %); SWPS_PUSH_WPE=1 / 4 forces
      const bool wpe4 = w->push_wpe == 4 || (w->push_wpe == 0 && U < 65536);
      const bool d300 = w->bfp_rb == 0 && bfp_shape(D) == 11;
      hipEvent_t xb = tm.ext(), xe = tm.ext();
      if (wpe4 && w->push_unr == 4 && U < 65536 && d300) {
        // D = 257..320, bfp32, small batches: 4 record rows in flight, 114 VGPRs, 4 waves per SIMD
        // without spills (same-box A/B, round 4: B = 100 3.01e8 -> 3.09e8 words/s; 5 / 6 / 8 rows:
        // 3.07 / 3.03 / 3.01e8; 5 waves per SIMD (13 spills) 2.85e8).  Not above 64k keys: B = 5000
        // +0.1 %, the config-4 shape's push 4.78 -> 5.00 ms.  SWPS_PUSH_WPE=1 turns it off too
        hipExtLaunchKernelGGL(k_push_b<1, 1, 0, 4, false, 4>, dim3(pgrid), dim3(256), 0, s, xb, xe, 0, pa, part,
                              (double *)nullptr);
      } else if (wpe4 && d300) {
        hipExtLaunchKernelGGL(k_push_b<1, 1, 0, 8, false, 4>, dim3(pgrid), dim3(256), 0, s, xb, xe, 0, pa, part,
                              (double *)nullptr);
      } else {
#define SWPS_F(a_, b_, r_)                                                                                    \
  hipExtLaunchKernelGGL(k_push_b<a_, b_, r_, 8, false>, dim3(pgrid), dim3(256), 0, s, xb, xe, 0, pa, part, \
                        (double *)nullptr)
        SWPS_BFP_DISPATCH(w, SWPS_F);
#undef SWPS_F
      }
      if (xb) {
        tm.ext_end(KT_PUSH, xb, xe);
        tm.drop(ep);
        ep = nullptr;
      }
      done = true;
    } else if (rows == kBfp) {  // the fp64 push payload
      // (4 record rows in flight here: 94 VGPRs, 5 waves per SIMD, but the sharded world-1 push
      // 2.487 -> 2.506 ms, same-box A/B, round 4: kept at 8)
      const double *part = w->d_partial.as<double>();
      double *g64 = (double *)d_grads;
      auto pass = [&](const PushArgs<float, float> &a) {
#define SWPS_F(a_, b_, r_) k_push_b<a_, b_, r_, 8, true><<<pgrid, 256, 0, s>>>(a, part, g64)
        SWPS_BFP_DISPATCH(w, SWPS_F);
#undef SWPS_F
      };
      SWPS_TRY(push_grads(w, pb.bi, pa, pass));
      done = true;
    } else if (pl.split) {  // every other (key, half) beside the gather, then the multi-chunk halves
      if (pl.fused_g)
        k_push_thp<1, 8, true, 1><<<pgrid, 256, 0, s>>>(pa);
      else
        k_push_thp<1, 8, false, 1><<<pgrid, 256, 0, s>>>(pa);
      SWPS_HIP(hipStreamWaitEvent(s, w->ev_gat, 0));
      if (pl.fused_g)
        k_push_thp<1, 8, true, 2><<<pgrid, 256, 0, s>>>(pa);
      else
        k_push_thp<1, 8, false, 2><<<pgrid, 256, 0, s>>>(pa);
      w->st_split++;
      done = true;
    } else if (pl.fused_g) {
      auto pass = [&](const PushArgs<float, float> &a) { k_push_thp<1, 8, true><<<pgrid, 256, 0, s>>>(a); };
      SWPS_TRY(push_grads(w, pb.bi, pa, pass));
      done = true;
    } else if (pl.fused_ip) {
      k_push_thp<1, 8><<<pgrid, 256, 0, s>>>(pa);
      done = true;
    } else if (rows == kTail && !d_grads && w->push_t) {
#define SWPS_F(n_) k_push_t<n_><<<kgrid, 256, 0, s>>>(pa)
      SWPS_TAIL_DISPATCH(D, SWPS_F);
#undef SWPS_F
      done = true;
    }
  }
  if (!done) {
#define SWPS_F(n_)                                         \
  if (pa.grads)                                            \
    k_push<T, A, n_, true><<<kgrid, 256, 0, s>>>(pa);      \
  else                                                     \
    k_push<T, A, n_, false><<<kgrid, 256, 0, s>>>(pa)
    SWPS_NCH_DISPATCH(w->NCH, SWPS_F);
#undef SWPS_F
  }
  SWPS_HIP(hipGetLastError());
  tm.end(KT_PUSH, ep, s);
  w->st_pushed += U;
  return SWPS_OK;
}

// One minibatch: prep_batch (swps_w2v_prep.hip) made everything that depends only on the corpus,
// the RNG streams and the batch's key set; this is everything that reads parameters.
template <typename T, typename A> int learn_batch(swps_w2v *w, const void *d_vals, A *d_grads) {
  SWPS_TRY(prep_batch(w));
  const auto pb = w->pb;
  hipStream_t s = w->s;
  const uint32_t U = pb.U;
  const int32_t *K = w->d_K.as<int32_t>() + w->batches[pb.bi].kofs;
  if (U && d_vals) SWPS_TRY(install_pulled<T>(w, K, U, d_vals));
  w->st_batches++;
  w->st_kept += pb.P;
  w->st_words += pb.nt;
  w->st_pulled += U;
  if (pb.records) SWPS_TRY((forward<T, A>(w, pb)));
  if (w->fwd_event) SWPS_HIP(hipEventRecord(w->fwd_event, s));
  const SumPlan pl = sum_plan<T, A>(w, pb, d_grads != nullptr);
  hipStream_t gs = s;  // the gather's stream
  if (pl.split) {
    if (!w->s_side) {
      int lo = 0, hi = 0;
      SWPS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
      SWPS_HIP(hipStreamCreateWithPriority(&w->s_side, hipStreamNonBlocking, hi));
      SWPS_HIP(hipEventCreateWithFlags(&w->ev_fwd, hipEventDisableTiming));
      SWPS_HIP(hipEventCreateWithFlags(&w->ev_gat, hipEventDisableTiming));
    }
    SWPS_HIP(hipEventRecord(w->ev_fwd, s));
    SWPS_HIP(hipStreamWaitEvent(w->s_side, w->ev_fwd, 0));
    gs = w->s_side;
  }
  if (pb.sorted) SWPS_TRY((gradient_sums<T, A>(w, pb, pl, gs)));
  if (U > 0) SWPS_TRY((push<T, A>(w, pb, pl, K, d_vals, d_grads)));
  w->pb.valid = false;
  w->cursor++;
  return SWPS_OK;
}

}  // namespace

namespace swps {

int learn_step(swps_w2v *w, const void *d_vals, void *d_grads) {
  if (w->f64) return learn_batch<double, double>(w, d_vals, (double *)d_grads);
  if (inter64(w->cfg)) return learn_batch<float, double>(w, d_vals, (double *)d_grads);
  return learn_batch<float, float>(w, d_vals, (float *)d_grads);  // fast, or BFP (d_grads: the fp64 payload)
}

static void swap_prep_set(swps_w2v *w) {
  for (int k = 0; k < swps_w2v::kPrepBufs; k++) {
    std::swap(w->prep_set[k]->p, w->alt[k].p);
    std::swap(w->prep_set[k]->bytes, w->alt[k].bytes);
  }
}

// Single-GPU minibatch loop with prep(i+1) (epoch plan, local key map,
// records, radix sort, chunk index — parameter-independent, SURVEY.md §3.2's
// draws) on s_prep into the second buffer set while learn(i) (pull, forward,
// gather, push) runs on s.  prep(i+1) waits for learn(i-1), the last user of
// that set (its push also clears that set's local-key map); learn(i+1) waits
// for prep(i+1).  Every kernel sees the same inputs as in the sequential
// loop, so results are bit-identical (tests: SWPS_OVERLAP=0 vs 1).  Nothing
// is left prepared when the call returns.
int train_overlapped(swps_w2v *w, uint64_t count) {
  if (!w->s_prep) {
    int lo = 0, hi = 0;
    SWPS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    // the prep chain is short latency-bound launches: at the highest priority they take CUs as
    // soon as they are issued instead of queueing behind the learn kernels (same-box A/B at
    // B = 100 lines: highest 0.317 ms/step, lowest 0.321); SWPS_PREP_PRIO=0 default, 1 lowest
    const char *pe = getenv("SWPS_PREP_PRIO");
    if (pe && atoi(pe) == 0)
      SWPS_HIP(hipStreamCreateWithFlags(&w->s_prep, hipStreamNonBlocking));
    else if (pe && atoi(pe) == 1)
      SWPS_HIP(hipStreamCreateWithPriority(&w->s_prep, hipStreamNonBlocking, lo));
    else
      SWPS_HIP(hipStreamCreateWithPriority(&w->s_prep, hipStreamNonBlocking, hi));
    SWPS_HIP(hipEventCreateWithFlags(&w->ev_learn, hipEventDisableTiming));
    SWPS_HIP(hipEventCreateWithFlags(&w->ev_prep, hipEventDisableTiming));
  }
  const uint64_t V = w->vocab_keys.size();
  if (!w->alt_local_ready) {
    DevMem &al = w->alt[swps_w2v::kPrepBufs - 1];
    SWPS_TRY(al.ensure(V * 4));
    SWPS_HIP(hipMemsetAsync(al.p, 0xFF, V * 4, w->s));
    w->alt_local_ready = true;
  }
  const hipStream_t s = w->s;
  bool prep_pending = false;  // batch i's prep ran on s_prep (ev_prep)
  if (w->overlap == 2) {
    // prep(i+1) issued after learn(i), waiting for forward(i): it runs beside the gather and the
    // push (latency-bound) instead of beside the forward (bandwidth-bound).  It writes the other
    // buffer set, whose last user learn(i-1) finished before forward(i) did.
    for (uint64_t i = 0; i < count; i++) {
      if (!w->pb.valid) SWPS_TRY(prep_batch(w));  // inline on s (first batch of the call)
      if (prep_pending) SWPS_HIP(hipStreamWaitEvent(s, w->ev_prep, 0));
      w->fwd_event = i + 1 < count ? w->ev_learn : nullptr;
      const int lrc = learn_step(w);  // cursor -> i + 1
      w->fwd_event = nullptr;
      SWPS_TRY(lrc);
      prep_pending = false;
      if (i + 1 < count) {
        SWPS_HIP(hipStreamWaitEvent(w->s_prep, w->ev_learn, 0));
        swap_prep_set(w);  // the other set becomes the current one: prep(i+1) fills it, learn(i+1) reads it
        w->s = w->s_prep;
        w->pb = swps_w2v::Prepped();
        const int rc = prep_batch(w);
        w->s = s;
        SWPS_TRY(rc);
        SWPS_HIP(hipEventRecord(w->ev_prep, w->s_prep));
        prep_pending = true;
      }
    }
    if (prep_pending) SWPS_HIP(hipStreamWaitEvent(s, w->ev_prep, 0));
    return SWPS_OK;
  }
  for (uint64_t i = 0; i < count; i++) {
    if (!w->pb.valid) SWPS_TRY(prep_batch(w));  // inline on s (first batch of the call)
    const swps_w2v::Prepped cur = w->pb;
    swps_w2v::Prepped next;
    if (i + 1 < count) {
      SWPS_HIP(hipEventRecord(w->ev_learn, s));  // learn(i-1) done -> the other set is free
      SWPS_HIP(hipStreamWaitEvent(w->s_prep, w->ev_learn, 0));
      swap_prep_set(w);
      w->s = w->s_prep;
      w->cursor++;
      w->pb = swps_w2v::Prepped();
      const int rc = prep_batch(w);
      next = w->pb;
      w->cursor--;
      w->s = s;
      swap_prep_set(w);
      SWPS_TRY(rc);
    }
    if (prep_pending) SWPS_HIP(hipStreamWaitEvent(s, w->ev_prep, 0));
    if (i + 1 < count) SWPS_HIP(hipEventRecord(w->ev_prep, w->s_prep));
    prep_pending = i + 1 < count;
    w->pb = cur;
    SWPS_TRY(learn_step(w));
    if (prep_pending) {
      swap_prep_set(w);
      w->pb = next;
    }
  }
  return SWPS_OK;
}

// ---- whole-vocab pulls and initialisers (the table's dtype picked here) ----
template <typename T> static int pull_all_t(swps_w2v *w) {
  const uint64_t V = w->vocab_keys.size();
  k_pull<T><<<nblk(V * 64), 256, 0, w->s>>>(nullptr, (uint32_t)V, w->d_vid_row.as<uint32_t>(), w->t->rows.as<T>(),
                                            w->D, w->d_cache_h.as<T>(), w->d_cache_v.as<T>(), w->d_local.as<int32_t>(),
                                            0, w->cs);
  SWPS_HIP(hipGetLastError());
  SWPS_HIP(hipStreamSynchronize(w->s));
  return SWPS_OK;
}
int pull_all(swps_w2v *w) { return w->f64 ? pull_all_t<double>(w) : pull_all_t<float>(w); }

template <typename T> static int rand_init_t(swps_w2v *w) {
  const uint64_t V = w->vocab_keys.size();
  const int D = w->D;
  // o[3..33] after srand(seed) (GlibcRand's seeding, swps_host.cpp)
  const std::vector<uint32_t> base = glibc_base(w->cfg.rand_seed);
  const uint64_t total = V * 2 * (uint64_t)D;
  const uint64_t first = 344 + w->cfg.rand_offset;  // o index of the first output used
  DevMem d_base;
  SWPS_TRY(upload(d_base, base, w->s));
  const uint64_t nthr = (total + kRandRun - 1) / kRandRun;
  if (total) {
    k_rand_init<T><<<nblk(nthr, 64), 64, 0, w->s>>>(d_base.as<uint32_t>(), first, total, D,
                                                    w->d_vid_row.as<uint32_t>(), w->t->rows.as<T>());
    k_zero_sums<T><<<nblk(total), 256, 0, w->s>>>(w->d_vid_row.as<uint32_t>(), V, D, w->t->rows.as<T>());
  }
  SWPS_HIP(hipGetLastError());
  SWPS_HIP(hipStreamSynchronize(w->s));
  return pull_all_t<T>(w);
}
int rand_init_gpu(swps_w2v *w) { return w->f64 ? rand_init_t<double>(w) : rand_init_t<float>(w); }

template <typename T> static int set_hv_t(swps_w2v *w, const double *hv) {
  const uint64_t V = w->vocab_keys.size();
  const int D = w->D;
  std::vector<T> rows(V * 4 * D, (T)0);
  for (uint64_t i = 0; i < V; i++)
    for (int e = 0; e < 2 * D; e++) rows[i * 4 * D + e] = (T)hv[i * 2 * D + e];
  DevMem d;
  SWPS_TRY(upload(d, rows, w->s));
  SWPS_TRY(table_set_rows(w->t, w->d_vid_row.as<uint32_t>(), V, d.p, w->s));
  SWPS_HIP(hipStreamSynchronize(w->s));
  return pull_all_t<T>(w);
}
int set_hv(swps_w2v *w, const double *hv) { return w->f64 ? set_hv_t<double>(w, hv) : set_hv_t<float>(w, hv); }

template <typename T> static int install_init_t(swps_w2v *w, const void *d_vals) {
  const uint64_t V = w->vocab_keys.size();
  k_install<T><<<nblk(V * 64), 256, 0, w->s>>>(w->d_init_order.as<int32_t>(), (uint32_t)V, (const T *)d_vals, w->D,
                                               w->d_cache_h.as<T>(), w->d_cache_v.as<T>(), w->d_local.as<int32_t>(), 0,
                                               w->cs);
  SWPS_HIP(hipGetLastError());
  return SWPS_OK;
}
int install_init(swps_w2v *w, const void *d_vals) {
  return w->f64 ? install_init_t<double>(w, d_vals) : install_init_t<float>(w, d_vals);
}

}  // namespace swps
