// Top-k nearest-neighbour and analogy queries over the HBM-resident shard.
//
// The reference has no query path: SparseTable::output (parameter/sparsetable.h:127-132) dumps
// the rows and its users score them on the host.  Here the shard itself answers: scores are a
// Q.R^T product on the f32-input MFMA followed by a selection, per query, of the best k rows
// under one total order.
//
// Scoring kernel (k_nearest_score), one block = 256 threads = 4 waves:
//   * a block owns one tile of kQT = 32 queries (blockIdx.y) and walks tiles of kRT = 128 rows
//     grid-stride (blockIdx.x); wave w scores rows 32w..32w+31 of the tile against the 32
//     queries with v_mfma_f32_32x32x2_f32: A = rows (lane l: row l & 31, k = l >> 5), B =
//     queries (k = l >> 5, query l & 31), one 32x32 accumulator (16 registers)
//   * the query tile stays in LDS for the whole block: qs[32][Dq + 1], Dq = D rounded up to
//     kKC = 32, zero beyond D and beyond nq
//   * a row tile is staged through LDS in chunks of kKC elements: 16-B loads along each row's
//     D-block (coalesced: 32 / E lanes per row, E = 16 / sizeof(T) elements each; E = 1 when
//     the block is not 16-B aligned, i.e. odd D), converted to fp32, stored as st[128][33]
//     (stride 33: the MFMA operand read, 32 different rows at one k per lane group, hits 32
//     different banks).  Rows past the end, rows the candidate list lacks and the k tail are
//     zeros.  The loads run one chunk ahead in registers, across tile boundaries too, so a
//     chunk's HBM / L2 latency hides behind the previous chunk's MFMAs.
//   * every dot product is the MFMA's k-ordered fp32 fma chain over k = 0..D-1; r.r is summed
//     from the same staged operand values (even k on lanes 0-31, odd k on lanes 32-63, then
//     even + odd): both depend only on the row's values, the query and D
//   * the tile's 32 x 128 scores go through LDS (aliasing the staging buffer) to the wave that
//     owns the query's best-k list (wave w: queries 8w..8w+7); the list is sorted, lane i holds
//     entry i, an insertion is one ballot and one lane shift
//   * the block writes its lists as candidates [nq][gridDim.x][k]
// Merge kernel (k_nearest_merge): one wave per query inserts the candidates of every block (or,
// on a routed table, of every rank) into the same sorted list and writes the final k.
//
// Total order: numbers by higher score, equal scores by smaller key; then NaN scores by smaller
// key; then empty slots (key ~0, score -inf).  Keys are distinct, so the order is strict and the
// best k do not depend on the order rows are met in.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "swps_internal.h"

using namespace swps;

namespace {

constexpr int kQT = 32;    // queries per block
constexpr int kRT = 128;   // rows per tile (32 per wave)
constexpr int kKC = 32;    // staged elements of D per chunk
constexpr int kSS = kKC + 1;  // staging row stride (floats)
constexpr int kCS = kRT + 1;  // score tile row stride (floats)
constexpr int kStageFloats = kRT * kSS > kQT * kCS ? kRT * kSS : kQT * kCS;
constexpr uint64_t kBatch = 65536;                // queries per batch (the host loops)
constexpr int kTargetBlocks = 2048;               // most blocks of a batch with several row blocks
constexpr uint64_t kScratchBound = kBatch * SWPS_NEAREST_MAX_K * 12;  // candidate scratch, 48 MiB
constexpr size_t kLdsMax = 160 * 1024;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// 0: a number, 1: NaN, 2: empty slot
__device__ __forceinline__ int nn_class(float s, uint64_t key) { return key == kEmptyKey ? 2 : (s != s ? 1 : 0); }

// (s, key) strictly before (s2, key2) in the total order
__device__ __forceinline__ bool nn_before(float s, uint64_t key, float s2, uint64_t key2) {
  const int c = nn_class(s, key), c2 = nn_class(s2, key2);
  if (c != c2) return c < c2;
  if (c == 0) {
    if (s > s2) return true;
    if (s < s2) return false;
  }
  return key < key2;
}

// Insert the wave's pending entries (lane-held (cs, ck), `want` set where there is one) into the
// sorted list whose entry i lane i holds (ms, mk), i < k.  Wave-uniform control flow.
__device__ __forceinline__ void nn_insert(float &ms, uint64_t &mk, int k, int lane, bool want, float cs, uint64_t ck) {
  uint64_t m = __ballot(want);
  while (m) {
    const int src = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const float s = __shfl(cs, src);
    const uint64_t key = (uint64_t)__shfl((unsigned long long)ck, src);
    const bool mine = lane < k;
    const int pos = __popcll(__ballot(mine && nn_before(ms, mk, s, key)));  // the list is sorted: a prefix
    const bool dup = __ballot(mine && mk == key) != 0;                       // the same key listed twice
    const float us = __shfl_up(ms, 1);
    const uint64_t uk = (uint64_t)__shfl_up((unsigned long long)mk, 1);
    if (!dup && pos < k && mine) {
      if (lane > pos) {
        ms = us;
        mk = uk;
      } else if (lane == pos) {
        ms = s;
        mk = key;
      }
    }
  }
}

template <typename T, int E> struct alignas(sizeof(T) * E) NVec {
  T v[E];
};

// rows: the table's row store; row block of row r at rows + r * row_elems + off (D elements).
// idx: the candidate subset's row indices (kNoRow: skipped) or nullptr for rows 0..n-1; n: rows
// to walk.  d_excl: [nq][nexcl] or nullptr.  Candidates: ck / cs [nq][gridDim.x][k].
template <typename T, int E>
__global__ __launch_bounds__(256) void k_nearest_score(const T *__restrict__ rows, const uint64_t *__restrict__ row_key,
                                                       uint32_t nrows, int row_elems, int off, int D, int Dq,
                                                       const uint32_t *__restrict__ idx, uint64_t n,
                                                       const float *__restrict__ q, uint64_t nq, int metric, int k,
                                                       const uint64_t *__restrict__ d_excl, int nexcl,
                                                       uint64_t *__restrict__ ck, float *__restrict__ cs) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint64_t *lk = reinterpret_cast<uint64_t *>(lds);             // [kQT][k] list keys
  uint64_t *tk = lk + kQT * k;                                   // [kRT] keys of the tile's rows
  float *ls = reinterpret_cast<float *>(tk + kRT);               // [kQT][k] list scores
  float *n2s = ls + kQT * k;                                     // [kRT] sqrtf(r.r)
  float *st = n2s + kRT;                                         // staging [kRT][kSS] / scores [kQT][kCS]
  float *qs = st + kStageFloats;                                 // [kQT][Dq + 1]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int QS = Dq + 1;
  const uint64_t q0 = (uint64_t)blockIdx.y * kQT;

  for (int i = tid; i < kQT * k; i += 256) {
    lk[i] = kEmptyKey;
    ls[i] = -INFINITY;
  }
  for (int i = tid; i < kQT * QS; i += 256) {
    const int j = i / QS, e = i - j * QS;
    qs[i] = (q0 + j < nq && e < D) ? q[(q0 + j) * D + e] : 0.0f;
  }

  constexpr int VPR = kKC / E;        // vectors per row per chunk
  constexpr int RPP = 256 / VPR;      // rows per staging pass
  constexpr int NP = kRT / RPP;       // passes
  const int sv = tid % VPR, sr = tid / VPR;
  const int nchunks = Dq / kKC;
  const uint64_t ntiles = (n + kRT - 1) / kRT;

  // the row (kNoRow: none) at position i of a tile
  auto row_of = [&](uint64_t tile, int i) -> uint32_t {
    const uint64_t p = tile * kRT + i;
    uint32_t r = kNoRow;
    if (p < n) r = idx ? idx[p] : (uint32_t)p;
    return r < nrows ? r : kNoRow;
  };
  // The staging loads run one chunk ahead of the MFMAs, in registers: the loads of chunk c + 1
  // (of the next tile after a tile's last chunk) are issued before chunk c's MFMA loop and
  // stored to LDS after it.  (lt, lc): the chunk v holds; lr: this thread's rows of tile lt.
  NVec<T, E> v[NP];
  uint32_t lr[NP];
  uint64_t lt = blockIdx.x;
  int lc = 0;
  auto load_rows = [&]() {
#pragma unroll
    for (int p = 0; p < NP; p++) lr[p] = lt < ntiles ? row_of(lt, sr + p * RPP) : kNoRow;
  };
  auto load_chunk = [&]() {
    const int e0 = lc * kKC + sv * E;
#pragma unroll
    for (int p = 0; p < NP; p++) {
      if (lr[p] != kNoRow && e0 < D) {
        v[p] = *reinterpret_cast<const NVec<T, E> *>(rows + (uint64_t)lr[p] * row_elems + off + e0);
      } else {
#pragma unroll
        for (int j = 0; j < E; j++) v[p].v[j] = (T)0;
      }
    }
  };
  load_rows();
  load_chunk();

  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's selection has read st / tk; the first tile: lists and qs are set
    if (tid < kRT) {
      const uint32_t r = row_of(tile, tid);
      tk[tid] = r == kNoRow ? kEmptyKey : row_key[r];
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;
    float n2 = 0.0f;
    for (int c = 0; c < nchunks; c++) {
      if (c) __syncthreads();  // the previous chunk's operand reads are done
#pragma unroll
      for (int p = 0; p < NP; p++) {
#pragma unroll
        for (int j = 0; j < E; j++) st[(sr + p * RPP) * kSS + sv * E + j] = (float)v[p].v[j];
      }
      __syncthreads();
      if (++lc == nchunks) {
        lc = 0;
        lt += gridDim.x;
        load_rows();
      }
      load_chunk();  // past the last tile: zeros, never stored
      const float *ap = st + (w * 32 + (lane & 31)) * kSS + (lane >> 5);
      const float *bp = qs + (lane & 31) * QS + c * kKC + (lane >> 5);
#pragma unroll
      for (int kk = 0; kk < kKC / 2; kk++) {
        const float a = ap[2 * kk], b = bp[2 * kk];
        n2 = fmaf(a, a, n2);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
    }
    {  // r.r of the wave's row (lane & 31): even k + odd k
      const float o = __shfl_xor(n2, 32);
      const float tot = lane < 32 ? n2 + o : o + n2;
      // sqrtf and the division below are correctly rounded in this build (hipcc's default for fp32
      // divide and sqrt; HIP's __fsqrt_rn is the native approximation unless OCML's rounded
      // operations are compiled in): np.float32(dot) / np.sqrt(np.float32(r.r)), bit for bit
      if (lane < 32) n2s[w * 32 + lane] = sqrtf(tot);  // 0 only for r.r == 0
    }
    __syncthreads();  // every wave is done with st as operands; n2s is set
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int i = w * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);  // the tile's row
      float s = acc[reg];
      if (metric == SWPS_METRIC_COS) {
        const float rn = n2s[i];
        s = rn == 0.0f ? 0.0f : s / rn;
      }
      st[(lane & 31) * kCS + i] = s;
    }
    __syncthreads();
    for (int qq = 0; qq < kQT / 4; qq++) {  // the wave's queries
      const int j = w * (kQT / 4) + qq;
      if (q0 + j >= nq) break;  // wave-uniform
      float ms = -INFINITY;
      uint64_t mk = kEmptyKey;
      if (lane < k) {
        ms = ls[j * k + lane];
        mk = lk[j * k + lane];
      }
      bool changed = false;
#pragma unroll
      for (int h = 0; h < kRT / 64; h++) {
        const float s = st[j * kCS + h * 64 + lane];
        const uint64_t key = tk[h * 64 + lane];
        const float wsc = __shfl(ms, k - 1);
        const uint64_t wk = (uint64_t)__shfl((unsigned long long)mk, k - 1);
        bool want = key != kEmptyKey && nn_before(s, key, wsc, wk);
        if (want)
          for (int e = 0; e < nexcl; e++) want = want && d_excl[(q0 + j) * nexcl + e] != key;
        if (__ballot(want)) {
          nn_insert(ms, mk, k, lane, want, s, key);
          changed = true;
        }
      }
      if (changed && lane < k) {
        ls[j * k + lane] = ms;
        lk[j * k + lane] = mk;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kQT * k; i += 256) {
    const int j = i / k, e = i - j * k;
    if (q0 + j < nq) {
      const uint64_t o = ((q0 + j) * gridDim.x + blockIdx.x) * (uint64_t)k + e;
      ck[o] = lk[i];
      cs[o] = ls[i];
    }
  }
}

// One wave per query: candidate (b, i) of query qi is at qi * qstride + b * bstride{k,s} + i.
__global__ __launch_bounds__(256) void k_nearest_merge(const uint64_t *__restrict__ ck, const float *__restrict__ cs,
                                                       uint64_t nq, uint64_t qstride, uint64_t bstride_k,
                                                       uint64_t bstride_s, uint32_t nb, int k,
                                                       uint64_t *__restrict__ keys_out, float *__restrict__ scores_out) {
  const uint64_t qi = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (qi >= nq) return;  // wave-uniform
  float ms = -INFINITY;
  uint64_t mk = kEmptyKey;
  const uint64_t total = (uint64_t)nb * k;
  for (uint64_t f0 = 0; f0 < total; f0 += 64) {
    const uint64_t f = f0 + lane;
    float s = -INFINITY;
    uint64_t key = kEmptyKey;
    if (f < total) {
      const uint64_t b = f / k, i = f - b * k;
      key = ck[qi * qstride + b * bstride_k + i];
      s = cs[qi * qstride + b * bstride_s + i];
    }
    const float wsc = __shfl(ms, k - 1);
    const uint64_t wk = (uint64_t)__shfl((unsigned long long)mk, k - 1);
    const bool want = key != kEmptyKey && nn_before(s, key, wsc, wk);
    if (__ballot(want)) nn_insert(ms, mk, k, lane, want, s, key);
  }
  if (lane < k) {
    keys_out[qi * k + lane] = mk;
    scores_out[qi * k + lane] = ms;
  }
}

// The analogy's operand rows as fp32 copies: out[i][D] = the part's block of row ridx[i]
// (zeros when the shard lacks the key), present[i] = 1 / 0.  One wave per key.
template <typename T>
__global__ void k_gather_f32(const T *__restrict__ rows, const uint32_t *__restrict__ ridx, uint64_t n, uint32_t nrows,
                             int row_elems, int off, int D, float *__restrict__ out, uint32_t *__restrict__ present) {
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint32_t r = ridx[i];
  const bool have = r < nrows;
  for (int e = lane; e < D; e += 64) out[i * D + e] = have ? (float)rows[(uint64_t)r * row_elems + off + e] : 0.0f;
  if (lane == 0) present[i] = have ? 1u : 0u;
}

// q = (b - a) + c in fp32, in that order; the query's exclusion list = (a, b, c)
__global__ void k_analogy_q(const float *__restrict__ abc, const uint64_t *__restrict__ abc_keys, uint64_t nq, int D,
                            float *__restrict__ q, uint64_t *__restrict__ excl) {
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (i >= nq) return;
  const float *a = abc + (i * 3) * D, *b = a + D, *c = b + D;
  for (int e = lane; e < D; e += 64) {
    const float d = b[e] - a[e];
    q[i * D + e] = d + c[e];
  }
  if (lane < 3) excl[i * 3 + lane] = abc_keys[i * 3 + lane];
}

inline unsigned nn_blocks(uint64_t threads) { return (unsigned)((threads + 255) / 256); }

size_t score_lds_bytes(int k, int Dq) {
  return (size_t)kQT * k * 8 + kRT * 8 + ((size_t)kQT * k + kRT + kStageFloats + (size_t)kQT * (Dq + 1)) * 4;
}

template <typename T, int E>
int launch_score(swps_table *t, int off, int Dq, const uint32_t *idx, uint64_t n, const float *d_q, uint64_t nq,
                 int metric, int k, const uint64_t *d_excl, int nexcl, uint32_t nb, uint64_t *ck, float *cs,
                 hipStream_t s) {
  const size_t lds = score_lds_bytes(k, Dq);
  auto kern = k_nearest_score<T, E>;
  SWPS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  const dim3 grid(nb, (unsigned)((nq + kQT - 1) / kQT));
  kern<<<grid, 256, lds, s>>>(t->rows.as<T>(), t->row_key.as<uint64_t>(), t->host_nrows, t->row_elems, off,
                              t->cfg.dim, Dq, idx, n, d_q, nq, metric, k, d_excl, nexcl, ck, cs);
  SWPS_HIP(hipGetLastError());
  return SWPS_OK;
}

int check_args(swps_table *t, int32_t part, int32_t metric, int32_t k, int32_t nexcl) {
  if (!t) return fail(SWPS_E_CFG, "null table");
  if (t->cfg.layout != SWPS_LAYOUT_W2V)
    return fail(SWPS_E_CFG, "nearest-neighbour queries need SWPS_LAYOUT_W2V (an LR table's rows are scalars)");
  if (part < 0 || part > 1) return fail(SWPS_E_CFG, "part " + std::to_string(part) + ": 0 (h) or 1 (v)");
  if (metric != SWPS_METRIC_DOT && metric != SWPS_METRIC_COS)
    return fail(SWPS_E_CFG, "metric " + std::to_string(metric) + ": SWPS_METRIC_DOT or SWPS_METRIC_COS");
  if (k < 1 || k > SWPS_NEAREST_MAX_K)
    return fail(SWPS_E_CFG, "k = " + std::to_string(k) + ": 1 <= k <= " + std::to_string(SWPS_NEAREST_MAX_K));
  if (nexcl < 0 || nexcl > SWPS_NEAREST_MAX_EXCL)
    return fail(SWPS_E_CFG, "nexcl = " + std::to_string(nexcl) + ": at most " + std::to_string(SWPS_NEAREST_MAX_EXCL));
  const int Dq = (t->cfg.dim + kKC - 1) / kKC * kKC;
  if (score_lds_bytes(SWPS_NEAREST_MAX_K, Dq) > kLdsMax)
    return fail(SWPS_E_UNSUPPORTED, "dim " + std::to_string(t->cfg.dim) + ": the query tile does not fit the LDS");
  if (t->comm) {
    if (t->finished) return fail(SWPS_E_STATE, "query after swps_finish");
    SWPS_TRY(comm_status(t->comm));
  }
  return SWPS_OK;
}

// the local shard's best k of every query into keys_out / scores_out [nq][k] (device), stream-ordered
int nearest_local(swps_table *t, int part, int metric, const float *d_q, uint64_t nq, int k, const uint64_t *d_excl,
                  int nexcl, const uint64_t *d_cand, uint64_t ncand, uint64_t *keys_out, float *scores_out) {
  hipStream_t s = t->stream;
  const int D = t->cfg.dim, Dq = (D + kKC - 1) / kKC * kKC, off = part * D;
  const uint32_t *idx = nullptr;
  uint64_t n = t->host_nrows;
  if (d_cand) {
    n = ncand;
    SWPS_TRY(t->nn_idx.ensure(std::max<uint64_t>(n, 1) * 4));
    SWPS_TRY(table_probe(t, d_cand, n, t->nn_idx.as<uint32_t>(), s));
    idx = t->nn_idx.as<uint32_t>();
  }
  const uint64_t ntiles = (n + kRT - 1) / kRT;
  const bool vec = ((size_t)D * t->esize) % 16 == 0;
  // Query batches of at most kBatch queries, and at most kQT * kTargetBlocks / nqb row blocks:
  // nqb * nb <= kBatch candidate lists of k <= 64 entries of 12 B, i.e. the scratch stays under
  // kScratchBound = 48 MiB whatever nq is.  SWPS_NEAREST_BATCH: a smaller batch (tests of the
  // batch loop).
  uint64_t nqb = std::min<uint64_t>(nq, kBatch);
  if (const char *e = getenv("SWPS_NEAREST_BATCH"))
    if (atoll(e) > 0) nqb = std::min<uint64_t>(nqb, (uint64_t)atoll(e));
  const uint64_t nqt = (nqb + kQT - 1) / kQT;
  // Row blocks per query tile: every block starts its lists empty and the merge reads nb lists per
  // query, so the fewest that still fill the chip: the first nb whose nqt * nb blocks run in
  // whole rounds of the resident set (LDS-bound blocks per CU x CUs) to 90 %, else the best seen.
  int cus = 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->cfg.device) != hipSuccess || cus < 1) {
    (void)hipGetLastError();
    cus = 256;
  }
  const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(8, kLdsMax / score_lds_bytes(k, Dq)));
  const uint64_t resident = per_cu * (uint64_t)cus;
  const uint64_t nb_max = std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)kQT * kTargetBlocks / nqb));
  uint32_t nb = 1;
  double best = 0.0;
  for (uint64_t c = 1; c <= nb_max; c++) {
    const uint64_t blocks = nqt * c, rounds = (blocks + resident - 1) / resident;
    const double eff = (double)blocks / (double)(rounds * resident);
    if (eff > best) {
      best = eff;
      nb = (uint32_t)c;
    }
    if (eff >= 0.9) break;
  }
  const uint64_t slots = nqb * nb * (uint64_t)k;
  if (slots * 12 > kScratchBound) return fail(SWPS_E_STATE, "nearest: candidate scratch over its bound");
  SWPS_TRY(t->nn_cand.ensure(slots * 12));
  uint64_t *ck = t->nn_cand.as<uint64_t>();
  float *cs = reinterpret_cast<float *>(ck + slots);
  for (uint64_t b0 = 0; b0 < nq; b0 += nqb) {
    const uint64_t m = std::min(nqb, nq - b0);
    const float *qb = d_q + b0 * D;
    const uint64_t *eb = d_excl ? d_excl + b0 * nexcl : nullptr;
    const int ne = d_excl ? nexcl : 0;
    if (t->cfg.dtype == SWPS_F64) {
      if (vec)
        SWPS_TRY((launch_score<double, 2>(t, off, Dq, idx, n, qb, m, metric, k, eb, ne, nb, ck, cs, s)));
      else
        SWPS_TRY((launch_score<double, 1>(t, off, Dq, idx, n, qb, m, metric, k, eb, ne, nb, ck, cs, s)));
    } else {
      if (vec)
        SWPS_TRY((launch_score<float, 4>(t, off, Dq, idx, n, qb, m, metric, k, eb, ne, nb, ck, cs, s)));
      else
        SWPS_TRY((launch_score<float, 1>(t, off, Dq, idx, n, qb, m, metric, k, eb, ne, nb, ck, cs, s)));
    }
    k_nearest_merge<<<nn_blocks(m * 64), 256, 0, s>>>(ck, cs, m, (uint64_t)nb * k, (uint64_t)k, (uint64_t)k, nb, k,
                                                      keys_out + b0 * k, scores_out + b0 * k);
    SWPS_HIP(hipGetLastError());
  }
  return SWPS_OK;
}

// swps_nearest after the argument checks; the table's row count is current
int nearest_run(swps_table *t, int part, int metric, const float *d_q, uint64_t nq, int k, const uint64_t *d_excl,
                int nexcl, const uint64_t *d_cand, uint64_t ncand, uint64_t *d_keys_out, float *d_scores_out) {
  hipStream_t s = t->stream;
  const int world = t->comm ? comm_world(t->comm) : 1;
  if (world == 1) {
    SWPS_TRY(nearest_local(t, part, metric, d_q, nq, k, d_excl, nexcl, d_cand, ncand, d_keys_out, d_scores_out));
    SWPS_HIP(hipStreamSynchronize(s));
    return SWPS_OK;
  }
  // every rank's [nq][k] answer, all-gathered and merged alike on every rank.  One rank's block:
  // keys u64[nq * k] | scores f32[nq * k] (+ 4 B when odd)
  const uint64_t nk = nq * (uint64_t)k, blk = nk * 8 + (nk * 4 + 7) / 8 * 8;
  SWPS_TRY(t->nn_part.ensure(blk * (world + 1)));
  char *mine = t->nn_part.as<char>(), *all = mine + blk;
  SWPS_TRY(nearest_local(t, part, metric, d_q, nq, k, d_excl, nexcl, d_cand, ncand, (uint64_t *)mine,
                         (float *)(mine + nk * 8)));
  std::vector<char> hin(blk), hall(blk * world);
  SWPS_HIP(hipMemcpyAsync(hin.data(), mine, blk, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  SWPS_TRY(comm_allgather(t->comm, hin.data(), hall.data(), blk, s));
  SWPS_HIP(hipMemcpyAsync(all, hall.data(), blk * world, hipMemcpyHostToDevice, s));
  k_nearest_merge<<<nn_blocks(nq * 64), 256, 0, s>>>((const uint64_t *)all, (const float *)(all + nk * 8), nq,
                                                     (uint64_t)k, blk / 8, blk / 4, (uint32_t)world, k, d_keys_out,
                                                     d_scores_out);
  SWPS_HIP(hipGetLastError());
  SWPS_HIP(hipStreamSynchronize(s));
  return SWPS_OK;
}

}  // namespace

extern "C" {

int swps_nearest(swps_table *t, int32_t part, int32_t metric, const float *d_q, uint64_t nq, int32_t k,
                 const uint64_t *d_excl, int32_t nexcl, const uint64_t *d_cand, uint64_t ncand, uint64_t *d_keys_out,
                 float *d_scores_out) {
  SWPS_TRY(check_args(t, part, metric, k, nexcl));
  if (nq == 0) return SWPS_OK;
  if (!d_q || !d_keys_out || !d_scores_out) return fail(SWPS_E_CFG, "null argument");
  if (nexcl > 0 && !d_excl) return fail(SWPS_E_CFG, "nexcl > 0 without an exclusion list");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  SWPS_TRY(table_check_error(t, t->stream));  // refreshes the row count
  return nearest_run(t, part, metric, d_q, nq, k, d_excl, nexcl, d_cand, ncand, d_keys_out, d_scores_out);
}

int swps_analogy(swps_table *t, int32_t part, int32_t metric, const uint64_t *d_abc, uint64_t nq, int32_t k,
                 const uint64_t *d_cand, uint64_t ncand, uint64_t *d_keys_out, float *d_scores_out) {
  SWPS_TRY(check_args(t, part, metric, k, 3));
  if (nq == 0) return SWPS_OK;
  if (!d_abc || !d_keys_out || !d_scores_out) return fail(SWPS_E_CFG, "null argument");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  SWPS_TRY(table_check_error(t, t->stream));
  hipStream_t s = t->stream;
  const int D = t->cfg.dim;
  const uint64_t n3 = nq * 3, rowb = n3 * (uint64_t)D * 4;
  // nn_abc: fp32 rows [nq * 3][D] | present u32[nq * 3] | row indices u32[nq * 3]
  SWPS_TRY(t->nn_abc.ensure(rowb + n3 * 8));
  float *abc = t->nn_abc.as<float>();
  uint32_t *present = reinterpret_cast<uint32_t *>(t->nn_abc.as<char>() + rowb), *ridx = present + n3;
  SWPS_TRY(table_probe(t, d_abc, n3, ridx, s));
  if (t->cfg.dtype == SWPS_F64)
    k_gather_f32<double><<<nn_blocks(n3 * 64), 256, 0, s>>>(t->rows.as<double>(), ridx, n3, t->host_nrows,
                                                            t->row_elems, part * D, D, abc, present);
  else
    k_gather_f32<float><<<nn_blocks(n3 * 64), 256, 0, s>>>(t->rows.as<float>(), ridx, n3, t->host_nrows, t->row_elems,
                                                           part * D, D, abc, present);
  SWPS_HIP(hipGetLastError());
  const int world = t->comm ? comm_world(t->comm) : 1;
  std::vector<uint32_t> hp(n3);
  SWPS_HIP(hipMemcpyAsync(hp.data(), present, n3 * 4, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  if (world == 1) {
    for (uint64_t i = 0; i < n3; i++)
      if (!hp[i])
        return fail(SWPS_E_BADKEY, "analogy question " + std::to_string(i / 3) + ": the table lacks operand " +
                                       std::to_string(i % 3) + " (a, b, c = 0, 1, 2)");
  } else {
    // every rank's presence flags, then the rows: each operand is a copy of the first holder's
    // values, its owner's (never a sum), the same on every rank
    const int me = comm_rank(t->comm);
    std::vector<uint32_t> pall(n3 * world);
    SWPS_TRY(comm_allgather(t->comm, hp.data(), pall.data(), n3 * 4, s));
    std::vector<int> src(n3, -1);
    for (uint64_t i = 0; i < n3; i++)
      for (int r = 0; r < world && src[i] < 0; r++)
        if (pall[(uint64_t)r * n3 + i]) src[i] = r;
    std::vector<float> hrows(n3 * (uint64_t)D), rall(n3 * (uint64_t)D * world);
    SWPS_HIP(hipMemcpyAsync(hrows.data(), abc, rowb, hipMemcpyDeviceToHost, s));
    SWPS_HIP(hipStreamSynchronize(s));
    SWPS_TRY(comm_allgather(t->comm, hrows.data(), rall.data(), rowb, s));
    for (uint64_t i = 0; i < n3; i++)  // after the exchange: every rank fails alike
      if (src[i] < 0)
        return fail(SWPS_E_BADKEY, "analogy question " + std::to_string(i / 3) + ": no shard holds operand " +
                                       std::to_string(i % 3) + " (a, b, c = 0, 1, 2)");
    for (uint64_t i = 0; i < n3; i++)
      if (src[i] != me)
        memcpy(hrows.data() + i * D, rall.data() + ((uint64_t)src[i] * n3 + i) * D, (size_t)D * 4);
    SWPS_HIP(hipMemcpyAsync(abc, hrows.data(), rowb, hipMemcpyHostToDevice, s));
    SWPS_HIP(hipStreamSynchronize(s));  // hrows leaves scope
  }
  SWPS_TRY(t->nn_q.ensure(nq * (uint64_t)D * 4));
  SWPS_TRY(t->nn_excl.ensure(n3 * 8));
  k_analogy_q<<<nn_blocks(nq * 64), 256, 0, s>>>(abc, d_abc, nq, D, t->nn_q.as<float>(), t->nn_excl.as<uint64_t>());
  SWPS_HIP(hipGetLastError());
  return nearest_run(t, part, metric, t->nn_q.as<float>(), nq, k, t->nn_excl.as<uint64_t>(), 3, d_cand, ncand,
                     d_keys_out, d_scores_out);
}

// Host-pointer forms: staged through HBM by the library.
int swps_nearest_h(swps_table *t, int32_t part, int32_t metric, const float *q, uint64_t nq, int32_t k,
                   const uint64_t *excl, int32_t nexcl, const uint64_t *cand, uint64_t ncand, uint64_t *keys_out,
                   float *scores_out) {
  SWPS_TRY(check_args(t, part, metric, k, nexcl));
  if (nq == 0) return SWPS_OK;
  if (!q || !keys_out || !scores_out) return fail(SWPS_E_CFG, "null argument");
  if (nexcl > 0 && !excl) return fail(SWPS_E_CFG, "nexcl > 0 without an exclusion list");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  hipStream_t s = t->stream;
  const uint64_t D = t->cfg.dim, nk = nq * (uint64_t)k;
  DevMem dq, de, dc, dk, ds;
  SWPS_TRY(dq.ensure(nq * D * 4));
  SWPS_TRY(dk.ensure(nk * 8));
  SWPS_TRY(ds.ensure(nk * 4));
  SWPS_HIP(hipMemcpyAsync(dq.p, q, nq * D * 4, hipMemcpyHostToDevice, s));
  if (nexcl > 0) {
    SWPS_TRY(de.ensure(nq * nexcl * 8));
    SWPS_HIP(hipMemcpyAsync(de.p, excl, nq * nexcl * 8, hipMemcpyHostToDevice, s));
  }
  if (cand) {
    SWPS_TRY(dc.ensure(std::max<uint64_t>(ncand, 1) * 8));
    if (ncand) SWPS_HIP(hipMemcpyAsync(dc.p, cand, ncand * 8, hipMemcpyHostToDevice, s));
  }
  SWPS_HIP(hipStreamSynchronize(s));
  SWPS_TRY(swps_nearest(t, part, metric, dq.as<float>(), nq, k, nexcl > 0 ? de.as<uint64_t>() : nullptr, nexcl,
                        cand ? dc.as<uint64_t>() : nullptr, ncand, dk.as<uint64_t>(), ds.as<float>()));  // syncs
  SWPS_HIP(hipMemcpy(keys_out, dk.p, nk * 8, hipMemcpyDeviceToHost));
  SWPS_HIP(hipMemcpy(scores_out, ds.p, nk * 4, hipMemcpyDeviceToHost));
  return SWPS_OK;
}

int swps_analogy_h(swps_table *t, int32_t part, int32_t metric, const uint64_t *abc, uint64_t nq, int32_t k,
                   const uint64_t *cand, uint64_t ncand, uint64_t *keys_out, float *scores_out) {
  SWPS_TRY(check_args(t, part, metric, k, 3));
  if (nq == 0) return SWPS_OK;
  if (!abc || !keys_out || !scores_out) return fail(SWPS_E_CFG, "null argument");
  SWPS_HIP(hipSetDevice(t->cfg.device));
  hipStream_t s = t->stream;
  const uint64_t nk = nq * (uint64_t)k;
  DevMem da, dc, dk, ds;
  SWPS_TRY(da.ensure(nq * 3 * 8));
  SWPS_TRY(dk.ensure(nk * 8));
  SWPS_TRY(ds.ensure(nk * 4));
  SWPS_HIP(hipMemcpyAsync(da.p, abc, nq * 3 * 8, hipMemcpyHostToDevice, s));
  if (cand) {
    SWPS_TRY(dc.ensure(std::max<uint64_t>(ncand, 1) * 8));
    if (ncand) SWPS_HIP(hipMemcpyAsync(dc.p, cand, ncand * 8, hipMemcpyHostToDevice, s));
  }
  SWPS_HIP(hipStreamSynchronize(s));
  SWPS_TRY(swps_analogy(t, part, metric, da.as<uint64_t>(), nq, k, cand ? dc.as<uint64_t>() : nullptr, ncand,
                        dk.as<uint64_t>(), ds.as<float>()));  // syncs
  SWPS_HIP(hipMemcpy(keys_out, dk.p, nk * 8, hipMemcpyDeviceToHost));
  SWPS_HIP(hipMemcpy(scores_out, ds.p, nk * 4, hipMemcpyDeviceToHost));
  return SWPS_OK;
}

}  // extern "C"
