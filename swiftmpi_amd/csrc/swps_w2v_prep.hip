// word2vec minibatch prep (swps_w2v_ctx.h): everything about a minibatch that
// depends only on the corpus, the two RNG streams and the batch's key set —
// the epoch plan (subsample flags, kept-position scan, main-LCG draw
// offsets), the local key map, the position and gradient records
// (learn_instance's draws) and the inverted index over the records (stable
// radix sort by local key, segment bounds, chunk descriptors).  No kernel
// here reads a parameter.
#include <algorithm>

#include "swps_scan.h"
#include "swps_sort.h"
#include "swps_w2v_ctx.h"

using namespace swps;

namespace {

__device__ __forceinline__ int32_t unigram_lookup(const uint64_t *__restrict__ starts, const int32_t *__restrict__ idx,
                                                  int shift, uint32_t V, uint64_t slot) {
  const uint64_t b = slot >> shift;
  uint32_t lo = (uint32_t)idx[b], hi = min((uint32_t)idx[b + 1] + 1u, V);
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (starts[mid] <= slot)
      lo = mid;
    else
      hi = mid;
  }
  return (int32_t)lo;
}

// float-LCG keep flags for the epoch (to_sample, word2vec_global.h:725-731):
// token t consumes the (t+1)-th draw after the epoch's start state.  k_keep_mb:
// each thread jumps once to the start of its run of kKeepRun tokens, then steps.
constexpr int kKeepRun = 16;
// float-LCG (subsampling) jumps by 2^i draws, x -> c_f2A[i] x + c_f2C[i] (set at create)
__constant__ uint64_t c_f2A[64];
__constant__ uint64_t c_f2C[64];
__device__ __forceinline__ uint64_t flcg_jump_p2(uint64_t x, uint64_t k) {
  for (int i = 0; k; i++, k >>= 1)
    if (k & 1) x = c_f2A[i] * x + c_f2C[i];
  return x;
}
// A wave takes 64 * kKeepIt consecutive tokens, lane l the tokens base + l + 64 j (coalesced loads and
// stores); the lane's float-LCG state jumps once to its first token, then 64 draws per step.
constexpr int kKeepIt = 16;
__global__ __launch_bounds__(256) void k_keep(const int32_t *__restrict__ tok, uint64_t nt,
                                              const float *__restrict__ ran, uint64_t fstate, int sample_on,
                                              int32_t *__restrict__ kflag) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t lane = g & 63, base = (g >> 6) * (64ULL * kKeepIt);
  if (base > nt) return;
  uint64_t y = sample_on ? flcg_jump_p2(fstate, base + lane) : 0;  // the state after token base+lane-1's draw
  const uint64_t A64 = c_f2A[6], C64 = c_f2C[6];
#pragma unroll 4
  for (int j = 0; j < kKeepIt; j++) {
    const uint64_t i = base + lane + 64ULL * (uint64_t)j;
    if (i > nt) break;
    int32_t keep = 0;  // kflag[nt] = 0: the scan's end
    if (i < nt) {
      keep = 1;
      if (sample_on) keep = flcg_value(y * kFlcgA + kLcgC) > ran[tok[i]];  // word2vec_global.h:725-731
    }
    kflag[i] = keep;
    y = A64 * y + C64;
  }
}

// word2vec.h:621-629 to_sample with per-minibatch counts: freq =
// count_in_batch / (int)_num_words, where _num_words (never reset) is
// tw[b] for batch b of this epoch; btok[b] = first token of batch b.
__global__ void k_keep_mb(const int32_t *__restrict__ bcnt, uint64_t nt, const int64_t *__restrict__ btok,
                          uint32_t nb, const int32_t *__restrict__ tw, float sample, uint64_t fstate, int sample_on,
                          int32_t *__restrict__ kflag) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i0 = r * kKeepRun;
  if (i0 > nt) return;
  uint64_t y = sample_on ? lcg_jump(fstate, i0, kFlcgA, kLcgC) : 0;
  uint32_t b = 0, hi = nb;  // batch of token i0
  while (hi - b > 1) {
    const uint32_t mid = (b + hi) >> 1;
    if ((uint64_t)btok[mid] <= i0)
      b = mid;
    else
      hi = mid;
  }
  for (uint64_t i = i0; i < i0 + kKeepRun && i <= nt; i++) {
    if (i == nt) {
      kflag[i] = 0;
      break;
    }
    int32_t keep = 1;
    if (sample_on) {
      while (b + 1 < nb && (uint64_t)btok[b + 1] <= i) b++;
      y = y * kFlcgA + kLcgC;
      const float freq = (float)bcnt[i] / (float)tw[b];
      const float ran = (float)(1 - sqrt((double)(sample / freq)));
      keep = flcg_value(y) > ran;
    }
    kflag[i] = keep;
  }
}

// main-LCG draws per line: 1 (learn_instance's initial b) + kept*(1+negative)
__global__ void k_line_draws(const int64_t *__restrict__ line_off, uint64_t nl, const int32_t *__restrict__ kscan,
                             int N, uint64_t *__restrict__ ldraw) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > nl) return;
  if (j == nl) {
    ldraw[j] = 0;
    return;
  }
  uint64_t kept = (uint64_t)(kscan[line_off[j + 1]] - kscan[line_off[j]]);
  ldraw[j] = 1 + kept * (uint64_t)(N + 1);
}

// kept-count prefix at each batch boundary (token offsets given)
__global__ void k_bounds(const int32_t *__restrict__ kscan, const int64_t *__restrict__ btok, uint64_t n,
                         int32_t *__restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = kscan[btok[i]];
}

// x mod d for a fixed divisor d < 2^63 with the precomputed m = floor((2^64-1)/d):
// q = mulhi(x, m) underestimates x/d by at most 2, so two corrections are exact.
__device__ __forceinline__ uint64_t fast_mod(uint64_t x, uint64_t d, uint64_t m) {
  const uint64_t q = __umul64hi(x, m);
  uint64_t r = x - q * d;
  if (r >= d) r -= d;
  if (r >= d) r -= d;
  return r;
}

struct RecArgs {
  const int32_t *tok, *tok_line;
  const int64_t *line_off;
  const int32_t *pos_tok;
  uint32_t P;
  const int32_t *kscan;   // epoch-wide
  const uint64_t *ldoff;  // epoch-wide
  uint64_t lstate;        // main LCG state at the epoch start
  int W, N;
  uint64_t mW;  // floor((2^64-1)/W)
  const int32_t *unigram;
  uint64_t uni_size, mT;
  const uint64_t *bstarts;  // minibatch-vocab mode: run starts of the batch's table [bU+1] (else nullptr)
  const int32_t *buk;       // the batch's vids in std::map key order (the table's word order)
  uint32_t bU;
  const uint64_t *ustarts;  // run-length unigram table + its coarse index (k_build_uidx), or nullptr: read unigram[]
  const int32_t *uidx;
  int ushift;
  uint32_t uV;
  const uint2 *alias;       // SWPS_SAMPLER_ALIAS: {prob bits, alias} per word of the (batch) vocab, else nullptr
  uint32_t alias_n;
  const int32_t *local;
  uint32_t U;
  const uint32_t *vid_row;  // direct table reads (single GPU): slots of pulled keys hold kTabRow | table row
  int32_t *rec;     // [P][RS]: word, ctx x 2W (-1 = none), target x (N+1) (-1 = skipped); each a cache vid
                    // or kTabRow | table row (slot_row)
  uint32_t *pkeys, *pvals;  // position-major: h record (p,d) at p*(N+1)+d; v record (p,j) at (N+1)*P + p*2W+j
  int32_t *trace;
  unsigned long long *rows_touched;
  const int2 *tloc;  // per batch token (from t0): {local key, position-record source} (k_tok_local), or nullptr
  uint64_t t0;
};

// Per token of the batch: its local key and the source its position-record slot holds (kTabRow |
// shard row for a pulled key on a single GPU, else its vid) — looked up once per token, so
// k_records_t reads a position's contexts and word as contiguous entries instead of two random
// lookups each
__global__ void k_tok_local(const int32_t *__restrict__ tok, uint64_t nt, const int32_t *__restrict__ local,
                            const uint32_t *__restrict__ vid_row, int2 *__restrict__ tloc) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  const int32_t v = tok[i], u = local[v];
  tloc[i] = make_int2(u, (u >= 0 && vid_row) ? (kTabRow | (int32_t)vid_row[v]) : v);
}

// One thread per kept position: replays learn_instance's LCG draws
// (word2vec_global.h:669,686-691) from the jumped state — b, the negatives
// from the unigram table, the context slots a = b..2W-b (a != W) inside the
// line — and writes the position record plus the (local key, record index)
// gradient records (key U = not in the batch's pulled key set: dropped, as the
// reference's pull reset drops them).
// The [RS]-int position records are built in LDS (thread stride RS) and
// stored by the whole block as one contiguous run: per-thread stores at a
// 4*RS-byte stride wrote partial cache lines (PMC: 1.25 GB written per batch
// for 0.28 GB of records and gradient records).
__global__ __launch_bounds__(256) void k_records(RecArgs a) {
  extern __shared__ int32_t srec[];
  const uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x;
  const uint64_t p = p0 + threadIdx.x;
  const int RS = 2 * a.W + a.N + 2;
  int nctx = 0, ntgt = 0;
  if (p < a.P) {
    const uint64_t P = a.P;
    const int W = a.W, N = a.N;
    const uint64_t HOFF = P * (uint64_t)(N + 1);
    const uint64_t t = (uint64_t)a.pos_tok[p];
    const int32_t l = a.tok_line[t];
    const int64_t ls = a.line_off[l];
    const int n = (int)(a.line_off[l + 1] - ls), pos = (int)((int64_t)t - ls);
    const int32_t word = a.tok[t];
    const uint64_t rank = (uint64_t)(a.kscan[t] - a.kscan[ls]);
    uint64_t x = lcg_jump(a.lstate, a.ldoff[l] + 1 + rank * (uint64_t)(N + 1), kLcgA, kLcgC);
    x = x * kLcgA + kLcgC;
    const int b = (int)fast_mod(x, (uint64_t)W, a.mW);
    int32_t *r = srec + threadIdx.x * RS;
    r[0] = word;
    for (int j = 0; j < 2 * W; j++) {
      int32_t cv = -1;
      if (j < 2 * (W - b)) {
        int aa = b + j;
        if (aa >= W) aa++;
        const int c = pos - W + aa;
        if (c >= 0 && c < n) cv = a.tok[ls + c];
      }
      uint32_t key = a.U;
      int32_t src = cv;
      if (cv >= 0) {
        nctx++;
        const int32_t u = a.local[cv];
        if (u >= 0) {
          key = (uint32_t)u;
          if (a.vid_row) src = kTabRow | (int32_t)a.vid_row[cv];
        }
      }
      r[1 + j] = src;
      const uint64_t k = HOFF + p * (uint64_t)(2 * W) + j;
      a.pkeys[k] = key;
      if (a.pvals) a.pvals[k] = (uint32_t)k;
    }
    for (int d = 0; d <= N; d++) {
      int32_t tv = word;
      if (d > 0) {
        x = x * kLcgA + kLcgC;
        const uint64_t slot = fast_mod(x >> 16, a.uni_size, a.mT);
        if (a.alias) {  // Walker/Vose alias over unigram^0.75: bucket from the LCG's high word; the
                        // coin from a mix of the whole state (the LCG's low bits have short periods)
          const uint32_t bkt = (uint32_t)(((x >> 32) * (uint64_t)a.alias_n) >> 32);
          const uint2 e = a.alias[bkt];
          const float coin = (float)(uint32_t)(splitmix64(x) >> 40) * (1.0f / 16777216.0f);
          const int32_t w = coin < __uint_as_float(e.x) ? (int32_t)bkt : (int32_t)e.y;
          tv = a.bstarts ? a.buk[w] : w;
        } else if (a.bstarts) {  // word2vec.h:398-425 table over the minibatch vocab, run-length form
          uint32_t lo = 0, hi = a.bU;  // largest u with bstarts[u] <= slot
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.bstarts[mid] <= slot)
              lo = mid;
            else
              hi = mid;
          }
          tv = a.buk[lo];
        } else if (a.uidx) {
          tv = unigram_lookup(a.ustarts, a.uidx, a.ushift, a.uV, slot);
        } else {
          tv = a.unigram[slot];
        }
        if (a.trace) a.trace[p * N + d - 1] = tv;
        if (tv == word) tv = -1;
      }
      uint32_t key = a.U;
      int32_t src = tv;
      if (tv >= 0) {
        ntgt++;
        const int32_t u = a.local[tv];
        if (u >= 0) {
          key = (uint32_t)u;
          if (a.vid_row) src = kTabRow | (int32_t)a.vid_row[tv];
        }
      }
      r[1 + 2 * W + d] = src;
      const uint64_t k = p * (uint64_t)(N + 1) + d;
      a.pkeys[k] = key;
      if (a.pvals) a.pvals[k] = (uint32_t)k;
    }
  }
  __syncthreads();
  {
    const uint32_t n = (uint32_t)min<uint64_t>(blockDim.x, a.P - min(p0, a.P)) * (uint32_t)RS;
    int32_t *dst = a.rec + p0 * RS;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = srec[i];
  }
  // rows the forward will read (roofline accounting), one atomic per wave
  unsigned long long c = (unsigned long long)nctx, g = (unsigned long long)ntgt;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    c += __shfl_xor(c, off, 64);
    g += __shfl_xor(g, off, 64);
  }
  if (a.rows_touched && (threadIdx.x & 63) == 0 && (c | g)) {  // profiled passes only
    atomicAdd(&a.rows_touched[0], c);
    atomicAdd(&a.rows_touched[1], g);
  }
}

// Main-LCG jump by k draws with per-bit constants (x -> A_i x + C_i jumps
// 2^i draws; powers of one affine map commute): the per-thread doubling loop
// of lcg_jump squared the same (A, C) pairs in every thread.
__constant__ uint64_t c_p2A[64];
__constant__ uint64_t c_p2C[64];
__device__ __forceinline__ uint64_t lcg_jump_p2(uint64_t x, uint64_t k) {
  for (int i = 0; k; i++, k >>= 1)
    if (k & 1) x = c_p2A[i] * x + c_p2C[i];
  return x;
}

// k_records for the common case — compile-time window W and negatives N, the
// reference's table sampler through the coarse index, one global vocab —
// restructured so each thread's independent loads are in flight together
// (all 2W context words, then all their local / row lookups; the N draws
// first, then the N unigram searches advanced in lockstep) instead of one
// dependent chain per slot.  Identical outputs to k_records.
template <int W, int N>
__global__ __launch_bounds__(256) void k_records_t(RecArgs a) {
  extern __shared__ int32_t srec[];
  constexpr int RS = 2 * W + N + 2;
  const uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x;
  const uint64_t p = p0 + threadIdx.x;
  int nctx = 0, ntgt = 0;
  if (p < a.P) {
    const uint64_t P = a.P;
    const uint64_t HOFF = P * (uint64_t)(N + 1);
    const uint64_t t = (uint64_t)a.pos_tok[p];
    const int32_t l = a.tok_line[t];
    const int64_t ls = a.line_off[l];
    const int n = (int)(a.line_off[l + 1] - ls), pos = (int)((int64_t)t - ls);
    const int32_t word = a.tok[t];
    const uint64_t rank = (uint64_t)(a.kscan[t] - a.kscan[ls]);
    uint64_t x = lcg_jump_p2(a.lstate, a.ldoff[l] + 1 + rank * (uint64_t)(N + 1));
    x = x * kLcgA + kLcgC;
    const int b = (int)fast_mod(x, (uint64_t)W, a.mW);
    int32_t *r = srec + threadIdx.x * RS;
    r[0] = word;
    // ---- contexts: a = b .. 2W-b (a != W) inside the line ----
    int32_t cv[2 * W], cu[2 * W], cs[2 * W];
    if (a.tloc) {  // the per-token lookups (k_tok_local): contiguous in the line
#pragma unroll
      for (int j = 0; j < 2 * W; j++) {
        cv[j] = -1;
        cu[j] = -1;
        cs[j] = -1;
        if (j < 2 * (W - b)) {
          int aa = b + j;
          if (aa >= W) aa++;
          const int c = pos - W + aa;
          if (c >= 0 && c < n) {
            const int2 x = a.tloc[(uint64_t)(ls + c) - a.t0];
            cv[j] = 0;  // present (its vid is not needed: cs holds the slot's source)
            cu[j] = x.x;
            cs[j] = x.y;
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2 * W; j++) {
        cv[j] = -1;
        if (j < 2 * (W - b)) {
          int aa = b + j;
          if (aa >= W) aa++;
          const int c = pos - W + aa;
          if (c >= 0 && c < n) cv[j] = a.tok[ls + c];
        }
      }
#pragma unroll
      for (int j = 0; j < 2 * W; j++) cu[j] = cv[j] >= 0 ? a.local[cv[j]] : -1;
#pragma unroll
      for (int j = 0; j < 2 * W; j++)
        cs[j] = (cu[j] >= 0 && a.vid_row) ? (kTabRow | (int32_t)a.vid_row[cv[j]]) : cv[j];
    }
    // ---- targets: the word, then N draws from the unigram table ----
    uint64_t slot[N + 1];
    uint32_t lo[N + 1], hi[N + 1];
#pragma unroll
    for (int d = 1; d <= N; d++) {
      x = x * kLcgA + kLcgC;
      slot[d] = fast_mod(x >> 16, a.uni_size, a.mT);
      const uint64_t bk = slot[d] >> a.ushift;
      lo[d] = (uint32_t)a.uidx[bk];
      hi[d] = min((uint32_t)a.uidx[bk + 1] + 1u, a.uV);
    }
    for (bool more = true; more;) {  // the N binary searches (unigram_lookup) step together
      more = false;
#pragma unroll
      for (int d = 1; d <= N; d++) {
        if (hi[d] - lo[d] > 1) {
          const uint32_t mid = (lo[d] + hi[d]) >> 1;
          if (a.ustarts[mid] <= slot[d])
            lo[d] = mid;
          else
            hi[d] = mid;
          more |= hi[d] - lo[d] > 1;
        }
      }
    }
    int32_t tv[N + 1];
    tv[0] = word;
#pragma unroll
    for (int d = 1; d <= N; d++) {
      tv[d] = (int32_t)lo[d];
      if (a.trace) a.trace[p * N + d - 1] = tv[d];
      if (tv[d] == word) tv[d] = -1;
    }
    int32_t tu[N + 1];
    int32_t ts[N + 1];
    if (a.tloc) {  // the word itself: its token's entry
      const int2 x = a.tloc[t - a.t0];
      tu[0] = x.x;
      ts[0] = x.y;
    }
#pragma unroll
    for (int d = a.tloc ? 1 : 0; d <= N; d++) tu[d] = tv[d] >= 0 ? a.local[tv[d]] : -1;
#pragma unroll
    for (int d = a.tloc ? 1 : 0; d <= N; d++)
      ts[d] = (tu[d] >= 0 && a.vid_row) ? (kTabRow | (int32_t)a.vid_row[tv[d]]) : tv[d];
    // ---- stores: position record (LDS), gradient records (position-major) ----
#pragma unroll
    for (int j = 0; j < 2 * W; j++) {
      nctx += cv[j] >= 0;
      r[1 + j] = cs[j];
      const uint64_t k = HOFF + p * (uint64_t)(2 * W) + j;
      a.pkeys[k] = cu[j] >= 0 ? (uint32_t)cu[j] : a.U;
      if (a.pvals) a.pvals[k] = (uint32_t)k;
    }
#pragma unroll
    for (int d = 0; d <= N; d++) {
      ntgt += tv[d] >= 0;
      r[1 + 2 * W + d] = ts[d];
      const uint64_t k = p * (uint64_t)(N + 1) + d;
      a.pkeys[k] = tu[d] >= 0 ? (uint32_t)tu[d] : a.U;
      if (a.pvals) a.pvals[k] = (uint32_t)k;
    }
  }
  __syncthreads();
  {
    const uint32_t nn = (uint32_t)min<uint64_t>(blockDim.x, a.P - min(p0, a.P)) * (uint32_t)RS;
    int32_t *dst = a.rec + p0 * RS;
    for (uint32_t i = threadIdx.x; i < nn; i += blockDim.x) dst[i] = srec[i];
  }
  unsigned long long c = (unsigned long long)nctx, g = (unsigned long long)ntgt;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    c += __shfl_xor(c, off, 64);
    g += __shfl_xor(g, off, 64);
  }
  if (a.rows_touched && (threadIdx.x & 63) == 0 && (c | g)) {  // profiled passes only
    atomicAdd(&a.rows_touched[0], c);
    atomicAdd(&a.rows_touched[1], g);
  }
}

constexpr uint32_t kGroupDesc = 16;  // = kGroup (k_combine's group size)

// item descriptors {first record, end record | kind << 31, (key, kind) index j, chunk}:
// one thread per item (hot keys have thousands of chunks), j found by binary
// search over the item offsets ioff[0..2U].
struct MultiOrder {  // k_item_desc: sort keys of the multi-chunk items by their first record's position
  uint32_t *key, *item;  // [max_items]: coarse position (kMultiPad for the rest) and item index; null = unsorted
  const uint32_t *vals;  // the sorted records
  uint32_t SH, SV;  // record slots per position: N+1 targets (h), 2W contexts (v)
  uint64_t HOFF;
  int shift;  // coarse position = p >> shift (< kMultiPad)
};
constexpr uint32_t kMultiPad = 0xFFFFu;  // 16-bit sort keys: items outside the multi list sort last

// the (key, kind) run of every item without a search: each run with items marks its first item
// (run_of zeroed before), then an inclusive max-scan carries the mark over the run's other items
__global__ void k_item_heads(const uint32_t *__restrict__ ioff, uint32_t R, uint32_t *__restrict__ run_of) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= R) return;
  const uint32_t a = ioff[j];
  if (ioff[j + 1] > a) run_of[a] = j;
}

__global__ void k_item_desc(const uint32_t *__restrict__ seg, const uint32_t *__restrict__ ioff, uint32_t U,
                            uint32_t CH, uint32_t CHM, uint64_t max_items, uint4 *__restrict__ desc, uint32_t *__restrict__ lead,
                            uint32_t *__restrict__ multi, MultiOrder mo, const uint32_t *__restrict__ run_of = nullptr) {
  const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = item < max_items && item < ioff[2ull * U];
  uint32_t lo = 0, hi = 2 * U;  // largest j with ioff[j] <= item
  if (live && run_of)
    lo = run_of[item];
  else if (live)
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (ioff[mid] <= item)
        lo = mid;
      else
        hi = mid;
    }
  if (multi) {
    // items of (key, kind) runs with more than one chunk, for k_gather_t when
    // k_push_thp sums the single-chunk runs itself (list order is irrelevant:
    // every item writes only its own partial slot); one atomic per wave
    const bool m = live && ioff[lo + 1] - ioff[lo] > 1;
    if (mo.key && item < max_items) {
      uint32_t key = kMultiPad;
      if (m) {  // the chunk's first record: index p*SH + d (h), HOFF + p*SV + j (v)
        const uint32_t jj = lo, u = jj >> 1, kind = jj & 1, k = (uint32_t)item - ioff[jj];
        const uint32_t pi = mo.vals[seg[(2 * kind) * U + u] + k * CHM];
        key = (kind ? (uint32_t)((uint64_t)pi - mo.HOFF) / mo.SV : pi / mo.SH) >> mo.shift;
      }
      mo.key[item] = key;
      mo.item[item] = (uint32_t)item;
    }
    const uint64_t bal = __ballot(m);
    if (bal) {
      const int lane = threadIdx.x & 63;
      const int first = __ffsll((long long)bal) - 1;
      uint32_t base = 0;
      if (lane == first) base = atomicAdd(&multi[0], (uint32_t)__popcll(bal));
      base = (uint32_t)__shfl((int)base, first, 64);
      if (m && !mo.key) multi[1 + base + (uint32_t)__popcll(bal & ((1ULL << lane) - 1))] = (uint32_t)item;
    }
  }
  if (!live) return;
  const uint32_t jj = lo, u = jj >> 1, kind = jj & 1, k = (uint32_t)item - ioff[jj];
  const uint32_t s = seg[(2 * kind) * U + u], e = seg[(2 * kind + 1) * U + u];
  const uint32_t ck = ioff[jj + 1] - ioff[jj] > 1 ? CHM : CH;  // single-item runs hold up to CH records
  const uint32_t cs = s + k * ck;
  desc[item] = make_uint4(cs, min(cs + ck, e) | (kind << 31), jj, k);
  // hot (key, kind) runs of more than kGroup chunks: k_combine pre-sums each
  // group of kGroup partials into its leader (the list order does not
  // matter: every leader writes only its own slot)
  if (lead && ioff[jj + 1] - ioff[jj] > kGroupDesc && k % kGroupDesc == 0) lead[1 + atomicAdd(&lead[0], 1u)] = (uint32_t)item;
}

// the batch's local key map and its kept positions in one launch (thread i does both jobs' i-th item)
__global__ void k_batch_setup(const int32_t *__restrict__ K, uint32_t U, int32_t *__restrict__ local,
                              const int32_t *__restrict__ kscan, uint64_t t0, uint64_t nt,
                              int32_t *__restrict__ pos_tok, uint4 *__restrict__ seg0, uint32_t *__restrict__ lead,
                              uint32_t *__restrict__ multi, const uint32_t *__restrict__ vid_row,
                              uint32_t *__restrict__ krow) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < U) local[K[i]] = (int32_t)i;
  if (krow && i < U) krow[i] = vid_row[K[i]];  // the batch keys' shard rows (k_push_thp)
  if (seg0 && i < U) seg0[i] = make_uint4(0, 0, 0, 0);  // seg[4][U] u32 = U x 16 B: keys without records
  if (lead && i == 0) lead[0] = 0;
  if (multi && i == 0) multi[0] = 0;
  if (i < nt && pos_tok) {
    const int32_t a = kscan[t0 + i];
    if (kscan[t0 + i + 1] != a) pos_tok[a - kscan[t0]] = (int32_t)(t0 + i);
  }
}

// Segment bounds of every (local key, kind) run of the sorted records, one
// thread per record (records of key u: its h records, index < HOFF, then its
// v records, each run in index order: the sort is stable).  seg[0][u],
// seg[1][u] = h-record range; seg[2][u], seg[3][u] = v-record range; keys
// without records keep the zeros k_batch_setup wrote.
__global__ void k_seg_bounds(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t M,
                             uint32_t HOFF, uint32_t U, uint32_t *__restrict__ seg) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const uint32_t u = keys[i];
  if (u >= U) return;  // "no key" records sort last
  const bool first = i == 0 || keys[i - 1] != u, last = i + 1 == M || keys[i + 1] != u;
  const bool isv = vals[i] >= HOFF;
  if (first) seg[u] = i;
  if (last) seg[3 * U + u] = i + 1;
  // the h/v split: the first v record, or the run's end when it has none
  if ((first && isv) || (!first && isv && vals[i - 1] < HOFF)) {
    seg[U + u] = i;
    seg[2 * U + u] = i;
  } else if (last && !isv) {
    seg[U + u] = i + 1;
    seg[2 * U + u] = i + 1;
  }
}

// k_seg_bounds with 4 consecutive records per thread (16-B loads of the sorted keys and their
// record indices; the neighbours on either side from the next / previous thread's words): the same
// bounds, a quarter of the threads and load instructions
__global__ __launch_bounds__(256) void k_seg_bounds4(const uint32_t *__restrict__ keys,
                                                     const uint32_t *__restrict__ vals, uint32_t M, uint32_t HOFF,
                                                     uint32_t U, uint32_t *__restrict__ seg) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x, i0 = q * 4;
  if (i0 >= M) return;
  constexpr uint32_t kNone = 0xFFFFFFFFu;  // past either end: no key
  uint32_t k[6], v[5];
  if (i0 + 4 <= M) {
    const uint4 kk = ((const uint4 *)keys)[q], vv = ((const uint4 *)vals)[q];
    k[1] = kk.x, k[2] = kk.y, k[3] = kk.z, k[4] = kk.w;
    v[1] = vv.x, v[2] = vv.y, v[3] = vv.z, v[4] = vv.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      k[j + 1] = i0 + j < M ? keys[i0 + j] : kNone;
      v[j + 1] = i0 + j < M ? vals[i0 + j] : 0u;
    }
  }
  k[0] = i0 ? keys[i0 - 1] : kNone;
  v[0] = i0 ? vals[i0 - 1] : 0u;
  k[5] = i0 + 4 < M ? keys[i0 + 4] : kNone;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t i = i0 + j, u = k[j + 1];
    if (i >= M || u >= U) continue;  // "no key" records sort last
    const bool first = k[j] != u, last = k[j + 2] != u;
    const bool isv = v[j + 1] >= HOFF;
    if (first) seg[u] = i;
    if (last) seg[3 * U + u] = i + 1;
    if ((first && isv) || (!first && isv && v[j] < HOFF)) {
      seg[U + u] = i;
      seg[2 * U + u] = i;
    } else if (last && !isv) {
      seg[U + u] = i + 1;
      seg[2 * U + u] = i + 1;
    }
  }
}

// chunks of <= CH records per (key, kind) from the bounds; cnt[2U] = 0 (the
// scan's tail).  Profiled passes (gstats) also add the records / items to
// gstats[0..1].
__global__ void k_seg_counts(const uint32_t *__restrict__ seg, uint32_t U, uint32_t CH, uint32_t CHM,
                             uint32_t *__restrict__ cnt, unsigned long long *__restrict__ gstats) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long rc = 0, ic = 0, mr = 0, mi = 0;
  if (u == U) cnt[2 * U] = 0;
  if (u < U) {
    const uint32_t a = seg[u], lo = seg[U + u], b = seg[3 * U + u];
    // a run of <= CH records is one item; longer runs are chunks of CHM <= CH
    const uint32_t nh = lo - a, nv = b - lo;
    const uint32_t ch = nh <= CH ? (nh > 0) : (nh + CHM - 1) / CHM, cv = nv <= CH ? (nv > 0) : (nv + CHM - 1) / CHM;
    cnt[2 * u] = ch;
    cnt[2 * u + 1] = cv;
    rc = b - a;
    ic = ch + cv;
    mr = (ch > 1 ? lo - a : 0) + (cv > 1 ? b - lo : 0);  // multi-chunk runs: k_gather_t's share when fused
    mi = (ch > 1 ? ch : 0) + (cv > 1 ? cv : 0);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    rc += __shfl_xor(rc, off, 64);
    ic += __shfl_xor(ic, off, 64);
    mr += __shfl_xor(mr, off, 64);
    mi += __shfl_xor(mi, off, 64);
  }
  if (gstats && (threadIdx.x & 63) == 0 && rc) {
    atomicAdd(&gstats[0], rc);
    atomicAdd(&gstats[1], ic);
    atomicAdd(&gstats[2], mr);
    atomicAdd(&gstats[3], mi);
  }
}

}  // namespace

namespace swps {

int upload_lcg_constants() {
  uint64_t PA[64], PC[64];  // the main LCG's jumps by 2^i draws
  for (int i = 0; i < 64; i++) {
    PA[i] = lcg_jump(1, 1ULL << i, kLcgA, kLcgC) - lcg_jump(0, 1ULL << i, kLcgA, kLcgC);
    PC[i] = lcg_jump(0, 1ULL << i, kLcgA, kLcgC);
  }
  uint64_t FA[64], FC[64];  // the subsampling float LCG's jumps by 2^i draws
  for (int i = 0; i < 64; i++) {
    FA[i] = lcg_jump(1, 1ULL << i, kFlcgA, kLcgC) - lcg_jump(0, 1ULL << i, kFlcgA, kLcgC);
    FC[i] = lcg_jump(0, 1ULL << i, kFlcgA, kLcgC);
  }
  if (hipMemcpyToSymbol(HIP_SYMBOL(c_f2A), FA, sizeof(FA)) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(c_f2C), FC, sizeof(FC)) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(c_p2A), PA, sizeof(PA)) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(c_p2C), PC, sizeof(PC)) != hipSuccess)
    return fail(SWPS_E_HIP, "constant upload");
  return SWPS_OK;
}

// Subsample masks and main-LCG offsets for a whole epoch.  They depend only on
// the two RNG streams (the float LCG advances one draw per processed token,
// the main LCG 1 + kept*(1+negative) draws per line), never on the
// parameters, so one pass per epoch replaces per-batch host syncs.
// Size every per-batch buffer for the epoch's largest batch once, at plan
// time, so no hipMalloc / hipFree (a device-wide sync) lands inside a step.
static int presize(swps_w2v *w, uint64_t maxP) {
  if (maxP == 0) return SWPS_OK;
  const int W = w->W, N = w->N, D = w->D, RS = 2 * W + N + 2;
  const uint64_t HOFF = maxP * (uint64_t)(N + 1), M = HOFF + maxP * (uint64_t)(2 * W);
  if (M >= (1ULL << 31)) return SWPS_OK;  // prep_batch reports it
  const size_t a = (w->f64 || w->cfg.fp64_intermediates) ? 8 : 4;  // partials (split mode: fp64 too)
  const uint64_t nrow = w->bfp ? (uint64_t)bfp_ld(D, w->bfp_rb) * 4 : (uint64_t)row_ld(D, a, w->row_pad) * a;
  SWPS_TRY(w->d_pos_tok.ensure(maxP * 4));
  SWPS_TRY(w->d_rec.ensure(maxP * RS * 4));
  SWPS_TRY(w->d_pkeys.ensure(M * 4));
  SWPS_TRY(w->d_pvals.ensure(M * 4));
  SWPS_TRY(w->d_pkeys_s.ensure(M * 4));
  SWPS_TRY(w->d_pvals_s.ensure(M * 4));
  SWPS_TRY(w->d_neu1.ensure(maxP * nrow));
  SWPS_TRY(w->d_neu1e.ensure(maxP * nrow));
  SWPS_TRY(w->d_pg.ensure(HOFF * 4));
  const uint64_t U = w->max_U;
  if (U) {
    int bits = 1;
    while ((1ULL << bits) <= U) bits++;
    // smaller batches of the epoch may take the small-tile sort (swps_sort.h): size for both
    for (uint64_t n : {M, std::min<uint64_t>(M, kSmallSort - 1)}) {
      SWPS_TRY(sort_pairs(w->d_tmp, w->d_pkeys.as<uint32_t>(), w->d_pkeys_s.as<uint32_t>(), w->d_pvals.as<uint32_t>(),
                          w->d_pvals_s.as<uint32_t>(), n, bits, w->s, false));
      SWPS_TRY(sort_pairs_iota(w->d_tmp, w->d_pkeys.as<uint32_t>(), w->d_pkeys_s.as<uint32_t>(),
                               w->d_pvals_s.as<uint32_t>(), n, bits, w->s, false));
    }
    const uint64_t max_items = 2ULL * U + M / multi_chunk(w, maxP) + 1;
    SWPS_TRY(w->d_lead.ensure((max_items / 8 + 2) * 4));
    SWPS_TRY(w->d_seg.ensure(U * 16));
    SWPS_TRY(w->d_icnt.ensure((2ULL * U + 1) * 4));
    SWPS_TRY(w->d_ioff.ensure((2ULL * U + 1) * 4));
    SWPS_TRY(w->d_desc.ensure(max_items * 16));
    SWPS_TRY(w->d_partial.ensure(max_items * D * a));
    SWPS_TRY(w->d_multi.ensure((max_items + 1) * 4));
    if (w->multi_sort && maxP >= w->multi_sort_min) {  // the multi-item order sort (prep_batch)
      SWPS_TRY(w->d_pkeys.ensure(max_items * 4));
      SWPS_TRY(w->d_pvals.ensure(max_items * 4));
      SWPS_TRY(w->d_icnt.ensure(max_items * 4));
      for (uint64_t n : {max_items, std::min<uint64_t>(max_items, kSmallSort - 1)})
        SWPS_TRY(sort_pairs(w->d_tmp, w->d_pkeys.as<uint32_t>(), w->d_icnt.as<uint32_t>(), w->d_pvals.as<uint32_t>(),
                            w->d_multi.as<uint32_t>(), n, 16, w->s, false));
    }
  }
  return SWPS_OK;
}

int plan_epoch(swps_w2v *w) {
  hipStream_t s = w->s;
  const uint64_t nb = w->batches.size();
  const uint64_t L = w->batches[nb - 1].l1;             // lines processed per epoch
  const uint64_t T = (uint64_t)w->line_off[L];          // tokens processed per epoch
  const bool sample_on = w->cfg.sample >= 0;
  SWPS_TRY(w->d_kflag.ensure((T + 1) * 4));
  SWPS_TRY(w->d_kscan.ensure((T + 1) * 4));
  SWPS_TRY(w->d_ldraw.ensure((L + 1) * 8));
  SWPS_TRY(w->d_ldoff.ensure((L + 1) * 8));
  hipEvent_t ek = w->timer.begin(s);
  std::vector<int32_t> tw;
  if (w->cfg.minibatch_vocab) {
    // _num_words when batch b of epoch e trains: the first full gather, e whole
    // epochs of gathers (incl. each epoch's final short gather), this epoch's
    // gathers up to b; `int train_words = num_words()` truncates to 32 bits
    const uint64_t e = w->cursor / nb;
    uint64_t per_epoch = w->gather_end;
    for (auto &b : w->batches) per_epoch += b.gathered;
    uint64_t acc = w->train_words + e * per_epoch;
    tw.resize(nb);
    for (uint64_t b = 0; b < nb; b++) {
      acc += w->batches[b].gathered;
      tw[b] = (int32_t)(uint32_t)acc;
    }
    SWPS_HIP(hipMemcpyAsync(w->d_tw.p, tw.data(), nb * 4, hipMemcpyHostToDevice, s));
    k_keep_mb<<<nblk((T + kKeepRun) / kKeepRun), 256, 0, s>>>(w->d_bcnt_tok.as<int32_t>(), T, w->d_btok.as<int64_t>(),
                                                              (uint32_t)nb, w->d_tw.as<int32_t>(), w->cfg.sample,
                                                              w->fstate, sample_on, w->d_kflag.as<int32_t>());
  } else {
    k_keep<<<nblk((T + 64 * kKeepIt) / (64 * kKeepIt) * 64), 256, 0, s>>>(w->d_tok.as<int32_t>(), T, w->d_ran.as<float>(),
                                                                          w->fstate, sample_on, w->d_kflag.as<int32_t>());
  }
  SWPS_HIP(hipGetLastError());
  SWPS_TRY(exclusive_scan(w->d_kflag.as<int32_t>(), w->d_kscan.as<int32_t>(), T + 1, w->d_tmp, s));
  k_line_draws<<<nblk(L + 1), 256, 0, s>>>(w->d_line_off.as<int64_t>(), L, w->d_kscan.as<int32_t>(), w->N,
                                           w->d_ldraw.as<uint64_t>());
  SWPS_HIP(hipGetLastError());
  SWPS_TRY(exclusive_scan(w->d_ldraw.as<uint64_t>(), w->d_ldoff.as<uint64_t>(), L + 1, w->d_tmp, s));
  w->timer.end(KT_KEEP, ek, s);
  // per-batch kept counts: kscan at every batch's token boundary
  SWPS_TRY(w->d_bounds.ensure((nb + 1) * 4));
  k_bounds<<<nblk(nb + 1), 256, 0, s>>>(w->d_kscan.as<int32_t>(), w->d_btok.as<int64_t>(), nb + 1,
                                        w->d_bounds.as<int32_t>());
  SWPS_HIP(hipGetLastError());
  std::vector<int32_t> ks(nb + 1);
  SWPS_HIP(hipMemcpyAsync(ks.data(), w->d_bounds.p, (nb + 1) * 4, hipMemcpyDeviceToHost, s));
  uint64_t draws = 0;
  SWPS_HIP(hipMemcpyAsync(&draws, w->d_ldoff.as<uint64_t>() + L, 8, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  w->plan_P.resize(nb);
  uint64_t maxP = 0;
  for (uint64_t i = 0; i < nb; i++) {
    w->plan_P[i] = (uint32_t)(ks[i + 1] - ks[i]);
    maxP = std::max<uint64_t>(maxP, w->plan_P[i]);
  }
  SWPS_TRY(presize(w, maxP));
  w->lstate_epoch = w->lstate;
  w->fstate_epoch = w->fstate;
  w->lstate = lcg_jump(w->lstate, draws, kLcgA, kLcgC);
  if (sample_on) w->fstate = lcg_jump(w->fstate, T, kFlcgA, kLcgC);
  return SWPS_OK;
}

// ---- one minibatch, in two halves ------------------------------------------
// prep_batch: everything that depends only on the corpus, the RNG streams and
// the batch's key set — the epoch plan, the local key map, the position and
// gradient records (learn_instance's draws) and the inverted index (sorted
// records, segments, chunk descriptors).  learn_batch: everything that reads
// parameters — pull (or install of the owners' values), forward, gathered
// gradient sums, push.  The sharded driver issues prep(i+1) right after
// learn(i) on the compute stream, so it runs while minibatch i's push and
// i+1's pull cross the fabric (exact lockstep semantics kept).

int prep_batch(swps_w2v *w) {
  if (w->pb.valid) return SWPS_OK;
  const uint64_t nb = w->batches.size();
  if (w->cursor % nb == 0) SWPS_TRY(plan_epoch(w));
  const uint64_t bi = w->cursor % nb;
  const swps_w2v::Batch &B = w->batches[bi];
  hipStream_t s = w->s;
  Timer &tm = w->timer;
  const int W = w->W, N = w->N;
  const uint64_t t0 = (uint64_t)w->line_off[B.l0], t1 = (uint64_t)w->line_off[B.l1];
  const uint64_t nt = t1 - t0;
  const uint32_t U = B.U;
  const int32_t *K = w->d_K.as<int32_t>() + B.kofs;
  const uint64_t P = w->plan_P[bi];
  auto &pb = w->pb;
  pb = swps_w2v::Prepped();
  pb.bi = bi;
  pb.P = P;
  pb.U = U;
  pb.nt = nt;
  // local key map of the batch (the grads[key] slots the pull resets,
  // global_pull_access.h:88-97; cleared again by the push) and the batch's
  // kept token indices, in one launch
  const bool tracing = w->trace.size() < w->trace_cap;
  const bool recs = P > 0 && (U > 0 || tracing);
  if (recs) SWPS_TRY(w->d_pos_tok.ensure(P * 4));
  const bool will_sort = recs && U > 0;
  if (will_sort) {  // zeroed by k_batch_setup: keys without records keep empty segments
    SWPS_TRY(w->d_seg.ensure((uint64_t)U * 16));
    // leaders: at most 2 per 17 items (a run of kGroup + 1 chunks has two)
    const uint64_t mi = 2ULL * U + P * (uint64_t)(N + 1 + 2 * W) / multi_chunk(w, P) + 1;  // max items
    SWPS_TRY(w->d_lead.ensure((mi / 8 + 2) * 4));
    SWPS_TRY(w->d_multi.ensure((mi + 1) * 4));
  }
  // the fused push's per-key shard rows (single GPU)
  const bool krow = U > 0 && !w->sharded && (w->bfp || (w->tail && w->fused_push));
  if (krow) SWPS_TRY(w->d_krow.ensure((uint64_t)U * 4));
  if (U || recs) {
    k_batch_setup<<<nblk(std::max<uint64_t>(U, recs ? nt : 0)), 256, 0, s>>>(
        K, U, w->d_local.as<int32_t>(), w->d_kscan.as<int32_t>(), t0, recs ? nt : 0,
        recs ? w->d_pos_tok.as<int32_t>() : nullptr, will_sort ? w->d_seg.as<uint4>() : nullptr,
        will_sort ? w->d_lead.as<uint32_t>() : nullptr, will_sort ? w->d_multi.as<uint32_t>() : nullptr,
        w->d_vid_row.as<uint32_t>(), krow ? w->d_krow.as<uint32_t>() : nullptr);
    SWPS_HIP(hipGetLastError());
  }
  if (recs) {
    // ---- position records + gradient records (learn_instance's draws) ----
    const uint64_t HOFF = P * (uint64_t)(N + 1);
    const uint64_t M = HOFF + P * (uint64_t)(2 * W);
    const int RS = 2 * W + N + 2;
    if (M >= (1ULL << 31)) return fail(SWPS_E_UNSUPPORTED, "minibatch too large (2^31 gradient records)");
    SWPS_TRY(w->d_pos_tok.ensure(P * 4));
    SWPS_TRY(w->d_rec.ensure(P * RS * 4));
    SWPS_TRY(w->d_pkeys.ensure(M * 4));
    SWPS_TRY(w->d_pvals.ensure(M * 4));
    SWPS_TRY(w->d_pkeys_s.ensure(M * 4));
    SWPS_TRY(w->d_pvals_s.ensure(M * 4));
    if (tracing) SWPS_TRY(w->d_trace.ensure(std::max<uint64_t>(1, P * N) * 4));
    const bool use_uidx = !w->cfg.minibatch_vocab && w->cfg.sampler != SWPS_SAMPLER_ALIAS && w->uni_index &&
                          w->d_uidx.p != nullptr;
    RecArgs ra{w->d_tok.as<int32_t>(), w->d_tok_line.as<int32_t>(), w->d_line_off.as<int64_t>(),
               w->d_pos_tok.as<int32_t>(), (uint32_t)P, w->d_kscan.as<int32_t>(), w->d_ldoff.as<uint64_t>(),
               w->lstate_epoch, W, N, ~0ULL / (uint64_t)W, w->d_unigram.as<int32_t>(), w->cfg.unigram_size,
               ~0ULL / w->cfg.unigram_size,
               w->cfg.minibatch_vocab ? w->d_bstarts.as<uint64_t>() + B.sofs : nullptr,
               w->cfg.minibatch_vocab ? w->d_UK.as<int32_t>() + B.kofs : nullptr, U,
               use_uidx ? w->d_starts.as<uint64_t>() : nullptr, use_uidx ? w->d_uidx.as<int32_t>() : nullptr,
               kUShift, (uint32_t)w->vocab_keys.size(),
               w->cfg.sampler == SWPS_SAMPLER_ALIAS
                   ? w->d_alias.as<uint2>() + (w->cfg.minibatch_vocab ? B.kofs : 0)
                   : nullptr,
               w->cfg.minibatch_vocab ? U : (uint32_t)w->vocab_keys.size(),
               w->d_local.as<int32_t>(), U, w->sharded ? nullptr : w->d_vid_row.as<uint32_t>(), w->d_rec.as<int32_t>(),
               w->d_pkeys.as<uint32_t>(), sort_iota() ? nullptr : w->d_pvals.as<uint32_t>(),
               tracing ? w->d_trace.as<int32_t>() : nullptr,
               tm.on ? w->d_rows_touched.as<unsigned long long>() : nullptr, nullptr, t0};
    if (W == 5 && N == 5 && use_uidx && !w->rec_generic && w->tok_local) {  // k_records_t reads per-token lookups
      SWPS_TRY(w->d_tloc.ensure(std::max<uint64_t>(nt, 1) * 8));
      k_tok_local<<<nblk(nt), 256, 0, s>>>(w->d_tok.as<int32_t>() + t0, nt, w->d_local.as<int32_t>(),
                                           w->sharded ? nullptr : w->d_vid_row.as<uint32_t>(), w->d_tloc.as<int2>());
      SWPS_HIP(hipGetLastError());
      ra.tloc = w->d_tloc.as<int2>();
    }
    hipEvent_t er = tm.begin(s);
    if (W == 5 && N == 5 && use_uidx && !w->rec_generic)
      k_records_t<5, 5><<<nblk(P), 256, 256 * RS * sizeof(int32_t), s>>>(ra);
    else
      k_records<<<nblk(P), 256, 256 * RS * sizeof(int32_t), s>>>(ra);
    SWPS_HIP(hipGetLastError());
    tm.end(KT_REC, er, s);
    pb.records = true;
    pb.HOFF = HOFF;
    pb.M = M;
    if (tracing) {
      std::vector<int32_t> tr(P * N);
      if (!tr.empty()) {
        SWPS_HIP(hipMemcpyAsync(tr.data(), w->d_trace.p, tr.size() * 4, hipMemcpyDeviceToHost, s));
        SWPS_HIP(hipStreamSynchronize(s));
      }
      for (auto v : tr)
        if (w->trace.size() < w->trace_cap) w->trace.push_back(v);
    }
    if (U > 0) {
      // ---- inverted index: stable radix sort of records by local key ----
      int bits = 1;
      while ((1ULL << bits) <= U) bits++;
      hipEvent_t es = tm.begin(s);
      if (sort_iota())  // the values are the record indices 0..M-1 (the records kernel wrote none)
        SWPS_TRY(sort_pairs_iota(w->d_tmp, w->d_pkeys.as<uint32_t>(), w->d_pkeys_s.as<uint32_t>(),
                                 w->d_pvals_s.as<uint32_t>(), M, bits, s));
      else
        SWPS_TRY(sort_pairs(w->d_tmp, w->d_pkeys.as<uint32_t>(), w->d_pkeys_s.as<uint32_t>(),
                            w->d_pvals.as<uint32_t>(), w->d_pvals_s.as<uint32_t>(), M, bits, s));
      SWPS_TRY(w->d_icnt.ensure((2ULL * U + 1) * 4));
      SWPS_TRY(w->d_ioff.ensure((2ULL * U + 1) * 4));
      if (w->seg4)
        k_seg_bounds4<<<nblk((M + 3) / 4), 256, 0, s>>>(w->d_pkeys_s.as<uint32_t>(), w->d_pvals_s.as<uint32_t>(),
                                                        (uint32_t)M, (uint32_t)HOFF, U, w->d_seg.as<uint32_t>());
      else
        k_seg_bounds<<<nblk(M), 256, 0, s>>>(w->d_pkeys_s.as<uint32_t>(), w->d_pvals_s.as<uint32_t>(), (uint32_t)M,
                                              (uint32_t)HOFF, U, w->d_seg.as<uint32_t>());
      const uint32_t chm = multi_chunk(w, P);
      k_seg_counts<<<nblk((uint64_t)U + 1), 256, 0, s>>>(w->d_seg.as<uint32_t>(), U, kChunk, chm, w->d_icnt.as<uint32_t>(),
                                                          tm.on ? w->d_gstats.as<unsigned long long>() : nullptr);
      SWPS_HIP(hipGetLastError());
      SWPS_TRY(exclusive_scan(w->d_icnt.as<uint32_t>(), w->d_ioff.as<uint32_t>(), 2ULL * U + 1, w->d_tmp, s));
      const uint64_t max_items = 2ULL * U + M / chm + 1;
      SWPS_TRY(w->d_desc.ensure(max_items * 16));
      // multi-chunk items in the order of their first record's position when
      // the batch's neu1 / neu1e rows outgrow the Infinity Cache: concurrently
      // running gather waves then read nearby positions, so a row's ~6
      // re-reads (by the records of its other keys) hit the cache
      MultiOrder mo{};
      const bool msort = w->multi_sort && P >= w->multi_sort_min;
      if (msort) {
        SWPS_TRY(w->d_pkeys.ensure(max_items * 4));
        SWPS_TRY(w->d_pvals.ensure(max_items * 4));
        SWPS_TRY(w->d_icnt.ensure(max_items * 4));
        int shift = 0;
        while ((P >> shift) >= kMultiPad) shift++;
        mo = MultiOrder{w->d_pkeys.as<uint32_t>(), w->d_pvals.as<uint32_t>(), w->d_pvals_s.as<uint32_t>(),
                        (uint32_t)(N + 1), (uint32_t)(2 * W), HOFF, shift};
      }
      const uint32_t *run_of = nullptr;
      if (w->item_heads) {  // every item's run by a max-scan of the runs' first items (no binary search)
        SWPS_TRY(w->d_irun.ensure(max_items * 4));
        SWPS_HIP(hipMemsetAsync(w->d_irun.p, 0, max_items * 4, s));
        k_item_heads<<<nblk(2ULL * U), 256, 0, s>>>(w->d_ioff.as<uint32_t>(), 2 * U, w->d_irun.as<uint32_t>());
        SWPS_TRY(inclusive_max_scan(w->d_irun.as<uint32_t>(), max_items, w->d_tmp, s));
        run_of = w->d_irun.as<uint32_t>();
      }
      k_item_desc<<<nblk(max_items), 256, 0, s>>>(w->d_seg.as<uint32_t>(), w->d_ioff.as<uint32_t>(), U, kChunk, chm,
                                                   max_items, w->d_desc.as<uint4>(), w->d_lead.as<uint32_t>(),
                                                   w->d_multi.as<uint32_t>(), mo, run_of);
      SWPS_HIP(hipGetLastError());
      pb.msorted = msort;
      if (msort)  // stable: equal coarse positions keep item order
        SWPS_TRY(sort_pairs(w->d_tmp, w->d_pkeys.as<uint32_t>(), w->d_icnt.as<uint32_t>(), w->d_pvals.as<uint32_t>(),
                            w->d_multi.as<uint32_t>() + 1, max_items, 16, s));
      SWPS_HIP(hipGetLastError());
      tm.end(KT_SORT, es, s);
      pb.sorted = true;
      pb.max_items = max_items;
    }
  }
  if (U > 0 && !pb.sorted) {  // no records: the push sees empty segments
    SWPS_TRY(w->d_seg.ensure((uint64_t)U * 16));
    SWPS_HIP(hipMemsetAsync(w->d_seg.p, 0, (uint64_t)U * 16, s));
    SWPS_TRY(w->d_ioff.ensure((2ULL * U + 1) * 4));
    SWPS_HIP(hipMemsetAsync(w->d_ioff.p, 0, (2ULL * U + 1) * 4, s));
  }
  pb.valid = true;
  return SWPS_OK;
}

}  // namespace swps
