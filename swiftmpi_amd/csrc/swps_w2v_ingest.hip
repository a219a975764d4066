// word2vec corpus ingest (swps_w2v_ctx.h): text or token ids -> vocab, vid
// tokens, the per-epoch batch schedule with every batch's key set, and the
// device tables the minibatch kernels read (unigram table and its coarse
// index, subsampling thresholds, exp table, alias tables).  A host
// restatement of the reference (ingest, build_schedule, build_schedule_mb) and
// the same on the GPU (tokenize_gpu, ingest_gpu, schedule_gpu), bit for bit.
#include <algorithm>
#include <cmath>
#include <map>
#include <unordered_map>
#include <unordered_set>

#include "swps_scan.h"
#include "swps_sort.h"
#include "swps_w2v_ctx.h"

using namespace swps;

namespace {

__global__ void k_build_unigram(const uint64_t *__restrict__ starts, uint32_t V, uint64_t T, int32_t *__restrict__ table) {
  uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; a < T; a += stride) {
    uint32_t lo = 0, hi = V;  // largest i with starts[i] <= a
    while (hi - lo > 1) {
      uint32_t mid = (lo + hi) >> 1;
      if (starts[mid] <= a)
        lo = mid;
      else
        hi = mid;
    }
    table[a] = (int32_t)lo;
  }
}

// Coarse index over the run-length unigram table: idx[b] = the word holding
// slot b << shift (the same "largest i with starts[i] <= a" as
// k_build_unigram), b in [0, nb].  A draw then binary-searches starts[] only
// between idx[b] and idx[b+1] (a few runs at 1024 slots per bucket) — 2.4 MB
// of L2-resident index instead of one random 4-B read into the 400-MB table.
__global__ void k_build_uidx(const uint64_t *__restrict__ starts, uint32_t V, int shift, uint64_t nb1,
                             int32_t *__restrict__ idx) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb1) return;
  const uint64_t a = b << shift;
  uint32_t lo = 0, hi = V;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (starts[mid] <= a)
      lo = mid;
    else
      hi = mid;
  }
  idx[b] = (int32_t)lo;
}

// ============================================================================
// Corpus ingest on the GPU (word2vec_global.h:215-227
// parse_instance, :385-444 gather_keys with nthreads = 1, :335-381 the
// minibatch windows).  Same results as the host restatement below (ingest +
// build_schedule), bit for bit; the host keeps only per-line and per-word
// work (line validity, the std::unordered_set iteration order of the V
// distinct keys, the batch boundaries):
//   tokenize   text bytes -> token starts (scan), BKDR / atoi per token
//   vocab      stable radix sort of (key, position); per run: count over valid
//              lines and first valid position (integer atomics: exact);
//              host inserts the V keys into std::unordered_set in first-
//              occurrence order (its iteration order = the vid order) and
//              sends back vid per run; tok[position] = vid
//   schedule   (batch << 32 | vid) for every token of every batch's B+3-line
//              window, radix sort, unique -> each batch's sorted key set
// ============================================================================
__global__ void k_tok_fp(const int32_t *__restrict__ tok, uint64_t n, unsigned long long *__restrict__ out) {
  unsigned long long acc = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    acc += splitmix64((uint64_t)(uint32_t)tok[i] ^ (i * 0x9E3779B97F4A7C15ULL));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);  // a wrapping integer sum: order-independent
}

// per byte: token start (not a delimiter, after a delimiter or at 0) and
// newline flags; element nb is 0 so the exclusive scans end with the totals
__global__ void k_text_flags(const char *__restrict__ t, uint64_t nb, uint32_t *__restrict__ st,
                             uint32_t *__restrict__ nl) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nb) return;
  if (i == nb) {
    st[i] = 0;
    nl[i] = 0;
    return;
  }
  const char c = t[i], p = i ? t[i - 1] : '\n';
  st[i] = (c != ' ' && c != '\n' && (p == ' ' || p == '\n')) ? 1u : 0u;
  nl[i] = c == '\n' ? 1u : 0u;
}

// token start positions, and line_off[l + 1] = first token after newline l
__global__ void k_text_index(const char *__restrict__ t, uint64_t nb, const uint32_t *__restrict__ st,
                             const uint32_t *__restrict__ tix, const uint32_t *__restrict__ lix,
                             uint64_t *__restrict__ tstart, int64_t *__restrict__ line_off) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  if (st[i]) tstart[tix[i]] = i;
  if (t[i] == '\n') line_off[lix[i] + 1] = (int64_t)tix[i + 1];
}

// BKDRHash (string.h:130-137: signed char) or atoi (word2vec.h:206) of one token
__global__ void k_text_keys(const char *__restrict__ t, uint64_t nb, const uint64_t *__restrict__ tstart, uint64_t n,
                            int atoi_mode, uint64_t *__restrict__ keys) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint64_t i = tstart[k];
  if (!atoi_mode) {
    uint64_t h = 0;
    for (; i < nb && t[i] != ' ' && t[i] != '\n'; i++) h = h * 13131ULL + (uint64_t)(int64_t)(signed char)t[i];
    keys[k] = h;
    return;
  }
  // glibc atoi = (int)strtol(s, 0, 10): leading isspace, sign, digits; strtol saturates
  uint64_t e = i;
  while (e < nb && t[e] != ' ' && t[e] != '\n') e++;
  while (i < e && (t[i] == '\t' || t[i] == '\v' || t[i] == '\f' || t[i] == '\r')) i++;
  bool neg = false;
  if (i < e && (t[i] == '+' || t[i] == '-')) neg = t[i++] == '-';
  const uint64_t lim = neg ? 9223372036854775808ULL : 9223372036854775807ULL;
  uint64_t v = 0;
  bool ovf = false;
  for (; i < e && t[i] >= '0' && t[i] <= '9'; i++) {
    const uint64_t d = (uint64_t)(t[i] - '0');
    if (ovf || v > (lim - d) / 10)
      ovf = true;
    else
      v = v * 10 + d;
  }
  if (ovf) v = lim;
  const int64_t sv = neg ? (int64_t)(0 - v) : (int64_t)v;
  keys[k] = (uint64_t)(int64_t)(int32_t)sv;
}

__global__ void k_gather_keys(const uint32_t *__restrict__ ids, uint64_t n, const uint64_t *__restrict__ wk,
                              uint64_t nw, uint64_t *__restrict__ keys, uint32_t *__restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = ids[i];
  if (id >= nw) {
    *bad = 1;
    keys[i] = 0;
  } else {
    keys[i] = wk[id];
  }
}

// line of every token (upper bound in line_off) and its validity
__global__ void k_tok_lines(const int64_t *__restrict__ off, uint64_t nl, uint64_t n, int min_len,
                            int32_t *__restrict__ tline, uint32_t *__restrict__ pos) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint64_t lo = 0, hi = nl;  // largest l with off[l] <= t (empty lines share an offset: take the last)
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)off[mid] <= t)
      lo = mid;
    else
      hi = mid;
  }
  tline[t] = (int32_t)lo;
  pos[t] = (uint32_t)t;
}

// run heads of the sorted keys, and whether each sorted token lies in a valid
// (gathered) line
__global__ void k_run_heads(const uint64_t *__restrict__ k, const uint32_t *__restrict__ ps, uint64_t n,
                            const int32_t *__restrict__ tline, const int64_t *__restrict__ off, int min_len,
                            uint32_t *__restrict__ head, uint32_t *__restrict__ valid) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    valid[n] = 0;  // the exclusive scan's tail
    return;
  }
  head[i] = (i == 0 || k[i] != k[i - 1]) ? 1u : 0u;
  const int32_t l = tline[ps[i]];
  valid[i] = off[l + 1] - off[l] >= min_len ? 1u : 0u;
}

__global__ void k_run_starts(const uint64_t *__restrict__ ks, const uint32_t *__restrict__ head,
                             const uint32_t *__restrict__ rid1, uint64_t n, uint64_t *__restrict__ ukey,
                             uint32_t *__restrict__ rstart) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  const uint32_t r = rid1[i] - 1;
  ukey[r] = ks[i];
  rstart[r] = (uint32_t)i;
}

// per run (one thread, no atomics: a hot word's run has millions of tokens):
// tokens in valid lines = difference of the valid-flag scan; first valid
// position = the first valid element (the sort is stable: positions ascend)
__global__ void k_run_stats(const uint32_t *__restrict__ rstart, uint32_t R, uint64_t n,
                            const uint32_t *__restrict__ vscan, const uint32_t *__restrict__ valid,
                            const uint32_t *__restrict__ ps, uint32_t *__restrict__ cnt, uint32_t *__restrict__ first) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const uint64_t s = rstart[r], e = r + 1 < R ? rstart[r + 1] : n;
  cnt[r] = vscan[e] - vscan[s];
  uint64_t i = s;
  while (i < e && !valid[i]) i++;
  first[r] = i < e ? ps[i] : 0xFFFFFFFFu;
}

__global__ void k_tok_vid(const uint32_t *__restrict__ ps, const uint32_t *__restrict__ rid1, uint64_t n,
                          const int32_t *__restrict__ vid_of_run, int32_t *__restrict__ tok) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tok[ps[i]] = vid_of_run[rid1[i] - 1];
}

// (batch << 32 | vid) of every token of every batch's gather window; tokens
// of invalid lines (never gathered) get the sentinel, which sorts last
__global__ void k_sched_keys(const uint64_t *__restrict__ eoff, const int64_t *__restrict__ ta, uint32_t nb,
                             uint64_t E, const int32_t *__restrict__ tok, const int32_t *__restrict__ tline,
                             const uint8_t *__restrict__ valid, uint64_t *__restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  uint32_t lo = 0, hi = nb;  // batch: largest b with eoff[b] <= e
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (eoff[mid] <= e)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t t = (uint64_t)ta[lo] + (e - eoff[lo]);
  out[e] = valid[tline[t]] ? ((uint64_t)lo << 32) | (uint32_t)tok[t] : ~0ULL;
}

__global__ void k_uniq_flags(const uint64_t *__restrict__ k, uint64_t n, uint32_t *__restrict__ f) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f[i] = (k[i] != ~0ULL && (i == 0 || k[i] != k[i - 1])) ? 1u : 0u;
}

__global__ void k_uniq_scatter(const uint64_t *__restrict__ k, const uint32_t *__restrict__ f,
                               const uint32_t *__restrict__ at, uint64_t n, uint64_t *__restrict__ uk,
                               int32_t *__restrict__ K) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && f[i]) {
    uk[at[i]] = k[i];
    K[at[i]] = (int32_t)(uint32_t)k[i];
  }
}

// kofs[b] = first unique key of batch b (lower bound of b << 32)
__global__ void k_batch_kofs(const uint64_t *__restrict__ uk, uint64_t nu, uint32_t nb, uint64_t *__restrict__ kofs) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nb) return;
  const uint64_t v = (uint64_t)b << 32;
  uint64_t lo = 0, hi = nu;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (uk[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  kofs[b] = lo;
}

}  // namespace

namespace swps {

int check_cfg(swps_w2v *w) {
  const auto &c = w->cfg;
  if (c.window <= 0 || 2 * c.window > 64) return fail(SWPS_E_CFG, "window must be in [1, 32]");
  if (c.negative < 0 || c.negative + 1 > 64) return fail(SWPS_E_CFG, "negative must be in [0, 63]");
  if (c.minibatch <= 0) return fail(SWPS_E_CFG, "minibatch must be positive");
  if (c.unigram_size == 0 || c.unigram_size > (1ULL << 31)) return fail(SWPS_E_CFG, "unigram_size out of range");
  if (c.sampler != SWPS_SAMPLER_TABLE && c.sampler != SWPS_SAMPLER_ALIAS) return fail(SWPS_E_CFG, "unknown sampler");
  const int E = w->f64 ? 2 : 4;
  if (w->D % E != 0) return fail(SWPS_E_UNSUPPORTED, "dim must be a multiple of 16 bytes (4 fp32 / 2 fp64)");
  int nc = w->D / E;
  w->NCH = (nc + 63) / 64;
  if (!w->f64 && w->D > 256 && w->D % 256 != 0 && w->D % 256 <= 64) w->tail = true;
  if (const char *e = getenv("SWPS_SLICE")) w->tail = w->tail && atoi(e) != 0;  // A/B timing
  if (w->NCH > 4) return fail(SWPS_E_UNSUPPORTED, "dim too large (max 1024 fp32 / 512 fp64)");
  if (c.fp64_intermediates < SWPS_INTER_FP32 || c.fp64_intermediates > SWPS_INTER_BFP32)
    return fail(SWPS_E_CFG, "fp64_intermediates must be SWPS_INTER_FP32, _FP64, _BFP40 or _BFP32");
  if (!w->f64 && (c.fp64_intermediates == SWPS_INTER_BFP40 || c.fp64_intermediates == SWPS_INTER_BFP32)) {
    if (w->D > kBfpMaxD) return fail(SWPS_E_UNSUPPORTED, "BFP intermediates: dim at most 512");
    w->bfp = true;
    w->bfp_rb = c.fp64_intermediates == SWPS_INTER_BFP40 ? 1 : 0;
  }
  return SWPS_OK;
}

// Vocab (word2vec_global.h:385-444, nthreads = 1): word counts over valid
// lines, `_local_keys` filled in first-occurrence order; vid = position in the
// std::unordered_set iteration order (= `_wordids`, the unigram-table order).
int ingest(swps_w2v *w, const std::vector<uint64_t> &tok_keys, std::vector<int64_t> &&line_off) {
  const uint64_t nl = line_off.size() - 1;
  w->line_off = std::move(line_off);
  w->line_valid.assign(nl, 0);
  std::unordered_map<uint64_t, int32_t> cnt;
  std::unordered_set<uint64_t> local_keys;
  uint64_t tw = 0;
  for (uint64_t l = 0; l < nl; l++) {
    const int64_t a = w->line_off[l], b = w->line_off[l + 1];
    const bool valid = (b - a) >= w->cfg.min_sentence_length;
    w->line_valid[l] = valid;
    if (w->cfg.minibatch_vocab && !valid && b > a)
      return fail(SWPS_E_UNSUPPORTED, "minibatch-vocab mode: a non-empty line shorter than min_sentence_length is "
                                      "trained but never gathered (word2vec.h:521-523, UB in the reference)");
    if (!valid) continue;
    tw += (uint64_t)(b - a);
    for (int64_t i = a; i < b; i++) {
      auto it = cnt.find(tok_keys[i]);
      if (it != cnt.end())
        it->second++;
      else {
        cnt.emplace(tok_keys[i], 1);
        local_keys.insert(tok_keys[i]);
      }
    }
  }
  if (local_keys.size() < 5) return fail(SWPS_E_UNSUPPORTED, "fewer than 5 keys (word2vec_global.h:556 returns)");
  w->train_words = tw;
  w->vocab_keys.assign(local_keys.begin(), local_keys.end());
  std::unordered_map<uint64_t, int32_t> vid;
  vid.reserve(w->vocab_keys.size() * 2);
  w->counts.resize(w->vocab_keys.size());
  for (size_t i = 0; i < w->vocab_keys.size(); i++) {
    if (w->vocab_keys[i] == 0)
      return fail(SWPS_E_UNSUPPORTED, "a vocab key hashes to 0 (the reference redraws such negatives)");
    vid[w->vocab_keys[i]] = (int32_t)i;
    w->counts[i] = cnt[w->vocab_keys[i]];
  }
  const uint64_t nt = tok_keys.size();
  w->tok.resize(nt);
  w->tok_line.resize(nt);
  for (uint64_t l = 0; l < nl; l++)
    for (int64_t i = w->line_off[l]; i < w->line_off[l + 1]; i++) {
      auto it = vid.find(tok_keys[i]);
      if (it == vid.end())
        return fail(SWPS_E_UNSUPPORTED, "a word occurs only in lines shorter than min_sentence_length "
                                        "(to_sample reads past word_freq in the reference)");
      w->tok[i] = it->second;
      w->tok_line[i] = (int32_t)l;
    }
  w->ntok = nt;
  w->tok_on_device = false;
  w->loaded = true;
  return SWPS_OK;
}

// gen_unigram_table (word2vec_global.h:467-497) in run-length form: the
// 1e8-entry walk assigns word i the slots [start_i, start_{i+1}); the switch
// to word i+1 happens at the first slot a >= start_i with a/T > d1_i.
void unigram_starts(const uint64_t *keys, const int32_t *counts, size_t V, uint64_t T, std::vector<uint64_t> &starts) {
  std::vector<std::pair<uint64_t, int32_t>> by_key(V);
  for (size_t i = 0; i < V; i++) by_key[i] = {keys[i], counts[i]};
  std::sort(by_key.begin(), by_key.end());
  double pw = 0;
  for (auto &kc : by_key) pw += std::pow(kc.second, 0.75);  // std::map order
  starts.assign(V + 1, T);
  starts[0] = 0;
  double d1 = std::pow(counts[0], 0.75) / (double)pw;
  for (size_t i = 0; i + 1 < V; i++) {
    const uint64_t lo = starts[i];
    auto pred = [&](uint64_t a) { return (int64_t)a / (double)T > d1; };
    uint64_t a = (uint64_t)std::max<double>((double)lo, std::floor(d1 * (double)T));
    if (a > T) a = T;
    while (a > lo && pred(a - 1)) a--;
    while (a < T && !pred(a)) a++;
    if (a >= T) break;  // word i runs to the end; later words get no slots
    starts[i + 1] = a + 1;
    d1 += std::pow(counts[i + 1], 0.75) / (double)pw;
  }
}

// The per-epoch batch schedule of TrainModelThread(0) (word2vec_global.h:
// 591-651): line 1 trains before the first gather (its gradients are dropped
// by the pull), then a push/gather/pull every `minibatch` lines; the gather
// window is the next minibatch+3 valid lines (3 tasks, `line_count >
// minibatch`); the epoch stops after the line where cur_train_words exceeds
// train_words.
void build_schedule(swps_w2v *w) {
  const uint64_t nl = w->line_off.size() - 1;
  const int B = w->cfg.minibatch;
  w->batches.clear();
  w->allK.clear();
  auto window = [&](uint64_t li) {
    std::vector<int32_t> K;
    int count = 0;
    for (int task = 0; task < 3; task++)
      while (li < nl) {
        const uint64_t l = li++;
        if (!w->line_valid[l]) continue;
        for (int64_t i = w->line_off[l]; i < w->line_off[l + 1]; i++) K.push_back(w->tok[i]);
        if (++count > B) break;
      }
    std::sort(K.begin(), K.end());
    K.erase(std::unique(K.begin(), K.end()), K.end());
    return K;
  };
  auto emit = [&](uint64_t l0, uint64_t l1, const std::vector<int32_t> *K) {
    swps_w2v::Batch b{l0, l1, w->allK.size(), 0};
    if (K) {
      b.U = (uint32_t)K->size();
      w->allK.insert(w->allK.end(), K->begin(), K->end());
    }
    w->batches.push_back(b);
  };
  std::vector<int32_t> K;
  bool haveK = false;
  uint64_t start = 0, cur = 0, line_counter = 0, last = 0;
  for (uint64_t li = 0; li < nl; li++) {
    cur += (uint64_t)(w->line_off[li + 1] - w->line_off[li]);
    line_counter++;
    last = li + 1;
    if (line_counter == 1) {
      emit(start, li + 1, haveK ? &K : nullptr);
      K = window(li + 1);
      haveK = true;
      start = li + 1;
    }
    if (line_counter % (uint64_t)B == 0) {
      emit(start, li + 1, haveK ? &K : nullptr);
      K = window(li + 1);
      start = li + 1;
    }
    if (cur > w->train_words) break;
  }
  emit(start, last, haveK ? &K : nullptr);
  w->max_tok = w->max_U = w->max_lines = 0;
  for (auto &b : w->batches) {
    w->max_tok = std::max<uint64_t>(w->max_tok, (uint64_t)(w->line_off[b.l1] - w->line_off[b.l0]));
    w->max_U = std::max<uint64_t>(w->max_U, b.U);
    w->max_lines = std::max<uint64_t>(w->max_lines, b.l1 - b.l0);
  }
}

// Vose's alias method over weights count^0.75 (the distribution the
// reference's unigram table discretises into table_size slots): entry i =
// {P(keep i) as float bits, alias}; deterministic (stable worklists).
static void build_alias(const int32_t *counts, size_t n, std::vector<uint2> &out) {
  std::vector<double> q(n);
  double sum = 0;
  for (size_t i = 0; i < n; i++) sum += (q[i] = std::pow((double)counts[i], 0.75));
  std::vector<uint32_t> small, large;
  for (size_t i = 0; i < n; i++) {
    q[i] = q[i] * (double)n / sum;
    (q[i] < 1.0 ? small : large).push_back((uint32_t)i);
  }
  const size_t o = out.size();
  out.resize(o + n);
  size_t si = 0, li = 0;
  while (si < small.size() && li < large.size()) {
    const uint32_t sm = small[si++], lg = large[li];
    float pr = (float)q[sm];
    out[o + sm] = make_uint2(__float_as_uint_host(pr), lg);
    q[lg] -= 1.0 - q[sm];
    if (q[lg] < 1.0) {
      li++;
      small.push_back(lg);
    }
  }
  for (; li < large.size(); li++) out[o + large[li]] = make_uint2(__float_as_uint_host(1.0f), large[li]);
  for (; si < small.size(); si++) out[o + small[si]] = make_uint2(__float_as_uint_host(1.0f), small[si]);
}

// word2vec.h:496-538 train_iter with nthreads = 1: gather_keys reads the next
// B+1 valid lines (word2vec.h:323-377; counts into a std::map, every word
// into _num_words), fewer than 5 keys ends the epoch, then B+1 lines (valid or
// not) are trained from the same position.  The batch's key set is its
// std::map key order; its unigram table (run starts) follows that order.
int build_schedule_mb(swps_w2v *w) {
  const uint64_t nl = w->line_off.size() - 1;
  const int B = w->cfg.minibatch;
  w->batches.clear();
  w->allK.clear();
  w->allUK.clear();
  w->bstarts.clear();
  w->alias.clear();
  w->bcnt_tok.assign(w->tok.size(), 0);
  std::map<int32_t, int32_t> freq_vid;  // counts per vid, then re-ordered by key
  uint64_t p = 0;
  std::vector<std::pair<uint64_t, int32_t>> kv;  // (key, vid)
  std::unordered_map<int32_t, int32_t> cnt_of;
  while (true) {
    cnt_of.clear();
    uint64_t G = 0;
    int count = 0;
    for (uint64_t q = p; q < nl;) {
      const uint64_t l = q++;
      if (!w->line_valid[l]) continue;
      for (int64_t i = w->line_off[l]; i < w->line_off[l + 1]; i++) {
        cnt_of[w->tok[i]]++;
        G++;
      }
      if (++count > B) break;
    }
    if (cnt_of.size() < 5) {
      w->gather_end = G;
      break;
    }
    swps_w2v::Batch b{p, std::min<uint64_t>(nl, p + (uint64_t)B + 1), w->allK.size(), (uint32_t)cnt_of.size(),
                      w->bstarts.size(), G};
    kv.clear();
    for (auto &c : cnt_of) kv.push_back({w->vocab_keys[c.first], c.first});
    std::sort(kv.begin(), kv.end());
    std::vector<uint64_t> keys(kv.size());
    std::vector<int32_t> cnts(kv.size());
    for (size_t i = 0; i < kv.size(); i++) {
      keys[i] = kv[i].first;
      cnts[i] = cnt_of[kv[i].second];
      w->allUK.push_back(kv[i].second);
      w->allK.push_back(kv[i].second);
    }
    std::vector<uint64_t> st;
    unigram_starts(keys.data(), cnts.data(), keys.size(), w->cfg.unigram_size, st);
    w->bstarts.insert(w->bstarts.end(), st.begin(), st.end());
    if (w->cfg.sampler == SWPS_SAMPLER_ALIAS) build_alias(cnts.data(), cnts.size(), w->alias);
    for (uint64_t l = b.l0; l < b.l1; l++)
      for (int64_t i = w->line_off[l]; i < w->line_off[l + 1]; i++) {
        auto it = cnt_of.find(w->tok[i]);
        if (it == cnt_of.end())
          return fail(SWPS_E_UNSUPPORTED, "a trained word is outside its minibatch's gathered vocab "
                                          "(to_sample reads past word_freq in the reference)");
        w->bcnt_tok[i] = it->second;
      }
    w->batches.push_back(b);
    p = b.l1;
  }
  if (w->batches.empty()) return fail(SWPS_E_UNSUPPORTED, "no minibatch with 5 keys (word2vec.h:532 breaks)");
  w->max_tok = w->max_U = w->max_lines = 0;
  for (auto &b : w->batches) {
    w->max_tok = std::max<uint64_t>(w->max_tok, (uint64_t)(w->line_off[b.l1] - w->line_off[b.l0]));
    w->max_U = std::max<uint64_t>(w->max_U, b.U);
    w->max_lines = std::max<uint64_t>(w->max_lines, b.l1 - b.l0);
  }
  return SWPS_OK;
}

static int tok_fingerprint(swps_w2v *w) {
  DevMem d;
  SWPS_TRY(d.ensure(8));
  SWPS_HIP(hipMemsetAsync(d.p, 0, 8, w->s));
  if (w->ntok) k_tok_fp<<<1024, 256, 0, w->s>>>(w->d_tok.as<int32_t>(), w->ntok, d.as<unsigned long long>());
  SWPS_HIP(hipGetLastError());
  uint64_t h = 0;
  SWPS_HIP(hipMemcpyAsync(&h, d.p, 8, hipMemcpyDeviceToHost, w->s));
  SWPS_HIP(hipStreamSynchronize(w->s));
  w->tok_fp = h ^ w->ntok;
  return SWPS_OK;
}

int token_keys_gpu(swps_w2v *w, const uint32_t *word_ids, uint64_t ntok, const uint64_t *word_keys, uint64_t nwords,
                   DevMem &d_keys) {
  DevMem d_ids, d_wk, d_bad;
  SWPS_TRY(d_ids.ensure(std::max<uint64_t>(ntok, 1) * 4));
  SWPS_TRY(d_wk.ensure(std::max<uint64_t>(nwords, 1) * 8));
  SWPS_TRY(d_keys.ensure(std::max<uint64_t>(ntok, 1) * 8));
  SWPS_TRY(d_bad.ensure(4));
  if (ntok) SWPS_HIP(hipMemcpyAsync(d_ids.p, word_ids, ntok * 4, hipMemcpyHostToDevice, w->s));
  if (nwords) SWPS_HIP(hipMemcpyAsync(d_wk.p, word_keys, nwords * 8, hipMemcpyHostToDevice, w->s));
  SWPS_HIP(hipMemsetAsync(d_bad.p, 0, 4, w->s));
  if (ntok)
    k_gather_keys<<<nblk(ntok), 256, 0, w->s>>>(d_ids.as<uint32_t>(), ntok, d_wk.as<uint64_t>(), nwords,
                                                 d_keys.as<uint64_t>(), d_bad.as<uint32_t>());
  SWPS_HIP(hipGetLastError());
  uint32_t bad = 0;
  SWPS_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, w->s));
  SWPS_HIP(hipStreamSynchronize(w->s));
  if (bad) return fail(SWPS_E_CFG, "word id out of range");
  return SWPS_OK;
}

// Vocab + tokens from device keys [ntok] (consumed) and host line offsets.
int ingest_gpu(swps_w2v *w, DevMem &d_keys, uint64_t nt, std::vector<int64_t> &&line_off) {
  hipStream_t s = w->s;
  const uint64_t nl = line_off.size() - 1;
  if (nt >= (1ULL << 32)) return fail(SWPS_E_UNSUPPORTED, "more than 2^32 tokens per rank");
  w->line_off = std::move(line_off);
  w->line_valid.assign(nl, 0);
  uint64_t tw = 0;
  for (uint64_t l = 0; l < nl; l++) {
    const int64_t len = w->line_off[l + 1] - w->line_off[l];
    w->line_valid[l] = len >= w->cfg.min_sentence_length;
    if (w->line_valid[l]) tw += (uint64_t)len;
  }
  SWPS_TRY(upload(w->d_line_off, w->line_off, s));
  SWPS_TRY(w->d_tok.ensure(std::max<uint64_t>(nt, 1) * 4));
  SWPS_TRY(w->d_tok_line.ensure(std::max<uint64_t>(nt, 1) * 4));
  DevMem pos, ks, ps, head, rid1, valid, vscan, tmp;
  SWPS_TRY(pos.ensure(std::max<uint64_t>(nt, 1) * 4));
  SWPS_TRY(ks.ensure(std::max<uint64_t>(nt, 1) * 8));
  SWPS_TRY(ps.ensure(std::max<uint64_t>(nt, 1) * 4));
  if (nt) {
    k_tok_lines<<<nblk(nt), 256, 0, s>>>(w->d_line_off.as<int64_t>(), nl, nt, w->cfg.min_sentence_length,
                                          w->d_tok_line.as<int32_t>(), pos.as<uint32_t>());
    SWPS_HIP(hipGetLastError());
    SWPS_TRY(sort_pairs(tmp, d_keys.as<uint64_t>(), ks.as<uint64_t>(), pos.as<uint32_t>(), ps.as<uint32_t>(), nt, 64,
                        s));
    d_keys.release();
    pos.release();
    SWPS_TRY(head.ensure(nt * 4));
    SWPS_TRY(rid1.ensure(nt * 4));
    SWPS_TRY(valid.ensure((nt + 1) * 4));
    SWPS_TRY(vscan.ensure((nt + 1) * 4));
    k_run_heads<<<nblk(nt + 1), 256, 0, s>>>(ks.as<uint64_t>(), ps.as<uint32_t>(), nt, w->d_tok_line.as<int32_t>(),
                                              w->d_line_off.as<int64_t>(), w->cfg.min_sentence_length,
                                              head.as<uint32_t>(), valid.as<uint32_t>());
    SWPS_HIP(hipGetLastError());
    SWPS_TRY(inclusive_scan(head.as<const uint32_t>(), rid1.as<uint32_t>(), nt, tmp, s));
    SWPS_TRY(exclusive_scan(valid.as<const uint32_t>(), vscan.as<uint32_t>(), nt + 1, tmp, s));
  }
  uint32_t nruns = 0;
  if (nt) SWPS_HIP(hipMemcpyAsync(&nruns, rid1.as<uint32_t>() + nt - 1, 4, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  DevMem ukey, cnt, first, rstart;
  SWPS_TRY(ukey.ensure(std::max<uint32_t>(nruns, 1) * 8));
  SWPS_TRY(cnt.ensure(std::max<uint32_t>(nruns, 1) * 4));
  SWPS_TRY(first.ensure(std::max<uint32_t>(nruns, 1) * 4));
  SWPS_TRY(rstart.ensure(std::max<uint32_t>(nruns, 1) * 4));
  if (nt) {
    k_run_starts<<<nblk(nt), 256, 0, s>>>(ks.as<uint64_t>(), head.as<uint32_t>(), rid1.as<uint32_t>(), nt,
                                           ukey.as<uint64_t>(), rstart.as<uint32_t>());
    k_run_stats<<<nblk(nruns), 256, 0, s>>>(rstart.as<uint32_t>(), nruns, nt, vscan.as<uint32_t>(),
                                             valid.as<uint32_t>(), ps.as<uint32_t>(), cnt.as<uint32_t>(),
                                             first.as<uint32_t>());
    SWPS_HIP(hipGetLastError());
  }
  ks.release();
  head.release();
  std::vector<uint64_t> hk(nruns);
  std::vector<uint32_t> hc(nruns), hf(nruns);
  if (nruns) {
    SWPS_HIP(hipMemcpyAsync(hk.data(), ukey.p, nruns * 8ULL, hipMemcpyDeviceToHost, s));
    SWPS_HIP(hipMemcpyAsync(hc.data(), cnt.p, nruns * 4ULL, hipMemcpyDeviceToHost, s));
    SWPS_HIP(hipMemcpyAsync(hf.data(), first.p, nruns * 4ULL, hipMemcpyDeviceToHost, s));
  }
  SWPS_HIP(hipStreamSynchronize(s));
  // _local_keys: std::unordered_set filled in first-occurrence order over the
  // valid lines; its iteration order is the vid order (ingest() above)
  std::vector<uint32_t> order;
  order.reserve(nruns);
  for (uint32_t r = 0; r < nruns; r++) {
    if (hc[r] == 0)
      return fail(SWPS_E_UNSUPPORTED, "a word occurs only in lines shorter than min_sentence_length "
                                      "(to_sample reads past word_freq in the reference)");
    order.push_back(r);
  }
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hf[a] < hf[b]; });
  std::unordered_set<uint64_t> local_keys;
  for (uint32_t r : order) local_keys.insert(hk[r]);
  if (local_keys.size() < 5) return fail(SWPS_E_UNSUPPORTED, "fewer than 5 keys (word2vec_global.h:556 returns)");
  w->train_words = tw;
  w->vocab_keys.assign(local_keys.begin(), local_keys.end());
  const uint64_t V = w->vocab_keys.size();
  std::vector<std::pair<uint64_t, int32_t>> kv(V);
  for (uint64_t i = 0; i < V; i++) {
    if (w->vocab_keys[i] == 0)
      return fail(SWPS_E_UNSUPPORTED, "a vocab key hashes to 0 (the reference redraws such negatives)");
    kv[i] = {w->vocab_keys[i], (int32_t)i};
  }
  std::sort(kv.begin(), kv.end());  // runs are in ascending key order too
  std::vector<int32_t> vid_of_run(nruns);
  w->counts.assign(V, 0);
  for (uint32_t r = 0; r < nruns; r++) {
    vid_of_run[r] = kv[r].second;
    w->counts[kv[r].second] = (int32_t)hc[r];
  }
  DevMem dv;
  SWPS_TRY(upload(dv, vid_of_run, s));
  if (nt) {
    k_tok_vid<<<nblk(nt), 256, 0, s>>>(ps.as<uint32_t>(), rid1.as<uint32_t>(), nt, dv.as<int32_t>(),
                                        w->d_tok.as<int32_t>());
    SWPS_HIP(hipGetLastError());
  }
  SWPS_HIP(hipStreamSynchronize(s));
  w->tok.clear();
  w->tok_line.clear();
  w->ntok = nt;
  w->tok_on_device = true;
  w->loaded = true;
  return SWPS_OK;
}

// build_schedule (above) with the windows' key sets made on the device
int schedule_gpu(swps_w2v *w) {
  hipStream_t s = w->s;
  const uint64_t nl = w->line_off.size() - 1;
  const int B = w->cfg.minibatch;
  w->batches.clear();
  std::vector<int64_t> ta;     // window token start per batch (batches without a key set: empty)
  std::vector<uint64_t> eoff;  // window element offsets
  eoff.push_back(0);
  auto window_end = [&](uint64_t li) {  // the line after the B+3-valid-line window from li
    int count = 0;
    for (int task = 0; task < 3; task++)
      while (li < nl) {
        const uint64_t l = li++;
        if (!w->line_valid[l]) continue;
        if (++count > B) break;
      }
    return li;
  };
  uint64_t wa = 0, we = 0;
  bool haveK = false;
  auto emit = [&](uint64_t l0, uint64_t l1, bool withK) {
    w->batches.push_back(swps_w2v::Batch{l0, l1, 0, 0});
    const int64_t a = withK ? w->line_off[wa] : 0, e = withK ? w->line_off[we] : 0;
    ta.push_back(a);
    eoff.push_back(eoff.back() + (uint64_t)(e - a));
  };
  uint64_t start = 0, cur = 0, line_counter = 0, last = 0;
  for (uint64_t li = 0; li < nl; li++) {
    cur += (uint64_t)(w->line_off[li + 1] - w->line_off[li]);
    line_counter++;
    last = li + 1;
    if (line_counter == 1) {
      emit(start, li + 1, haveK);
      wa = li + 1;
      we = window_end(li + 1);
      haveK = true;
      start = li + 1;
    }
    if (line_counter % (uint64_t)B == 0) {
      emit(start, li + 1, haveK);
      wa = li + 1;
      we = window_end(li + 1);
      start = li + 1;
    }
    if (cur > w->train_words) break;
  }
  emit(start, last, haveK);
  const uint32_t nb = (uint32_t)w->batches.size();
  const uint64_t E = eoff.back();
  DevMem d_eoff, d_ta, d_valid, keys, keys_s, flags, at, uk, tmp, kofs;
  SWPS_TRY(upload(d_eoff, eoff, s));
  SWPS_TRY(upload(d_ta, ta, s));
  SWPS_TRY(upload(d_valid, w->line_valid, s));
  uint64_t nu = 0;
  if (E) {
    SWPS_TRY(keys.ensure(E * 8));
    SWPS_TRY(keys_s.ensure(E * 8));
    k_sched_keys<<<nblk(E), 256, 0, s>>>(d_eoff.as<uint64_t>(), d_ta.as<int64_t>(), nb, E, w->d_tok.as<int32_t>(),
                                          w->d_tok_line.as<int32_t>(), d_valid.as<uint8_t>(), keys.as<uint64_t>());
    SWPS_HIP(hipGetLastError());
    SWPS_TRY(sort_keys(tmp, keys.as<uint64_t>(), keys_s.as<uint64_t>(), E, 64, s));
    keys.release();
    SWPS_TRY(flags.ensure((E + 1) * 4));
    SWPS_TRY(at.ensure((E + 1) * 4));
    k_uniq_flags<<<nblk(E), 256, 0, s>>>(keys_s.as<uint64_t>(), E, flags.as<uint32_t>());
    SWPS_HIP(hipMemsetAsync(flags.as<uint32_t>() + E, 0, 4, s));
    SWPS_TRY(exclusive_scan(flags.as<const uint32_t>(), at.as<uint32_t>(), E + 1, tmp, s));
    uint32_t n32 = 0;
    SWPS_HIP(hipMemcpyAsync(&n32, at.as<uint32_t>() + E, 4, hipMemcpyDeviceToHost, s));
    SWPS_HIP(hipStreamSynchronize(s));
    nu = n32;
    SWPS_TRY(uk.ensure(std::max<uint64_t>(nu, 1) * 8));
    SWPS_TRY(w->d_K.ensure(std::max<uint64_t>(nu, 1) * 4));
    k_uniq_scatter<<<nblk(E), 256, 0, s>>>(keys_s.as<uint64_t>(), flags.as<uint32_t>(), at.as<uint32_t>(), E,
                                            uk.as<uint64_t>(), w->d_K.as<int32_t>());
    SWPS_HIP(hipGetLastError());
  } else {
    SWPS_TRY(w->d_K.ensure(4));
    SWPS_TRY(uk.ensure(8));
  }
  SWPS_TRY(kofs.ensure((nb + 1ULL) * 8));
  k_batch_kofs<<<nblk(nb + 1ULL), 256, 0, s>>>(uk.as<uint64_t>(), nu, nb, kofs.as<uint64_t>());
  SWPS_HIP(hipGetLastError());
  std::vector<uint64_t> hk(nb + 1);
  SWPS_HIP(hipMemcpyAsync(hk.data(), kofs.p, (nb + 1ULL) * 8, hipMemcpyDeviceToHost, s));
  w->allK.resize(nu);
  if (nu) SWPS_HIP(hipMemcpyAsync(w->allK.data(), w->d_K.p, nu * 4, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  w->max_tok = w->max_U = w->max_lines = 0;
  for (uint32_t b = 0; b < nb; b++) {
    auto &bt = w->batches[b];
    bt.kofs = hk[b];
    bt.U = (uint32_t)(hk[b + 1] - hk[b]);
    w->max_tok = std::max<uint64_t>(w->max_tok, (uint64_t)(w->line_off[bt.l1] - w->line_off[bt.l0]));
    w->max_U = std::max<uint64_t>(w->max_U, bt.U);
    w->max_lines = std::max<uint64_t>(w->max_lines, bt.l1 - bt.l0);
  }
  return SWPS_OK;
}

// text file -> device keys + line offsets (load_text's split on ' ' and '\n'
// only; a file holding a NUL byte takes the host path, whose lines end at
// their first NUL like the reference's std::string(cline))
int tokenize_gpu(swps_w2v *w, const std::vector<char> &text, DevMem &d_keys, uint64_t &nt,
                 std::vector<int64_t> &line_off) {
  hipStream_t s = w->s;
  const uint64_t nb = text.size();
  DevMem d_text, st, nlf, tix, lix, tstart, d_off, tmp;
  SWPS_TRY(d_text.ensure(std::max<uint64_t>(nb, 1)));
  if (nb) SWPS_HIP(hipMemcpyAsync(d_text.p, text.data(), nb, hipMemcpyHostToDevice, s));
  SWPS_TRY(st.ensure((nb + 1) * 4));
  SWPS_TRY(nlf.ensure((nb + 1) * 4));
  SWPS_TRY(tix.ensure((nb + 1) * 4));
  SWPS_TRY(lix.ensure((nb + 1) * 4));
  k_text_flags<<<nblk(nb + 1), 256, 0, s>>>(d_text.as<char>(), nb, st.as<uint32_t>(), nlf.as<uint32_t>());
  SWPS_HIP(hipGetLastError());
  SWPS_TRY(exclusive_scan(st.as<const uint32_t>(), tix.as<uint32_t>(), nb + 1, tmp, s));
  SWPS_TRY(exclusive_scan(nlf.as<const uint32_t>(), lix.as<uint32_t>(), nb + 1, tmp, s));
  uint32_t tot[2];
  SWPS_HIP(hipMemcpyAsync(&tot[0], tix.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipMemcpyAsync(&tot[1], lix.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  nt = tot[0];
  const uint64_t nnl = tot[1];
  const uint64_t nlines = nnl + ((nb && text[nb - 1] != '\n') ? 1 : 0);
  SWPS_TRY(tstart.ensure(std::max<uint64_t>(nt, 1) * 8));
  SWPS_TRY(d_off.ensure((nlines + 2) * 8));
  SWPS_HIP(hipMemsetAsync(d_off.p, 0, 8, s));
  if (nb)
    k_text_index<<<nblk(nb), 256, 0, s>>>(d_text.as<char>(), nb, st.as<uint32_t>(), tix.as<uint32_t>(),
                                           lix.as<uint32_t>(), tstart.as<uint64_t>(), d_off.as<int64_t>());
  SWPS_HIP(hipGetLastError());
  SWPS_TRY(d_keys.ensure(std::max<uint64_t>(nt, 1) * 8));
  if (nt)
    k_text_keys<<<nblk(nt), 256, 0, s>>>(d_text.as<char>(), nb, tstart.as<uint64_t>(), nt,
                                          w->cfg.key_mode == SWPS_KEY_ATOI, d_keys.as<uint64_t>());
  SWPS_HIP(hipGetLastError());
  line_off.assign(nlines + 1, 0);
  if (nnl) SWPS_HIP(hipMemcpyAsync(line_off.data(), d_off.p, (nnl + 1) * 8, hipMemcpyDeviceToHost, s));
  SWPS_HIP(hipStreamSynchronize(s));
  line_off[nlines] = (int64_t)nt;  // a last line without '\n'
  return SWPS_OK;
}

int upload_corpus(swps_w2v *w) {
  hipStream_t s = w->s;
  const uint64_t V = w->vocab_keys.size();
  if (!w->tok_on_device) {
    SWPS_TRY(upload(w->d_tok, w->tok, s));
    SWPS_TRY(upload(w->d_tok_line, w->tok_line, s));
    SWPS_TRY(upload(w->d_K, w->allK, s));
  }
  SWPS_TRY(upload(w->d_line_off, w->line_off, s));
  SWPS_TRY(tok_fingerprint(w));
  std::vector<int64_t> btok;  // token offset of every batch start + the epoch end
  for (auto &b : w->batches) btok.push_back(w->line_off[b.l0]);
  btok.push_back(w->line_off[w->batches.back().l1]);
  SWPS_TRY(upload(w->d_btok, btok, s));
  // subsampling thresholds (word2vec_global.h:728-729), computed on the host
  std::vector<float> ran(V);
  for (uint64_t i = 0; i < V; i++) {
    float freq = float(w->counts[i]) / (float)w->train_words;
    ran[i] = (float)(1 - std::sqrt((double)(w->cfg.sample / freq)));
  }
  SWPS_TRY(upload(w->d_ran, ran, s));
  // ExpTable (word2vec_global.h:252-258)
  std::vector<float> ex(1000);
  for (int i = 0; i < 1000; i++) {
    float x = (i / (float)1000 * 2 - 1) * 6;
    float e = (float)std::exp((double)x);
    ex[i] = e / (e + 1);
  }
  SWPS_TRY(upload(w->d_exptab, ex, s));
  if (w->cfg.sampler == SWPS_SAMPLER_ALIAS) {
    if (!w->cfg.minibatch_vocab) {
      w->alias.clear();
      build_alias(w->counts.data(), V, w->alias);
    }
    SWPS_TRY(upload(w->d_alias, w->alias, s));
  }
  if (w->cfg.minibatch_vocab) {
    SWPS_TRY(upload(w->d_bstarts, w->bstarts, s));
    SWPS_TRY(upload(w->d_UK, w->allUK, s));
    SWPS_TRY(upload(w->d_bcnt_tok, w->bcnt_tok, s));
    SWPS_TRY(w->d_tw.ensure(w->batches.size() * 4));
  } else if (w->cfg.sampler != SWPS_SAMPLER_ALIAS) {
    std::vector<uint64_t> starts;
    unigram_starts(w->vocab_keys.data(), w->counts.data(), V, w->cfg.unigram_size, starts);
    SWPS_TRY(upload(w->d_starts, starts, s));
    SWPS_TRY(w->d_unigram.ensure(w->cfg.unigram_size * 4));
    k_build_unigram<<<4096, 256, 0, s>>>(w->d_starts.as<uint64_t>(), (uint32_t)V, w->cfg.unigram_size,
                                         w->d_unigram.as<int32_t>());
    SWPS_HIP(hipGetLastError());
    const uint64_t nb1 = ((w->cfg.unigram_size - 1) >> kUShift) + 2;
    SWPS_TRY(w->d_uidx.ensure(nb1 * 4));
    k_build_uidx<<<nblk(nb1), 256, 0, s>>>(w->d_starts.as<uint64_t>(), (uint32_t)V, kUShift, nb1,
                                           w->d_uidx.as<int32_t>());
    SWPS_HIP(hipGetLastError());
  }
  const size_t es = w->f64 ? 8 : 4;
  w->cs = row_ld(w->D, es, w->cache_pad);
  SWPS_TRY(w->d_cache_h.ensure(V * w->cs * es));
  SWPS_TRY(w->d_cache_v.ensure(V * w->cs * es));
  SWPS_TRY(w->d_local.ensure(V * 4));
  SWPS_HIP(hipMemsetAsync(w->d_local.p, 0xFF, V * 4, s));
  SWPS_TRY(w->d_vid_row.ensure(V * 4));
  SWPS_HIP(hipStreamSynchronize(s));  // host vectors above go out of scope
  return SWPS_OK;
}

}  // namespace swps
