// The word2vec context shared by its translation units: swps_w2v.hip (C ABI,
// sharded entry points, snapshots), swps_w2v_ingest.hip (corpus, vocab, batch
// schedule), swps_w2v_prep.hip (epoch plan, records, inverted index) and
// swps_w2v_learn.hip (pull, forward, gradient sums, push).  Kernels and their
// argument structs stay private to the unit that launches them; what crosses
// units is declared here.
#pragma once
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include "swps_internal.h"

namespace swps {

// forward slot entry tag: a table row index (not a worker-cache vid); see slot_row
constexpr int32_t kTabRow = 0x40000000;
constexpr int kUShift = 10;  // unigram coarse index: 1024 slots per bucket

constexpr int kBfpMaxD = 512;
inline int bfp_ld(int D, int RB) { return (D + RB * D / 4 + 1 + 31) / 32 * 32; }  // floats per BFP row
// (NCH, NT) lane layout of the BFP-mode kernels for dim D (swps_w2v_bfp.h), as 10*NCH + NT
inline int bfp_shape(int D) {
  const int nch = D / 256, rem = D % 256;
  if (rem == 0) return 10 * nch;
  if (rem <= 128) return 10 * nch + (rem + 63) / 64;
  return 10 * (nch + 1);
}
// g_0..g_N of a position ride in its neu1 row, in the N + 1 floats after the row scale, when the
// row's zero pad holds them (bfp_ld unchanged): N + 1 then, else 0 (the readers gather pg)
inline int bfp_row_g(int D, int RB, int N) { return D + RB * D / 4 + 1 + N + 1 <= bfp_ld(D, RB) ? N + 1 : 0; }

// ---- per-kernel HIP-event timing ----------------------------------------
enum { KT_KEEP = 0, KT_FWD, KT_SORT, KT_GATHER, KT_PUSH, KT_PULL, KT_REC, KT_N };

// neu1/neu1e row stride: D elements rounded up to whole 128-B cache lines, so
// the forward writes and the gather reads full lines only (1200-B fp32 rows at
// D = 300 straddled 10-11 lines: PMC showed 28 % extra forward write bytes).
inline int row_ld(int D, size_t es, bool pad = true) {
  const int q = pad ? (int)(128 / es) : 1;
  return (D + q - 1) / q * q;
}

// fp64 intermediates (parity mode): neu1/neu1e, partials and the push payload in fp64
inline bool inter64(const swps_w2v_cfg &c) { return c.fp64_intermediates == SWPS_INTER_FP64; }

struct Timer {
  bool on = false;
  std::vector<hipEvent_t> pool;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
  double ms[KT_N] = {0};
  uint64_t cnt[KT_N] = {0};
  hipEvent_t get() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
  hipEvent_t begin(hipStream_t s) {
    if (!on) return nullptr;
    hipEvent_t e = get();
    (void)hipEventRecord(e, s);
    return e;
  }
  void end(int k, hipEvent_t b, hipStream_t s) {
    if (!on || !b) return;
    hipEvent_t e = get();
    (void)hipEventRecord(e, s);
    pending.push_back({k, {b, e}});
  }
  // a pair for hipExtLaunchKernelGGL: stamped by the GPU at the kernels' own start / end (no stream
  // gaps in the time, as rocprof measures it); ext_end registers it in place of begin / end
  hipEvent_t ext() { return on ? get() : nullptr; }
  void ext_end(int k, hipEvent_t b, hipEvent_t e) {
    if (b && e) pending.push_back({k, {b, e}});
  }
  void drop(hipEvent_t e) {  // an event begin() recorded that ext stamps replace
    if (e) pool.push_back(e);
  }
  void resolve() {  // caller has synchronized the stream
    for (auto &q : pending) {
      float t = 0;
      (void)hipEventElapsedTime(&t, q.second.first, q.second.second);
      ms[q.first] += t;
      cnt[q.first]++;
      pool.push_back(q.second.first);
      pool.push_back(q.second.second);
    }
    pending.clear();
  }
  ~Timer() {
    for (auto &q : pending) {
      (void)hipEventDestroy(q.second.first);
      (void)hipEventDestroy(q.second.second);
    }
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};

}  // namespace swps

struct swps_w2v {
  using DevMem = swps::DevMem;
  using Timer = swps::Timer;
  swps_table *t = nullptr;
  swps_w2v_cfg cfg{};
  int D = 0, W = 0, N = 0, NCH = 1;
  bool f64 = false;
  bool tail = false;  // fast mode: FSlice kernels (D = 256*NCH + tail, 0 < tail <= 64)
  bool bfp = false;  // fp32 table, fp64_intermediates = SWPS_INTER_BFP40 / _BFP32: the BFP-row kernels (swps_w2v_bfp.h)
  int bfp_rb = 0;    // ... with an int8 residual per element (BFP40: 1) or not (BFP32: 0)
  int xcd_order = 1;  // forward blocks in XCD-contiguous order (SWPS_XCD_ORDER=0 turns it off for A/B timing)
  int push_t = 1;     // fast mode: k_push_t (SWPS_PUSH_T=0: k_push, for A/B timing)
  int push_wpe = 0;  // SWPS_PUSH_WPE: 0 = by batch size, 4 / 1 = k_push_b<1,1,0> at 4 waves per SIMD or not
  int push_unr = 4;  // k_push_b<1,1,0>'s record rows in flight: 4 (SWPS_PUSH_UNR8=1: 8, the previous default)
  // BFP modes: g rides in the neu1 row where its pad holds it: -1 = batches of at least 65536 keys,
  // 0 = never (the pg gather), 1 = at any size (SWPS_ROW_G; A/B, tests)
  int row_g = -1;
  uint32_t gather_grid = 65536;  // k_gather_t / k_combine grid cap in blocks (SWPS_GATHER_GRID; A/B: 2048..65536 -> 65536 best)
  bool cache_pad = true;  // worker-cache rows padded to 128 B (SWPS_CACHE_PAD=0: D-strided, for A/B timing)
  int cs = 0;              // worker-cache row stride in elements (set with the cache allocation)
  bool uni_index = true;  // negatives via the coarse-indexed run-length table (SWPS_UNI_INDEX=0: the 1e8-slot table)
  bool seg4 = true;       // k_seg_bounds4: 4 sorted records per thread (SWPS_SEG4=0: one, A/B)
  bool tok_local = true;  // k_tok_local + k_records_t's per-token lookups (SWPS_TOK_LOCAL=0: off, A/B)
  // k_item_desc's runs by k_item_heads + max-scan instead of a binary search (SWPS_ITEM_HEADS=1; off:
  // same-box A/B, round 4, 2 reps: B = 5000 unchanged, B = 100 3.01e8 -> 2.92e8 words/s — four more
  // launches on the prep stream)
  bool item_heads = false;
  DevMem d_irun;           // its item -> run map
  DevMem d_tloc;          // its per-token {local, source} of the batch being prepped
  bool row_pad = true;  // neu1/neu1e rows padded to 128 B (SWPS_ROW_PAD=0: D-strided, for A/B timing)
  hipStream_t s = nullptr;
  // host corpus / vocab
  std::vector<int32_t> tok;       // host ingest only (the GPU ingest leaves tokens in d_tok)
  std::vector<int32_t> tok_line;
  uint64_t ntok = 0;              // corpus tokens
  uint64_t tok_fp = 0;            // device-computed fingerprint of d_tok (checkpoint corpus check)
  bool tok_on_device = false;     // d_tok / d_tok_line / d_K were built by the GPU ingest
  std::vector<int64_t> line_off;
  std::vector<uint8_t> line_valid;
  std::vector<uint64_t> vocab_keys;
  std::vector<int32_t> counts;
  uint64_t train_words = 0;
  bool loaded = false, inited = false;
  bool pinned = false;  // table_pin held (from the completed init to destroy)
  // schedule (identical every epoch)
  struct Batch {
    uint64_t l0, l1, kofs;
    uint32_t U;
    uint64_t sofs = 0;    // minibatch-vocab mode: offset of the batch's table run starts
    uint64_t gathered = 0;  // words its gather_keys counted into _num_words
  };
  std::vector<Batch> batches;
  std::vector<int32_t> allK;
  uint64_t max_tok = 0, max_U = 0, max_lines = 0;
  uint64_t cursor = 0;  // next global batch index
  // device
  DevMem d_uidx;
  DevMem d_tok, d_tok_line, d_line_off, d_ran, d_exptab, d_unigram, d_starts, d_vid_row, d_cache_h, d_cache_v,
      d_local, d_K;
  DevMem d_btok, d_bounds;
  DevMem d_kflag, d_kscan, d_ldraw, d_ldoff, d_pos_tok, d_rec, d_neu1, d_neu1e, d_pkeys, d_pvals, d_pkeys_s,
      d_pvals_s, d_pg, d_seg, d_icnt, d_ioff, d_partial, d_desc, d_tmp, d_trace, d_rows_touched, d_gstats;
  swps::ShardDriver *drv = nullptr;  // swps_w2v_shard_comm: the library drives the exchange
  bool rec_generic = false;          // SWPS_REC_GENERIC=1: the generic k_records (A/B, tests)
  DevMem d_lead;  // hot-group leaders of the batch's gather items: [0] = count, then item indices
  DevMem d_multi;  // items of multi-chunk runs (k_gather_t's work when the push is fused): [0] = count, then items
  DevMem d_krow;   // per batch key: its shard row (vid_row[K[u]]), for k_push_thp
  int fused_push = 1;  // fast mode: k_push_thp sums single-chunk runs itself (SWPS_FUSED_PUSH=0: k_gather_t + k_push_t)
  uint32_t push_grid = 0;  // k_push_thp grid cap in blocks (SWPS_PUSH_GRID; 0 = by batch size)
  // k_combine pre-sums hot runs' partials in groups of kGroup: 1 always, 0 never (the push reads every
  // partial), 2 (default) when the batch has at least combine_min records -- measured: -2.6% without it at
  // B = 5000 (21M records), +1.6% at B = 100 (0.4M), where its launch costs more than the re-reads
  int combine = 2;
  uint64_t combine_min = 1ull << 22;
  int full_lines = 1;  // neu1/neu1e and cache-row stores write the row pad as zeros (SWPS_FULL_LINES=0: off; A/B)
  int split_grads = 1;  // sharded learner (world > 1): mean gradients in two owner-half passes (SWPS_SPLIT_GRADS=0: one)
  hipEvent_t ev_half = nullptr;  // recorded between the two passes of the last step
  bool half_ready = false;       // the last step ran the two passes (the driver takes and clears it)
  int split_push = 0;  // SWPS_SPLIT_PUSH: 1 = gather beside the push always, -1 = below 64 k keys, 0 = never
                      // (default: same-box A/B at B = 100 lines 0.321 ms/step in one stream vs 0.349 split)
  hipStream_t s_side = nullptr;
  hipEvent_t ev_fwd = nullptr, ev_gat = nullptr;
  uint32_t multi_chunk = 0;  // SWPS_MULTI_CHUNK: chunk size of multi-chunk runs (1..128; 0 = kChunk)
  int multi_sort = 1;                 // order the multi-chunk items by position (SWPS_MULTI_SORT=0: off; A/B)
  uint64_t multi_sort_min = 65536;    // ... for batches of at least this many kept positions (SWPS_MULTI_SORT_MIN)
  uint64_t *h_small = nullptr;  // pinned readback
  // RNG (utils/random.h:44-47, seed 2008)
  uint64_t lstate = 2008ULL;
  uint64_t fstate = std::numeric_limits<unsigned long>::max() / 2;
  uint64_t lstate_epoch = 0;        // main LCG state at the current epoch's start
  uint64_t fstate_epoch = 0;        // float LCG state at the current epoch's start
  // sharded mode: keys owned by BasicHashFrag node rank+1
  int rank = 0, world = 1, frag_num = 0;
  bool sharded = false;
  std::vector<uint64_t> bcounts;   // [nb][world] keys requested per owner per batch
  std::vector<uint64_t> icounts;   // [world] init request per owner
  std::vector<int32_t> init_order; // vids grouped by owner
  DevMem d_vkeys, d_init_order, d_serve_rows, d_push_rows;
  DevMem d_mark;          // late_mask: a stamp per table row
  // the next step's pull values in two parts (AppOps::install_parts; consumed by that step)
  const uint32_t *pull_rows = nullptr;  // world 1: the slot's shard rows, read in place by the step's install
  struct Parts {
    const void *vals[2] = {nullptr, nullptr};
    const uint32_t *pos[2] = {nullptr, nullptr};
    uint64_t n[2] = {0, 0};
  } parts;
  uint32_t mark_stamp = 0;
  hipStream_t ss = nullptr;  // serve stream (request / serve_pull / serve_push); nullptr = s
  // the library driver's step slot (AppOps::set_slot): the keys served at a slot are the same every
  // epoch, so their row lookups and the push's grouping sort are kept per slot
  int64_t slot = -1;
  struct SlotRows {
    DevMem rows, sorted;
    uint64_t n = 0;
    bool sorted_valid = false;
  };
  std::vector<std::unique_ptr<SlotRows>> slot_rows;
  std::vector<uint32_t> plan_P;     // kept positions per batch of the current epoch
  // minibatch-vocab mode (word2vec.h MiniBatch, w2v_local.cpp)
  std::vector<int32_t> allUK;       // per batch: its vids in std::map key order (offset kofs)
  std::vector<uint64_t> bstarts;    // per batch: U+1 table run starts (offset sofs)
  std::vector<int32_t> bcnt_tok;    // per trained token: its word's count in its batch
  uint64_t gather_end = 0;          // words counted by the epoch's final (< 5 keys) gather
  DevMem d_bstarts, d_UK, d_bcnt_tok, d_tw;
  // SWPS_SAMPLER_ALIAS: alias tables (global: one over the vocab in vid order;
  // minibatch-vocab: one per batch over its map order, offset = batch kofs)
  std::vector<uint2> alias;
  DevMem d_alias;
  // the prepared (parameter-independent) half of the next minibatch
  struct Prepped {
    bool valid = false, records = false, sorted = false, msorted = false;
    uint64_t bi = 0, P = 0, nt = 0, HOFF = 0, M = 0, max_items = 0;
    uint32_t U = 0;
  } pb;
  // overlapped single-GPU driver (train_overlapped): the second set of the
  // parameter-independent per-batch buffers, swapped with the members above,
  // and the stream prep(i+1) runs on while learn(i) runs on s
  static constexpr int kPrepBufs = 15;
  DevMem alt[kPrepBufs];
  bool alt_local_ready = false;
  // train_overlapped: -1 = auto (on for minibatches of at most kOverlapTok tokens: at B = 100 lines the
  // prep chain — records, sort, index: ~12 short latency-bound launches — hides behind the learn, 0.41 ->
  // 0.36 ms/step; at B = 5000 forward and gather already fill every CU and the HBM: 4.25e8 sequential vs
  // 4.24e8 / 4.02e8 overlapped); SWPS_OVERLAP=0/1 forces it
  int overlap = -1;
  hipStream_t s_prep = nullptr;
  hipEvent_t ev_learn = nullptr, ev_prep = nullptr;
  hipEvent_t fwd_event = nullptr;  // learn_batch records it after the forward when set (overlap mode 2)
  DevMem *prep_set[kPrepBufs] = {&d_pos_tok, &d_rec,  &d_pkeys, &d_pvals, &d_pkeys_s, &d_pvals_s, &d_tmp,
                                 &d_seg,     &d_icnt, &d_ioff,  &d_desc,  &d_lead,    &d_multi, &d_krow, &d_local};
  // stats
  uint64_t st_batches = 0, st_kept = 0, st_words = 0, st_pairs = 0, st_pulled = 0, st_pushed = 0;
  uint64_t st_sums = 0, st_fused = 0, st_fused_g = 0, st_split = 0;  // batches with gradient sums; of those, fused in-place
                                                       // pushes / fused mean-gradient (sharded) pushes
  // negative trace
  uint64_t trace_cap = 0;
  std::vector<int64_t> trace;
  Timer timer;
};

namespace swps {

constexpr uint32_t kChunk = 128;  // a (key, kind) run of at most kChunk records is one item
// chunk size of the longer runs: kChunk (SWPS_MULTI_CHUNK sets 1..128 for A/B: 32 and 16 at
// B = 100 lines were 4 % and 7 % slower — more partials and second-level groups, no latency win)
inline uint32_t multi_chunk(const swps_w2v *w, uint64_t) { return w->multi_chunk ? w->multi_chunk : kChunk; }
constexpr uint64_t kOverlapTok = 1000000;  // auto-overlap threshold (tokens per minibatch)

// ---- swps_w2v_ingest.hip: corpus -> vocab, tokens, batch schedule, device tables ----
int check_cfg(swps_w2v *w);
int ingest(swps_w2v *w, const std::vector<uint64_t> &tok_keys, std::vector<int64_t> &&line_off);
void unigram_starts(const uint64_t *keys, const int32_t *counts, size_t V, uint64_t T, std::vector<uint64_t> &starts);
void build_schedule(swps_w2v *w);
int build_schedule_mb(swps_w2v *w);
int tokenize_gpu(swps_w2v *w, const std::vector<char> &text, DevMem &d_keys, uint64_t &nt,
                 std::vector<int64_t> &line_off);
// host word ids + their keys -> device keys [ntok] (an id >= nwords fails)
int token_keys_gpu(swps_w2v *w, const uint32_t *word_ids, uint64_t ntok, const uint64_t *word_keys, uint64_t nwords,
                   DevMem &d_keys);
int ingest_gpu(swps_w2v *w, DevMem &d_keys, uint64_t nt, std::vector<int64_t> &&line_off);
int schedule_gpu(swps_w2v *w);
int upload_corpus(swps_w2v *w);

// ---- swps_w2v_prep.hip: the parameter-independent half of a minibatch ----
int upload_lcg_constants();  // the kernels' per-bit LCG jump tables (once per context, same values)
int plan_epoch(swps_w2v *w);
int prep_batch(swps_w2v *w);

// ---- swps_w2v_learn.hip: the half that reads and writes parameters ----
// one minibatch in the context's precision: install the pulled values (d_vals: the sharded learner's,
// else none), forward, gradient sums, push (d_grads: the mean gradients go there instead of AdaGrad)
int learn_step(swps_w2v *w, const void *d_vals = nullptr, void *d_grads = nullptr);
int train_overlapped(swps_w2v *w, uint64_t count);
int pull_all(swps_w2v *w);
int rand_init_gpu(swps_w2v *w);
int set_hv(swps_w2v *w, const double *hv);
int install_init(swps_w2v *w, const void *d_vals);  // the sharded first full pull's values, init_order

}  // namespace swps
