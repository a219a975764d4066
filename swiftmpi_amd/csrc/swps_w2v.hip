// word2vec CBOW negative sampling on one MI355X: the reference's
// pull -> learn_instance -> push minibatch loop (apps/word2vec/
// word2vec_global.h:552-731, nthreads = 1 semantics) as a chain of HIP
// kernels over HBM-resident data.
//
// Per minibatch n (trained lines T_n, gathered key set K_n, U = |K_n|):
//   k_pull      cache[vid] <- table row (h, v) for vid in K_n; local[vid] = u
//               (global_pull_access.h:80-101: params[key]=val, grads reset)
//   k_keep      float-LCG subsample test per token, LCG jumped to the
//               token's stream offset (word2vec_global.h:725-731)
//   scans       kept positions per line -> main-LCG draw offset per kept
//               position (1 draw per line + (1+negative) per kept position)
//   k_forward   one wave per kept position: neu1 = sum of context v rows,
//               dots with the positive and the negative h rows (fp64),
//               exp-table sigmoid, neu1e; writes neu1/neu1e rows and one
//               (key, pair index) record per target and per context
//               (word2vec_global.h:663-718)
//   radix sort  records by local key index (stable: position order kept)
//   k_gather    chunked segmented sums  h_grad[k] = sum g*neu1[p],
//               v_grad[k] = sum neu1e[p]  into per-chunk partials (no atomics)
//   k_push      partials summed in chunk order, mean over the counts
//               (word2vec_global.h:122-134), AdaGrad on the table row
//               (word2vec_global.h:176-185)
// Params are read only from the frozen cache during a batch, exactly like the
// reference worker.  Negatives outside K_n read the stale cache and their
// gradients are dropped (the reference resets them at the next pull).
//
// One stage per translation unit (swps_w2v_ctx.h holds the context they
// share): swps_w2v_ingest.hip (corpus, vocab, batch schedule),
// swps_w2v_prep.hip (k_keep, scans, records, radix sort, chunk index),
// swps_w2v_learn.hip (k_pull, forward, gather, push and the minibatch
// drivers).  This file: the C ABI, the sharded entry points and the worker
// checkpoint.
#include <algorithm>
#include <cstdlib>
#include <cstdio>

#include "swps_w2v_ctx.h"

using namespace swps;

namespace {

__global__ void k_vid_keys(const int32_t *__restrict__ K, uint64_t n, const uint64_t *__restrict__ vkeys,
                           uint64_t *__restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = vkeys[K[i]];
}

// owner side of the early / late pull split (AppOps::late_mask): stamp the table rows served
// at one slot, then flag the rows of another slot that carry the stamp
__global__ void k_stamp_rows(const uint32_t *__restrict__ rows, uint64_t n, uint32_t cap, uint32_t stamp,
                             uint32_t *__restrict__ mark) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && rows[i] < cap) mark[rows[i]] = stamp;
}
__global__ void k_flag_rows(const uint32_t *__restrict__ rows, uint64_t n, uint32_t cap, uint32_t stamp,
                            const uint32_t *__restrict__ mark, uint8_t *__restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[i] = rows[i] >= cap || mark[rows[i]] == stamp;  // an unknown row: late (safe)
}

}  // namespace

extern "C" {

int swps_w2v_create(swps_table *t, const swps_w2v_cfg *cfg, swps_w2v **out) {
  if (!t || !cfg || !out) return fail(SWPS_E_CFG, "null argument");
  *out = nullptr;
  if (t->cfg.layout != SWPS_LAYOUT_W2V) return fail(SWPS_E_CFG, "table layout must be SWPS_LAYOUT_W2V");
  SWPS_TRY(check_app_table(t));
  SWPS_HIP(hipSetDevice(t->cfg.device));
  swps_w2v *w = new swps_w2v();
  w->t = t;
  w->cfg = *cfg;
  w->D = t->cfg.dim;
  w->W = cfg->window;
  w->N = cfg->negative;
  w->f64 = t->cfg.dtype == SWPS_F64;
  w->s = t->stream;
  w->timer.on = cfg->profile != 0;
  if (const char *e = getenv("SWPS_XCD_ORDER")) w->xcd_order = atoi(e) != 0;
  if (const char *e = getenv("SWPS_PUSH_T")) w->push_t = atoi(e) != 0;  // A/B timing
  if (const char *e = getenv("SWPS_FUSED_PUSH")) w->fused_push = atoi(e) != 0;  // A/B timing
  if (const char *e = getenv("SWPS_COMBINE")) w->combine = atoi(e);
  if (const char *e = getenv("SWPS_COMBINE_MIN")) w->combine_min = strtoull(e, nullptr, 10);
  if (const char *e = getenv("SWPS_FULL_LINES")) w->full_lines = atoi(e) != 0;
  if (const char *e = getenv("SWPS_SPLIT_PUSH")) w->split_push = atoi(e);
  if (const char *e = getenv("SWPS_SPLIT_GRADS")) w->split_grads = atoi(e) != 0;
  if (const char *e = getenv("SWPS_PUSH_GRID")) w->push_grid = (uint32_t)std::max(0, atoi(e));
  if (const char *e = getenv("SWPS_MULTI_SORT")) w->multi_sort = atoi(e);        // A/B timing
  if (const char *e = getenv("SWPS_MULTI_CHUNK")) w->multi_chunk = (uint32_t)std::min(128, std::max(0, atoi(e)));
  if (const char *e = getenv("SWPS_MULTI_SORT_MIN")) w->multi_sort_min = strtoull(e, nullptr, 10);
  if (const char *e = getenv("SWPS_ROW_PAD")) w->row_pad = atoi(e) != 0;  // A/B timing
  if (const char *e = getenv("SWPS_UNI_INDEX")) w->uni_index = atoi(e) != 0;  // A/B timing
  if (const char *e = getenv("SWPS_SEG4")) w->seg4 = atoi(e) != 0;            // A/B timing
  if (const char *e = getenv("SWPS_TOK_LOCAL")) w->tok_local = atoi(e) != 0;  // A/B timing
  if (const char *e = getenv("SWPS_ITEM_HEADS")) w->item_heads = atoi(e) != 0;  // A/B timing
  if (const char *e = getenv("SWPS_CACHE_PAD")) w->cache_pad = atoi(e) != 0;  // A/B timing
  if (const char *e = getenv("SWPS_OVERLAP")) w->overlap = atoi(e);  // A/B timing
  if (const char *e = getenv("SWPS_REC_GENERIC")) w->rec_generic = atoi(e) != 0;
  if (const char *e = getenv("SWPS_GATHER_GRID")) w->gather_grid = std::max(64, atoi(e));
  if (const char *e = getenv("SWPS_PUSH_WPE")) w->push_wpe = atoi(e);  // A/B: push occupancy
  if (const char *e = getenv("SWPS_PUSH_UNR8")) w->push_unr = atoi(e) ? 8 : 4;  // A/B, tests
  if (const char *e = getenv("SWPS_ROW_G")) w->row_g = atoi(e) != 0;             // A/B, tests
  int rc = check_cfg(w);
  if (!rc && hipHostMalloc((void **)&w->h_small, 64) != hipSuccess) rc = fail(SWPS_E_OOM, "pinned alloc");
  if (!rc) rc = w->d_rows_touched.ensure(16);
  if (!rc && hipMemset(w->d_rows_touched.p, 0, 16) != hipSuccess) rc = fail(SWPS_E_HIP, "memset");
  if (!rc) rc = w->d_gstats.ensure(32);
  if (!rc && hipMemset(w->d_gstats.p, 0, 32) != hipSuccess) rc = fail(SWPS_E_HIP, "memset");
  if (!rc) rc = upload_lcg_constants();
  if (rc) {
    if (w->h_small) (void)hipHostFree(w->h_small);
    delete w;
    return rc;
  }
  *out = w;
  return SWPS_OK;
}

int swps_w2v_destroy(swps_w2v *w) {
  if (!w) return SWPS_OK;
  (void)hipSetDevice(w->t->cfg.device);
  (void)hipStreamSynchronize(w->s);
  if (w->s_prep) {
    (void)hipStreamSynchronize(w->s_prep);
    (void)hipStreamDestroy(w->s_prep);
  }
  if (w->s_side) {
    (void)hipStreamSynchronize(w->s_side);
    (void)hipStreamDestroy(w->s_side);
  }
  if (w->ev_learn) (void)hipEventDestroy(w->ev_learn);
  if (w->ev_prep) (void)hipEventDestroy(w->ev_prep);
  if (w->ev_fwd) (void)hipEventDestroy(w->ev_fwd);
  if (w->ev_half) (void)hipEventDestroy(w->ev_half);
  if (w->ev_gat) (void)hipEventDestroy(w->ev_gat);
  if (w->h_small) (void)hipHostFree(w->h_small);
  if (w->pinned) table_unpin(w->t);
  delete w->drv;
  delete w;
  (void)hipGetLastError();  // leave no sticky error from the calls above
  return SWPS_OK;
}

// LineFileReader + split(" ") + BKDRHash / atoi (word2vec_global.h:215-227)
int swps_w2v_load_text(swps_w2v *w, const char *path) {
  if (!w->cfg.minibatch_vocab && !w->cfg.host_ingest) {  // the GPU ingest (no NUL bytes in the file)
    FILE *f = fopen(path, "rb");
    if (!f) return fail(SWPS_E_IO, std::string("no such file or directory: ") + path);
    std::vector<char> text;
    char chunk[1 << 16];
    size_t k;
    while ((k = fread(chunk, 1, sizeof(chunk), f)) > 0) text.insert(text.end(), chunk, chunk + k);
    fclose(f);
    if (!memchr(text.data(), 0, text.size())) {
      SWPS_HIP(hipSetDevice(w->t->cfg.device));
      DevMem d_keys;
      uint64_t nt = 0;
      std::vector<int64_t> off;
      SWPS_TRY(tokenize_gpu(w, text, d_keys, nt, off));
      std::vector<char>().swap(text);
      SWPS_TRY(ingest_gpu(w, d_keys, nt, std::move(off)));
      SWPS_TRY(schedule_gpu(w));
      return upload_corpus(w);
    }
  }
  FILE *f = fopen(path, "rb");
  if (!f) return fail(SWPS_E_IO, std::string("no such file or directory: ") + path);
  std::vector<uint64_t> keys;
  std::vector<int64_t> off{0};
  char *buf = nullptr;
  size_t cap = 0;
  ssize_t n;
  std::string word;
  while ((n = getdelim(&buf, &cap, '\n', f)) >= 0) {
    if (n >= 1 && buf[n - 1] == '\n') buf[--n] = 0;
    const size_t len = strlen(buf);  // std::string(cline) stops at a NUL
    size_t i = 0;
    while (i < len) {
      while (i < len && buf[i] == ' ') i++;
      if (i >= len) break;
      size_t j = i;
      while (j < len && buf[j] != ' ') j++;
      word.assign(buf + i, j - i);
      keys.push_back(w->cfg.key_mode == SWPS_KEY_ATOI ? (uint64_t)(int64_t)atoi(word.c_str()) : bkdr(word.c_str()));
      i = j;
    }
    off.push_back((int64_t)keys.size());
  }
  free(buf);
  fclose(f);
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  SWPS_TRY(ingest(w, keys, std::move(off)));
  if (w->cfg.minibatch_vocab)
    SWPS_TRY(build_schedule_mb(w));
  else
    build_schedule(w);
  return upload_corpus(w);
}

int swps_w2v_load_tokens(swps_w2v *w, const uint32_t *word_ids, uint64_t ntok, const uint64_t *line_off,
                         uint64_t nlines, const uint64_t *word_keys, uint64_t nwords) {
  if (line_off[0] != 0 || line_off[nlines] != ntok) return fail(SWPS_E_CFG, "line_off must span [0, ntok]");
  std::vector<int64_t> off(line_off, line_off + nlines + 1);
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  if (!w->cfg.minibatch_vocab && !w->cfg.host_ingest) {  // the GPU ingest
    DevMem d_keys;
    SWPS_TRY(token_keys_gpu(w, word_ids, ntok, word_keys, nwords, d_keys));
    SWPS_TRY(ingest_gpu(w, d_keys, ntok, std::move(off)));
    SWPS_TRY(schedule_gpu(w));
    return upload_corpus(w);
  }
  std::vector<uint64_t> keys(ntok);
  for (uint64_t i = 0; i < ntok; i++) {
    if (word_ids[i] >= nwords) return fail(SWPS_E_CFG, "word id out of range");
    keys[i] = word_keys[word_ids[i]];
  }
  SWPS_TRY(ingest(w, keys, std::move(off)));
  if (w->cfg.minibatch_vocab)
    SWPS_TRY(build_schedule_mb(w));
  else
    build_schedule(w);
  return upload_corpus(w);
}

int swps_w2v_corpus(swps_w2v *w, int32_t *vid, int32_t *line, uint64_t cap) {
  if (!w->loaded) return fail(SWPS_E_STATE, "load a corpus first");
  if (cap < w->ntok) return fail(SWPS_E_CFG, "buffer too small");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  if (w->ntok) {
    SWPS_HIP(hipMemcpyAsync(vid, w->d_tok.p, w->ntok * 4, hipMemcpyDeviceToHost, w->s));
    SWPS_HIP(hipMemcpyAsync(line, w->d_tok_line.p, w->ntok * 4, hipMemcpyDeviceToHost, w->s));
  }
  SWPS_HIP(hipStreamSynchronize(w->s));
  return SWPS_OK;
}

int swps_w2v_batch_keys(swps_w2v *w, uint64_t b, int32_t *out, uint64_t cap, uint64_t *n, uint64_t *lines2) {
  if (!w->loaded) return fail(SWPS_E_STATE, "load a corpus first");
  if (b >= w->batches.size()) return fail(SWPS_E_CFG, "no such batch");
  const auto &bt = w->batches[b];
  *n = bt.U;
  if (lines2) {
    lines2[0] = bt.l0;
    lines2[1] = bt.l1;
  }
  if (cap < bt.U) return fail(SWPS_E_CFG, "buffer too small");
  std::copy(w->allK.begin() + bt.kofs, w->allK.begin() + bt.kofs + bt.U, out);
  return SWPS_OK;
}

int swps_w2v_vocab(swps_w2v *w, uint64_t *keys, int32_t *counts, uint64_t cap, uint64_t *n) {
  *n = w->vocab_keys.size();
  if (cap < *n) return fail(SWPS_E_CFG, "buffer too small");
  for (size_t i = 0; i < w->vocab_keys.size(); i++) {
    if (keys) keys[i] = w->vocab_keys[i];
    if (counts) counts[i] = w->counts[i];
  }
  return SWPS_OK;
}

int swps_w2v_info(swps_w2v *w, uint64_t *o) {
  o[0] = w->vocab_keys.size();
  o[1] = w->train_words;
  o[2] = w->line_off.empty() ? 0 : w->line_off.size() - 1;
  o[3] = w->ntok;
  o[4] = w->batches.size();
  o[5] = w->max_tok;
  o[6] = w->lstate;
  o[7] = w->fstate;
  return SWPS_OK;
}

// The first full pull (word2vec_global.h:557-562 -> accessmethod.h:63-70):
// every vocab key misses and gets a fresh WParam.
int swps_w2v_init(swps_w2v *w) {
  if (!w->loaded) return fail(SWPS_E_STATE, "load a corpus first");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  if (w->drv) return w->drv->full_pull();  // the first full pull, over the communicator
  if (w->t->comm)
    return fail(SWPS_E_UNSUPPORTED, "the table is key-sharded (swps_table_route): drive the context with "
                                    "swps_w2v_shard_comm");
  const uint64_t V = w->vocab_keys.size();
  DevMem dk;
  SWPS_TRY(upload(dk, w->vocab_keys, w->s));
  SWPS_TRY(table_find_or_insert(w->t, dk.as<uint64_t>(), V, w->d_vid_row.as<uint32_t>(), w->s));
  if (w->cfg.init_mode == SWPS_W2V_INIT_REF) {
    // Vec::randInit (vec1.h:229-232): (rand()/(float)RAND_MAX - 0.5)/D, h then
    // v per key, keys in _local_keys order, after rand_offset earlier calls —
    // generated on the GPU by jump-ahead (rand_init_gpu)
    SWPS_TRY(rand_init_gpu(w));
  } else {
    SWPS_TRY(pull_all(w));
  }
  table_pin_once(w->t, w->pinned);  // vid_row / slot rows index the shard from here on
  w->inited = true;
  return SWPS_OK;
}

int swps_w2v_train_batches(swps_w2v *w, uint64_t count) {
  if (!w->inited) return fail(SWPS_E_STATE, "call swps_w2v_init first");
  if (w->drv) {
    SWPS_HIP(hipSetDevice(w->t->cfg.device));
    return w->drv->steps(count);  // collective: `count` lockstep steps on every rank
  }
  if (w->sharded) return fail(SWPS_E_STATE, "sharded context: drive it with request / serve_pull / step / serve_push");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  const bool ov = w->overlap > 0 || (w->overlap < 0 && w->max_tok <= kOverlapTok);
  if (ov && count > 1 && !w->cfg.minibatch_vocab && w->trace.size() >= w->trace_cap && !w->pb.valid)
    return train_overlapped(w, count);
  for (uint64_t i = 0; i < count; i++) SWPS_TRY(learn_step(w));
  return SWPS_OK;
}

int swps_w2v_train_epochs(swps_w2v *w, int32_t niters) {
  if (w->drv) {
    if (w->drv->spe && w->drv->cursor % w->drv->spe) return fail(SWPS_E_STATE, "not at an epoch boundary");
    SWPS_TRY(swps_w2v_train_batches(w, (uint64_t)niters * w->drv->spe));
    return swps_w2v_sync(w);
  }
  if (w->cursor % std::max<size_t>(1, w->batches.size()) != 0) return fail(SWPS_E_STATE, "not at an epoch boundary");
  SWPS_TRY(swps_w2v_train_batches(w, (uint64_t)niters * w->batches.size()));
  return swps_w2v_sync(w);
}

int swps_w2v_sync(swps_w2v *w) {
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  if (w->drv) SWPS_TRY(w->drv->sync());
  SWPS_HIP(hipStreamSynchronize(w->s));
  if (w->ss) SWPS_HIP(hipStreamSynchronize(w->ss));
  w->timer.resolve();
  return SWPS_OK;
}

int swps_w2v_stats(swps_w2v *w, uint64_t *o) {
  o[0] = w->st_batches;
  o[1] = w->st_kept;
  o[2] = w->st_words;
  o[3] = w->st_pairs;
  o[4] = w->lstate;
  o[5] = w->fstate;
  o[6] = w->st_pulled;
  o[7] = w->st_pushed;
  uint64_t rt[2] = {0, 0};
  SWPS_HIP(hipStreamSynchronize(w->s));
  SWPS_HIP(hipMemcpy(rt, w->d_rows_touched.p, 16, hipMemcpyDeviceToHost));
  o[8] = rt[0];
  o[9] = rt[1];
  return SWPS_OK;
}

int swps_w2v_gather_stats(swps_w2v *w, uint64_t *out2) {
  SWPS_HIP(hipStreamSynchronize(w->s));
  SWPS_HIP(hipMemcpy(out2, w->d_gstats.p, 16, hipMemcpyDeviceToHost));
  return SWPS_OK;
}

int swps_w2v_sum_stats(swps_w2v *w, uint64_t *out8) {
  SWPS_HIP(hipStreamSynchronize(w->s));
  SWPS_HIP(hipMemcpy(out8, w->d_gstats.p, 32, hipMemcpyDeviceToHost));
  out8[4] = w->st_fused;
  out8[5] = w->st_sums;
  out8[6] = w->st_fused_g;
  out8[7] = w->st_split;
  return SWPS_OK;
}

int swps_w2v_get_params(swps_w2v *w, double *out) {
  SWPS_TRY(swps_w2v_sync(w));
  const uint64_t V = w->vocab_keys.size();
  const int R = 4 * w->D;
  DevMem d;
  const size_t es = w->f64 ? 8 : 4;
  SWPS_TRY(d.ensure(V * R * es));
  SWPS_TRY(table_get_rows(w->t, w->d_vid_row.as<uint32_t>(), V, d.p, w->s));
  std::vector<char> h(V * R * es);
  SWPS_HIP(hipMemcpyAsync(h.data(), d.p, h.size(), hipMemcpyDeviceToHost, w->s));
  SWPS_HIP(hipStreamSynchronize(w->s));
  for (uint64_t i = 0; i < V * R; i++) out[i] = w->f64 ? ((double *)h.data())[i] : (double)((float *)h.data())[i];
  return SWPS_OK;
}

int swps_w2v_set_params(swps_w2v *w, const double *hv) {
  if (!w->inited) SWPS_TRY(swps_w2v_init(w));
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  return set_hv(w, hv);
}

int swps_w2v_unigram_at(swps_w2v *w, const uint64_t *idx, uint64_t n, uint32_t *out) {
  if (w->cfg.minibatch_vocab) return fail(SWPS_E_STATE, "minibatch-vocab mode has one table per minibatch");
  if (w->cfg.sampler == SWPS_SAMPLER_ALIAS) return fail(SWPS_E_STATE, "the alias sampler has no slot table");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  SWPS_HIP(hipStreamSynchronize(w->s));
  for (uint64_t i = 0; i < n; i++) {
    if (idx[i] >= w->cfg.unigram_size) return fail(SWPS_E_CFG, "slot out of range");
    SWPS_HIP(hipMemcpy(out + i, w->d_unigram.as<int32_t>() + idx[i], 4, hipMemcpyDeviceToHost));
  }
  return SWPS_OK;
}

int swps_w2v_trace_negatives(swps_w2v *w, uint64_t cap) {
  w->trace_cap = cap;
  w->trace.clear();
  return SWPS_OK;
}

int swps_w2v_negatives(swps_w2v *w, int64_t *out, uint64_t cap, uint64_t *n) {
  *n = std::min<uint64_t>(cap, w->trace.size());
  std::copy(w->trace.begin(), w->trace.begin() + *n, out);
  return SWPS_OK;
}

int swps_w2v_set_profile(swps_w2v *w, int32_t on) {
  SWPS_TRY(swps_w2v_sync(w));
  w->timer.on = on != 0;
  return SWPS_OK;
}

int swps_w2v_kernel_times(swps_w2v *w, double *out, int32_t reset) {
  SWPS_TRY(swps_w2v_sync(w));
  for (int k = 0; k < KT_N; k++) {
    out[2 * k] = w->timer.ms[k];
    out[2 * k + 1] = (double)w->timer.cnt[k];
    if (reset) {
      w->timer.ms[k] = 0;
      w->timer.cnt[k] = 0;
    }
  }
  return SWPS_OK;
}

void *swps_w2v_stream(swps_w2v *w) { return (void *)w->s; }

int swps_unigram_starts(const uint64_t *keys, const int32_t *counts, uint64_t V, uint64_t table_size,
                        uint64_t *starts) {
  if (V == 0 || table_size == 0) return fail(SWPS_E_CFG, "empty vocab or table");
  std::vector<uint64_t> st;
  unigram_starts(keys, counts, V, table_size, st);
  std::copy(st.begin(), st.end(), starts);
  return SWPS_OK;
}

int swps_glibc_rand(uint32_t seed, uint64_t skip, uint64_t n, int32_t *out) {
  GlibcRand r(seed);
  r.discard(skip);
  for (uint64_t i = 0; i < n; i++) out[i] = r.next();
  return SWPS_OK;
}

}  // extern "C"

// ============================================================================
// Sharded mode: every rank is a worker (its own corpus,
// vocab, RNG streams and full-vocab cache, like a reference MPI rank) and a
// server for the keys BasicHashFrag assigns to node rank+1.  The caller moves
// bytes between ranks (RCCL all-to-all-v through torch.distributed; see
// swiftmpi_amd/dist.py); this library produces and consumes the payloads:
//   request    keys of the next batch grouped by owner      (pull request)
//   serve_pull owner: rows of the received keys  [n][h|v]    (pull response)
//   step       install the pulled rows, learn the batch, emit the mean
//              gradients [U][h|v] fp64 in request order        (push request)
//   serve_push owner: AdaGrad per source rank, in rank order (server.h:156-176)
// ============================================================================
extern "C" {

int swps_w2v_shard(swps_w2v *w, int32_t rank, int32_t world, int32_t frag_num) {
  if (!w->loaded) return fail(SWPS_E_STATE, "load a corpus first");
  if (w->inited) return fail(SWPS_E_STATE, "shard before swps_w2v_init / the first pull");
  if (world < 1 || rank < 0 || rank >= world) return fail(SWPS_E_CFG, "bad rank/world");
  if (w->cfg.init_mode == SWPS_W2V_INIT_REF)
    return fail(SWPS_E_UNSUPPORTED, "sharded mode initialises on the owners (SWPS_W2V_INIT_TABLE + SWPS_INIT_HASH): "
                                    "the reference's rand() order depends on message arrival");
  std::vector<uint32_t> map(frag_num);
  SWPS_TRY(swps_hashfrag_table(frag_num, world, map.data()));
  const uint64_t V = w->vocab_keys.size(), nb = w->batches.size();
  std::vector<int32_t> owner(V);
  for (uint64_t i = 0; i < V; i++) owner[i] = (int32_t)map[fmix64(w->vocab_keys[i]) % (uint64_t)frag_num] - 1;
  auto by_owner = [&](int32_t a, int32_t b) { return owner[a] != owner[b] ? owner[a] < owner[b] : a < b; };
  w->bcounts.assign(nb * world, 0);
  for (uint64_t bi = 0; bi < nb; bi++) {
    auto &b = w->batches[bi];
    std::sort(w->allK.begin() + b.kofs, w->allK.begin() + b.kofs + b.U, by_owner);
    for (uint32_t u = 0; u < b.U; u++) w->bcounts[bi * world + owner[w->allK[b.kofs + u]]]++;
  }
  w->init_order.resize(V);
  for (uint64_t i = 0; i < V; i++) w->init_order[i] = (int32_t)i;
  std::sort(w->init_order.begin(), w->init_order.end(), by_owner);
  w->icounts.assign(world, 0);
  for (uint64_t i = 0; i < V; i++) w->icounts[owner[i]]++;
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  SWPS_TRY(upload(w->d_K, w->allK, w->s));
  SWPS_TRY(upload(w->d_vkeys, w->vocab_keys, w->s));
  SWPS_TRY(upload(w->d_init_order, w->init_order, w->s));
  SWPS_HIP(hipStreamSynchronize(w->s));
  w->rank = rank;
  w->world = world;
  w->frag_num = frag_num;
  w->sharded = true;
  return SWPS_OK;
}

int swps_w2v_batch_counts(swps_w2v *w, uint64_t *out, uint64_t cap, uint64_t *nb) {
  if (!w->sharded) return fail(SWPS_E_STATE, "not sharded");
  *nb = w->batches.size();
  if (cap < w->bcounts.size()) return fail(SWPS_E_CFG, "buffer too small");
  std::copy(w->bcounts.begin(), w->bcounts.end(), out);
  return SWPS_OK;
}

// Server-side work (request, serve_pull, serve_push) is issued on the serve
// stream when one is set — the pipelined driver overlaps it, and the RCCL
// exchanges ordered on it, with the compute stream's minibatch.
int swps_w2v_set_serve_stream(swps_w2v *w, void *stream) {
  w->ss = (hipStream_t)stream;
  return SWPS_OK;
}

int swps_w2v_request(swps_w2v *w, int32_t init, uint64_t *counts, uint64_t *d_keys, uint64_t *n) {
  if (!w->sharded) return fail(SWPS_E_STATE, "not sharded");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  hipStream_t ss = w->ss ? w->ss : w->s;
  if (init) {
    std::copy(w->icounts.begin(), w->icounts.end(), counts);
    *n = w->vocab_keys.size();
    if (d_keys) k_vid_keys<<<nblk(*n), 256, 0, ss>>>(w->d_init_order.as<int32_t>(), *n, w->d_vkeys.as<uint64_t>(), d_keys);
  } else {
    const uint64_t bi = w->cursor % w->batches.size();
    const auto &b = w->batches[bi];
    std::copy(w->bcounts.begin() + bi * w->world, w->bcounts.begin() + (bi + 1) * w->world, counts);
    *n = b.U;
    if (d_keys && b.U)
      k_vid_keys<<<nblk(b.U), 256, 0, ss>>>(w->d_K.as<int32_t>() + b.kofs, b.U, w->d_vkeys.as<uint64_t>(), d_keys);
  }
  SWPS_HIP(hipGetLastError());
  return SWPS_OK;
}

int swps_w2v_serve_pull(swps_w2v *w, const uint64_t *d_keys, const uint64_t *src_counts, int32_t insert,
                        void *d_vals) {
  if (!w->sharded) return fail(SWPS_E_STATE, "not sharded");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  hipStream_t ss = w->ss ? w->ss : w->s;
  uint64_t n = 0;
  for (int r = 0; r < w->world; r++) n += src_counts[r];
  SWPS_TRY(w->d_serve_rows.ensure(std::max<uint64_t>(n, 1) * 4));
  uint32_t *rows = w->d_serve_rows.as<uint32_t>();
  if (!insert && w->slot >= 0) {  // a driver step slot: the same keys every epoch
    while ((uint64_t)w->slot >= w->slot_rows.size()) w->slot_rows.emplace_back(new swps_w2v::SlotRows());
    auto &e = *w->slot_rows[w->slot];
    if (e.n != n || !e.rows.p) {
      SWPS_TRY(e.rows.ensure(std::max<uint64_t>(n, 1) * 4));
      SWPS_TRY(table_lookup(w->t, d_keys, n, e.rows.as<uint32_t>(), ss));
      e.n = n;
      e.sorted_valid = false;
    }
    if (!d_vals && n) {  // the driver's in-place pull (AppOps::pull_in_place): the step's install reads
      if (w->world != 1) return fail(SWPS_E_STATE, "an in-place pull needs world 1");
      w->pull_rows = e.rows.as<uint32_t>();  // these rows of the shard itself
      return SWPS_OK;
    }
    return table_copy_pull(w->t, e.rows.as<uint32_t>(), n, d_vals, ss);
  }
  if (!d_vals && n) return fail(SWPS_E_STATE, "serve_pull without a value buffer needs a world-1 driver step slot");
  if (insert) {  // keys are distinct within a source, not across sources
    uint64_t off = 0;
    for (int r = 0; r < w->world; r++) {
      SWPS_TRY(table_find_or_insert(w->t, d_keys + off, src_counts[r], rows + off, ss));
      off += src_counts[r];
    }
  } else {
    SWPS_TRY(table_lookup(w->t, d_keys, n, rows, ss));
  }
  SWPS_TRY(table_copy_pull(w->t, rows, n, d_vals, ss));
  return SWPS_OK;
}

int swps_w2v_install_init(swps_w2v *w, const void *d_vals) {
  if (!w->sharded) return fail(SWPS_E_STATE, "not sharded");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  SWPS_TRY(install_init(w, d_vals));
  table_pin_once(w->t, w->pinned);  // vid_row / slot rows index the shard from here on
  w->inited = true;
  return SWPS_OK;
}

int swps_w2v_prep(swps_w2v *w) {
  if (!w->inited) return fail(SWPS_E_STATE, "init first");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  return prep_batch(w);
}

int swps_w2v_step(swps_w2v *w, const void *d_vals, void *d_grads) {
  if (!w->sharded) return fail(SWPS_E_STATE, "not sharded");
  if (!w->inited) return fail(SWPS_E_STATE, "init first");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  return learn_step(w, d_vals, d_grads);
}

// d_keys: the keys of the matching serve_pull (the push request carries its
// keys, as the reference's push Request does, global_push_access.h:48-67).
int swps_w2v_serve_push(swps_w2v *w, const uint64_t *d_keys, const void *d_grads, const uint64_t *src_counts) {
  if (!w->sharded) return fail(SWPS_E_STATE, "not sharded");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  hipStream_t ss = w->ss ? w->ss : w->s;
  uint64_t n = 0;
  for (int r = 0; r < w->world; r++) n += src_counts[r];
  const bool g32 = !w->f64 && !w->cfg.fp64_intermediates;  // fast mode: fp32 push payload
  int nsrc = 0;
  for (int r = 0; r < w->world; r++) nsrc += src_counts[r] > 0;
  if (w->slot >= 0 && (uint64_t)w->slot < w->slot_rows.size() && w->slot_rows[w->slot]->n == n &&
      w->slot_rows[w->slot]->rows.p) {  // this slot's pull looked the same keys up
    auto &e = *w->slot_rows[w->slot];
    return table_push_sources(w->t, e.rows.as<uint32_t>(), n, d_grads, ss, g32, nsrc <= 1, &e.sorted,
                              &e.sorted_valid);
  }
  SWPS_TRY(w->d_push_rows.ensure(std::max<uint64_t>(n, 1) * 4));
  SWPS_TRY(table_lookup(w->t, d_keys, n, w->d_push_rows.as<uint32_t>(), ss));
  // one AdaGrad step per source, in rank order, all sources in one pass
  return table_push_sources(w->t, w->d_push_rows.as<uint32_t>(), n, d_grads, ss, g32, nsrc <= 1);
}

// flags[j] = 1 when the j-th key served at slot `cur` (its cached row lookups) was served at slot
// `prev` too: a push of slot prev may change its row, so its pull must follow that push
static int w2v_late_mask(swps_w2v *w, int64_t cur, int64_t prev, uint8_t *d_flags, uint64_t n) {
  if (cur < 0 || prev < 0 || (uint64_t)cur >= w->slot_rows.size() || (uint64_t)prev >= w->slot_rows.size())
    return fail(SWPS_E_STATE, "late_mask: slot rows not cached");
  auto &ec = *w->slot_rows[cur], &ep = *w->slot_rows[prev];
  if (ec.n != n || (n && !ec.rows.p) || (ep.n && !ep.rows.p)) return fail(SWPS_E_STATE, "late_mask: slot rows not cached");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  hipStream_t ss = w->ss ? w->ss : w->s;
  const uint32_t cap = (uint32_t)w->t->cfg.capacity;
  if (!w->d_mark.p) {
    SWPS_TRY(w->d_mark.ensure((uint64_t)cap * 4));
    SWPS_HIP(hipMemsetAsync(w->d_mark.p, 0, (uint64_t)cap * 4, ss));
  }
  const uint32_t stamp = ++w->mark_stamp;
  if (ep.n) k_stamp_rows<<<nblk(ep.n), 256, 0, ss>>>(ep.rows.as<uint32_t>(), ep.n, cap, stamp, w->d_mark.as<uint32_t>());
  if (n)
    k_flag_rows<<<nblk(n), 256, 0, ss>>>(ec.rows.as<uint32_t>(), n, cap, stamp, w->d_mark.as<uint32_t>(), d_flags);
  SWPS_HIP(hipGetLastError());
  return SWPS_OK;
}

int swps_w2v_shard_comm(swps_w2v *w, swps_comm *c, int32_t frag_num) {
  if (!c) return fail(SWPS_E_CFG, "null communicator");
  if (comm_device(c) != w->t->cfg.device) return fail(SWPS_E_CFG, "communicator and table are on different devices");
  if (w->t->comm && w->t->comm != c) return fail(SWPS_E_CFG, "the table is routed over another communicator");
  if (w->drv) return fail(SWPS_E_STATE, "swps_w2v_shard_comm was already called on this context");
  SWPS_TRY(swps_w2v_shard(w, comm_rank(c), comm_world(c), frag_num));
  ShardDriver *d = new ShardDriver();
  d->c = c;
  AppOps &o = d->ops;
  o.h = w;
  o.cs = w->s;
  o.width = 2 * (uint64_t)w->D;
  o.val_bytes = w->f64 ? 8 : 4;
  o.grad_bytes = (w->f64 || w->cfg.fp64_intermediates) ? 8 : 4;
  o.batch_counts = [](void *h, uint64_t *out, uint64_t cap, uint64_t *nb) {
    return swps_w2v_batch_counts((swps_w2v *)h, out, cap, nb);
  };
  o.request = [](void *h, int32_t init, uint64_t *cnt, uint64_t *k, uint64_t *n) {
    return swps_w2v_request((swps_w2v *)h, init, cnt, k, n);
  };
  o.serve_pull = [](void *h, const uint64_t *k, const uint64_t *sc, int32_t ins, void *v) {
    return swps_w2v_serve_pull((swps_w2v *)h, k, sc, ins, v);
  };
  o.install = [](void *h, const void *v) { return swps_w2v_install_init((swps_w2v *)h, v); };
  // world 1: the step installs from the shard (serve_pull with no value buffer); SWPS_PULL_IN_PLACE=0: off (A/B)
  const char *pip = getenv("SWPS_PULL_IN_PLACE");
  o.pull_in_place = !(pip && atoi(pip) == 0);
  o.step = [](void *h, const void *v, void *g) { return swps_w2v_step((swps_w2v *)h, v, g); };
  o.serve_push = [](void *h, const uint64_t *k, const void *g, const uint64_t *sc) {
    return swps_w2v_serve_push((swps_w2v *)h, k, g, sc);
  };
  o.prep = [](void *h) { return swps_w2v_prep((swps_w2v *)h); };
  o.set_serve_stream = [](void *h, void *s) { return swps_w2v_set_serve_stream((swps_w2v *)h, s); };
  o.half_event = [](void *h) -> void * {
    swps_w2v *x = (swps_w2v *)h;
    const bool r = x->half_ready;
    x->half_ready = false;
    return r ? (void *)x->ev_half : nullptr;
  };
  o.set_slot = [](void *h, int64_t slot) {
    ((swps_w2v *)h)->slot = slot;
    return (int)SWPS_OK;
  };
  o.late_mask = [](void *h, int64_t cur, int64_t prev, uint8_t *f, uint64_t n) {
    return w2v_late_mask((swps_w2v *)h, cur, prev, f, n);
  };
  o.install_parts = [](void *h, const void *v0, const uint32_t *p0, uint64_t n0, const void *v1, const uint32_t *p1,
                       uint64_t n1) {
    auto &q = ((swps_w2v *)h)->parts;
    q.vals[0] = v0;
    q.pos[0] = p0;
    q.n[0] = n0;
    q.vals[1] = v1;
    q.pos[1] = p1;
    q.n[1] = n1;
    return (int)SWPS_OK;
  };
  const int rc = d->setup();
  if (rc) {
    delete d;
    return rc;
  }
  w->drv = d;
  return SWPS_OK;
}

int swps_w2v_exchange_stats(swps_w2v *w, int32_t on, double *out4) {
  if (!w->drv) return fail(SWPS_E_STATE, "not driven by swps_w2v_shard_comm");
  SWPS_TRY(w->drv->sync());
  if (out4) {
    out4[0] = (double)w->drv->bytes_remote;
    out4[1] = (double)w->drv->bytes_total;
    out4[2] = (double)w->drv->calls;
    out4[3] = w->drv->xms;
  }
  if (on >= 0) {
    w->drv->xprof = on != 0;
    w->drv->bytes_remote = w->drv->bytes_total = w->drv->calls = 0;
    w->drv->xms = 0;
  }
  return SWPS_OK;
}

}  // extern "C"

// ============================================================================
// Worker checkpoint (swps_w2v_save_state / swps_w2v_restore_state).  With the
// table snapshot (swps_save) it is an exact resume point at any batch
// boundary: the epoch plan is a function of the two LCG states at the epoch
// start, so those are stored instead of the plan, and the worker cache is
// stored because negatives outside a batch's key set read its stale rows.
//   "SWPSW2V2" | u64 config fp | u64 corpus fp | u64 V | u32 D | u32 esize |
//   u64 table snapshot checksum (swps_table::snap_sum of the swps_save that
//   goes with this state; restore_state requires the table to have been
//   swps_restore-d from exactly that file) |
//   u64 cursor, lstate0, fstate0, 6 counters, 2 row counters |
//   cache_h [V][D] | cache_v [V][D] (table dtype) | u64 checksum
// ============================================================================
namespace {

const char kW2VMagic[8] = {'S', 'W', 'P', 'S', 'W', '2', 'V', '2'};

uint64_t w2v_config_fp(const swps_w2v *w) {
  const auto &c = w->cfg;
  const uint64_t f[] = {(uint64_t)c.window,   (uint64_t)c.negative,         (uint64_t)c.min_sentence_length,
                        (uint64_t)c.minibatch, __float_as_uint_host(c.sample), __float_as_uint_host(c.alpha),
                        c.unigram_size,        (uint64_t)c.key_mode,         (uint64_t)c.fp64_intermediates,
                        (uint64_t)c.minibatch_vocab, (uint64_t)c.sampler,    (uint64_t)w->D,
                        (uint64_t)w->f64,      (uint64_t)w->sharded,         (uint64_t)w->rank,
                        (uint64_t)w->world,    (uint64_t)w->frag_num,
                        __float_as_uint_host(w->t->cfg.learning_rate), __float_as_uint_host(w->t->cfg.fudge)};
  return checksum64(1, f, sizeof(f));
}

uint64_t w2v_corpus_fp(const swps_w2v *w) {
  uint64_t h = checksum64(2, &w->train_words, 8);
  h = checksum64(h, w->vocab_keys.data(), w->vocab_keys.size() * 8);
  h = checksum64(h, w->counts.data(), w->counts.size() * 4);
  h = checksum64(h, w->line_off.data(), w->line_off.size() * 8);
  return checksum64(h, &w->tok_fp, 8);
}

}  // namespace

extern "C" {

int swps_w2v_save_state(swps_w2v *w, const char *path) {
  if (!w->inited) return fail(SWPS_E_STATE, "nothing to save: the context is not initialised");
  if (w->drv && w->drv->spe && w->drv->cursor % w->drv->spe != 0)
    return fail(SWPS_E_STATE, "a library-driven sharded context saves at epoch boundaries (swps_w2v_train_epochs)");
  SWPS_TRY(swps_w2v_sync(w));
  const uint64_t nb = std::max<uint64_t>(1, w->batches.size());
  // the current epoch is planned once its first batch was prepared
  const bool planned = w->cursor % nb != 0 || w->pb.valid;
  const uint64_t V = w->vocab_keys.size();
  const uint32_t es = w->f64 ? 8 : 4;
  uint64_t rt[2] = {0, 0};
  SWPS_HIP(hipMemcpy(rt, w->d_rows_touched.p, 16, hipMemcpyDeviceToHost));
  if (!w->t->snap_sum)
    return fail(SWPS_E_STATE, "save the table first (swps_save): the worker state is tied to that table snapshot");
  const uint64_t head[] = {w2v_config_fp(w), w2v_corpus_fp(w), V, (uint64_t)w->D | ((uint64_t)es << 32),
                           w->t->snap_sum};
  const uint64_t st[] = {w->cursor,       planned ? w->lstate_epoch : w->lstate,
                         planned ? w->fstate_epoch : w->fstate,
                         w->st_batches,   w->st_kept, w->st_words, w->st_pairs, w->st_pulled, w->st_pushed, rt[0], rt[1]};
  std::vector<char> cache(V * w->D * es);
  SnapFile f;
  SWPS_TRY(f.open(path, true));
  SWPS_TRY(f.put(kW2VMagic, 8));
  SWPS_TRY(f.put(head, sizeof(head)));
  SWPS_TRY(f.put(st, sizeof(st)));
  for (DevMem *m : {&w->d_cache_h, &w->d_cache_v}) {
    if (!cache.empty())  // unpadded [V][D] in the file whatever the device row stride
      SWPS_HIP(hipMemcpy2D(cache.data(), w->D * es, m->p, (size_t)w->cs * es, w->D * es, V, hipMemcpyDeviceToHost));
    SWPS_TRY(f.put(cache.data(), cache.size()));
  }
  return f.finish_write();
}

int swps_w2v_restore_state(swps_w2v *w, const char *path) {
  if (!w->loaded) return fail(SWPS_E_STATE, "load the corpus first");
  if (w->inited) return fail(SWPS_E_STATE, "restore_state needs a fresh context (corpus loaded, not initialised)");
  SWPS_HIP(hipSetDevice(w->t->cfg.device));
  const uint64_t V = w->vocab_keys.size();
  const uint32_t es = w->f64 ? 8 : 4;
  SnapFile f;
  SWPS_TRY(f.open(path, false));
  char magic[8];
  uint64_t head[5], st[11];
  if (f.get(magic, 8) != SWPS_OK || memcmp(magic, kW2VMagic, 8) != 0)
    return fail(SWPS_E_IO, std::string("not a swps word2vec state snapshot: ") + path);
  SWPS_TRY(f.get(head, sizeof(head)));
  SWPS_TRY(f.get(st, sizeof(st)));
  if (head[0] != w2v_config_fp(w))
    return fail(SWPS_E_CFG, "snapshot was taken with a different word2vec config (window, negative, minibatch, "
                            "sample, alpha, dim, dtype, precision mode, sampler or sharding)");
  if (head[1] != w2v_corpus_fp(w) || head[2] != V || head[3] != ((uint64_t)w->D | ((uint64_t)es << 32)))
    return fail(SWPS_E_CFG, "snapshot was taken on a different corpus");
  if (head[4] != w->t->snap_sum)
    return fail(SWPS_E_STATE, "the table was not restored from the table snapshot saved with this worker state "
                              "(swps_restore <prefix>.table of the same save first)");
  std::vector<char> ch(V * w->D * es), cv(ch.size());
  SWPS_TRY(f.get(ch.data(), ch.size()));
  SWPS_TRY(f.get(cv.data(), cv.size()));
  SWPS_TRY(f.finish_read());
  if (!w->sharded) {  // the vocab rows must be in the table already (swps_restore)
    DevMem dk;
    SWPS_TRY(upload(dk, w->vocab_keys, w->s));
    SWPS_TRY(table_lookup(w->t, dk.as<uint64_t>(), V, w->d_vid_row.as<uint32_t>(), w->s));
    if (table_check_error(w->t, w->s) != SWPS_OK)
      return fail(SWPS_E_STATE, "the table lacks the worker's vocab rows: swps_restore its table snapshot first");
  }
  if (!ch.empty()) {
    SWPS_HIP(hipMemcpy2D(w->d_cache_h.p, (size_t)w->cs * es, ch.data(), w->D * es, w->D * es, V,
                         hipMemcpyHostToDevice));
    SWPS_HIP(hipMemcpy2D(w->d_cache_v.p, (size_t)w->cs * es, cv.data(), w->D * es, w->D * es, V,
                         hipMemcpyHostToDevice));
  }
  SWPS_HIP(hipMemcpy(w->d_rows_touched.p, st + 9, 16, hipMemcpyHostToDevice));
  w->cursor = st[0];
  w->lstate = st[1];
  w->fstate = st[2];
  w->st_batches = st[3];
  w->st_kept = st[4];
  w->st_words = st[5];
  w->st_pairs = st[6];
  w->st_pulled = st[7];
  w->st_pushed = st[8];
  w->pb = swps_w2v::Prepped();
  const uint64_t nb = std::max<uint64_t>(1, w->batches.size());
  if (w->cursor % nb != 0) SWPS_TRY(plan_epoch(w));  // mid-epoch: re-plan from the epoch-start states
  if (w->drv) {
    // the library driver's lockstep step count is not this rank's batch count (ranks with fewer
    // batches idle to the epoch's end), so its saves are at epoch boundaries (save_state), where
    // it is epochs * spe; its server work then goes to the serve stream, as after full_pull
    if (w->cursor % nb != 0) return fail(SWPS_E_STATE, "library-driven sharded state not at an epoch boundary");
    w->drv->cursor = w->cursor / nb * w->drv->spe;
    if (w->drv->ops.set_serve_stream) SWPS_TRY(w->drv->ops.set_serve_stream(w, w->drv->S));
  }
  table_pin_once(w->t, w->pinned);  // vid_row / slot rows index the shard from here on
  w->inited = true;
  return SWPS_OK;
}

}  // extern "C"
