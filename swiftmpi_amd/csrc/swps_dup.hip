// Repeated keys on the HBM shard: coalesce, lookup and the coalescing push.
//
// swps_pull / swps_push take distinct keys (the reference's std::unordered_set key sets).  The
// calls of this unit take a batch of ids as a caller holds it: the keys may repeat and ~0 is a
// padding id.  The dedup is a stable radix sort of (key, position) pairs, so each key's run is in
// ascending position and its head is the first occurrence; the insert / lookup kernels of the
// table only ever see the distinct keys; the gradients of a run are summed in fp64 in the order
// fixed by include/swps.h (chunks of SWPS_DUP_CHUNK occurrences, each a chain from its first
// element, the chunk sums chained in chunk order) and applied as ONE step of the push rule.
//
// No kernel here waits on another thread: every dependency is a kernel boundary.  The kernels and
// the host helpers live in swps_dup.h, which the pooled calls (swps_bag.hip) share.
#include "swps_dup.h"
#include "swps_admit.h"

using namespace swps;

extern "C" {

int swps_coalesce(swps_table *t, const uint64_t *d_keys, uint64_t n, uint64_t *d_uniq, uint32_t *d_inv,
                  uint32_t *d_count, uint64_t *nu, void *stream) {
  if (!t || (n && !d_keys)) return fail(SWPS_E_CFG, "null argument");
  SWPS_TRY(check_n(n));
  if (nu) *nu = 0;
  if (n == 0) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : t->stream;
  Runs R;
  SWPS_TRY(sorted_runs(t, d_keys, n, s, false, R));
  SWPS_TRY(rank_runs(t, R, d_uniq, d_inv, d_count, s));
  SWPS_HIP(hipStreamSynchronize(s));
  if (nu) *nu = R.nu;
  return SWPS_OK;
}

int swps_lookup(swps_table *t, const uint64_t *d_keys, uint64_t n, int32_t insert, void *d_vals, uint8_t *d_found,
                void *stream) {
  if (insert != 0 && insert != 1) return fail(SWPS_E_CFG, "insert must be 0 or 1");
  if (!t || (n && (!d_keys || !d_vals))) return fail(SWPS_E_CFG, "null argument");
  SWPS_TRY(check_n(n));
  if (t->comm && !insert) return fail(SWPS_E_UNSUPPORTED, "swps_lookup without insert on a routed table");
  if (n == 0 && !t->comm) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : t->stream;
  Runs R;
  uint64_t *uniq = nullptr;
  uint32_t *inv = nullptr, *count = nullptr;
  const bool gated = insert && !t->comm && t->adm_min > 1;  // admission by count
  if (n) {
    SWPS_TRY(sorted_runs(t, d_keys, n, s, false, R));
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
  uint32_t *pad_flag = insert ? t->counters.as<uint32_t>() + 1 : nullptr;
  if (t->comm) {  // collective: the routed pull of the distinct keys, scattered through inv
    const size_t cb = (size_t)t->pull_elems * t->esize;
    SWPS_TRY(t->dup[B_VALS].ensure((R.nu + 1) * cb));
    SWPS_TRY(routed_pull(t, uniq, R.nu, t->dup[B_VALS].p, s));
    if (n) SWPS_TRY(gather(t, inv, nullptr, n, t->dup[B_VALS].p, cb, d_vals, d_found, pad_flag, s));
    return table_check_error(t, s);
  }
  SWPS_TRY(t->dup[B_ROWS].ensure((R.nu + 1) * 4));
  uint32_t *row_u = t->dup[B_ROWS].as<uint32_t>();
  int rc = SWPS_OK;
  std::string msg;
  if (insert) {
    // exactly swps_pull's insert of the distinct list (growth, init_param, latches); a failure
    // (table full) still leaves the found keys' rows, which are returned as swps_pull returns them;
    // gated: the same insert of the admitted keys only, a refused key reads as an absent one
    rc = gated ? admit_insert(t, uniq, count, R.nu, row_u, s) : table_find_or_insert(t, uniq, R.nu, row_u, s);
    if (rc != SWPS_OK && rc != SWPS_E_OOM && rc != SWPS_E_BADKEY) return rc;
    if (rc != SWPS_OK) msg = swps_last_error();
  } else {
    SWPS_TRY(table_probe(t, uniq, R.nu, row_u, s));
  }
  SWPS_TRY(gather(t, inv, row_u, n, t->rows.p, (size_t)t->row_elems * t->esize, d_vals, d_found, pad_flag, s));
  const int rc2 = table_check_error(t, s);
  if (rc != SWPS_OK) return fail(rc, msg);
  return rc2;
}

int swps_push_dup(swps_table *t, const uint64_t *d_keys, uint64_t n, const void *d_grads, int32_t gdtype,
                  int32_t reduce, double scale, void *stream) {
  if (reduce != SWPS_REDUCE_SUM && reduce != SWPS_REDUCE_MEAN) return fail(SWPS_E_CFG, "unknown reduce");
  if (gdtype != SWPS_F32 && gdtype != SWPS_F64) return fail(SWPS_E_CFG, "gdtype must be SWPS_F32 or SWPS_F64");
  if (!t || (n && (!d_keys || !d_grads))) return fail(SWPS_E_CFG, "null argument");
  SWPS_TRY(check_n(n));
  if (t->cfg.layout == SWPS_LAYOUT_LR && gdtype != SWPS_F32)
    return fail(SWPS_E_CFG, "an LR table takes fp32 gradients (gdtype SWPS_F32)");
  if (n == 0 && !t->comm) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : t->stream;
  Runs R;
  uint64_t *rkeys = nullptr;
  if (n) {
    SWPS_TRY(sorted_runs(t, d_keys, n, s, true, R));
    SWPS_TRY(t->dup[B_UNIQ].ensure((R.nu + 1) * 8));
    rkeys = t->dup[B_UNIQ].as<uint64_t>();  // the distinct keys in key order: no rank is needed here
    if (R.nu) {
      k_dup_run_keys<<<nblk(R.nu), 256, 0, s>>>(R.ks, R.run_start, R.nu, rkeys);
      SWPS_HIP(hipGetLastError());
    }
  }
  if (t->comm) {  // collective: one reduced gradient per distinct key, then the routed push
    const size_t gb = (size_t)t->push_elems * (t->cfg.layout == SWPS_LAYOUT_W2V ? 8 : 4);
    SWPS_TRY(t->dup[B_VALS].ensure((R.nu + 1) * gb));
    if (R.nu) SWPS_TRY(reduce_runs<false>(t, R, d_grads, gdtype, nullptr, t->dup[B_VALS].p, reduce, scale, s));
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
    SWPS_TRY(reduce_runs<true>(t, R, d_grads, gdtype, row_r, nullptr, reduce, scale, s));
  }
  return table_check_error(t, s);
}

int swps_lookup_h(swps_table *t, const uint64_t *keys, uint64_t n, int32_t insert, void *vals, uint8_t *found) {
  if (insert != 0 && insert != 1) return fail(SWPS_E_CFG, "insert must be 0 or 1");
  if (!t || (n && (!keys || !vals))) return fail(SWPS_E_CFG, "null argument");
  SWPS_TRY(check_n(n));
  if (n == 0 && !t->comm) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  const uint64_t m = n * (uint64_t)t->pull_elems;
  DevMem dk, dv, df;
  SWPS_TRY(dk.ensure(n * 8));
  SWPS_TRY(dv.ensure(m * t->esize));
  SWPS_TRY(df.ensure(n));
  SWPS_HIP(hipMemcpyAsync(dk.p, keys, n * 8, hipMemcpyHostToDevice, t->stream));
  const int rc = swps_lookup(t, dk.as<uint64_t>(), n, insert, dv.p, df.as<uint8_t>(), nullptr);  // syncs
  if (rc != SWPS_OK && rc != SWPS_E_OOM && rc != SWPS_E_BADKEY) return rc;
  const std::string msg = rc != SWPS_OK ? swps_last_error() : "";
  if (found && n) SWPS_HIP(hipMemcpy(found, df.p, n, hipMemcpyDeviceToHost));
  const bool w2v = t->cfg.layout == SWPS_LAYOUT_W2V;
  const size_t out_es = w2v ? 8 : 4;
  if (t->esize == out_es) {
    if (m) SWPS_HIP(hipMemcpy(vals, dv.p, m * out_es, hipMemcpyDeviceToHost));
  } else {
    std::vector<char> tmp(m * t->esize);
    if (m) SWPS_HIP(hipMemcpy(tmp.data(), dv.p, tmp.size(), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < m; i++) {
      if (w2v)
        ((double *)vals)[i] = (double)((float *)tmp.data())[i];
      else
        ((float *)vals)[i] = (float)((double *)tmp.data())[i];
    }
  }
  return rc != SWPS_OK ? fail(rc, msg) : SWPS_OK;
}

int swps_push_dup_h(swps_table *t, const uint64_t *keys, uint64_t n, const void *grads, int32_t reduce,
                    double scale) {
  if (reduce != SWPS_REDUCE_SUM && reduce != SWPS_REDUCE_MEAN) return fail(SWPS_E_CFG, "unknown reduce");
  if (!t || (n && (!keys || !grads))) return fail(SWPS_E_CFG, "null argument");
  SWPS_TRY(check_n(n));
  if (n == 0 && !t->comm) return SWPS_OK;
  SWPS_HIP(hipSetDevice(t->cfg.device));
  const bool w2v = t->cfg.layout == SWPS_LAYOUT_W2V;
  const size_t gb = n * (uint64_t)t->push_elems * (w2v ? 8 : 4);
  DevMem dk, dg;
  SWPS_TRY(dk.ensure(n * 8));
  SWPS_TRY(dg.ensure(gb));
  SWPS_HIP(hipMemcpyAsync(dk.p, keys, n * 8, hipMemcpyHostToDevice, t->stream));
  SWPS_HIP(hipMemcpyAsync(dg.p, grads, gb, hipMemcpyHostToDevice, t->stream));
  return swps_push_dup(t, dk.as<uint64_t>(), n, dg.p, w2v ? SWPS_F64 : SWPS_F32, reduce, scale, nullptr);  // syncs
}

}  // extern "C"
