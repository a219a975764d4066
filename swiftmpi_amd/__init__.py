"""swiftmpi_amd — MI355X-native rebuild of SwiftMPI's data-parallel hot path.

The pull -> gradient -> push loop of SwiftMPI's sparse parameter server
(word2vec CBOW negative sampling, sparse logistic regression) runs as HIP
kernels over HBM-resident key-hash-sharded tables (libswps.so, C ABI in
include/swps.h).  This package is the Python mirror of the reference's app
interfaces over that ABI:

    Table     <- parameter/sparsetable.h + cluster/server.h pull/push handlers
    Word2Vec  <- apps/word2vec/word2vec_global.h  (Word2Vec<MiniBatch>)
    Sent2Vec  <- apps/sent2vec/sent2vec.cpp       (Sent2Vec)
    LR        <- apps/logistic/lr.cpp             (LR)
    Config    <- utils/ConfigParser.h

Every compute call goes through libswps.so; if it is missing the import of the
classes below raises (no CPU fallback).
"""
import ctypes
import weakref

import numpy as np

from . import capi
from .capi import SwpsError, check, ptr

__all__ = ["Table", "Word2Vec", "Sent2Vec", "LR", "Config", "SwpsError", "bkdr", "fmix64", "hashfrag_table",
           "to_node_id", "load_library", "grow_plan", "erase_plan"]


def load_library():
    return capi.lib()


def bkdr(word):
    """BKDRHash<size_t>(word, 13131) (utils/string.h:130-137)."""
    if isinstance(word, str):
        word = word.encode("utf-8")
    return int(capi.lib().swps_bkdr(word))


def fmix64(x):
    return int(capi.lib().swps_fmix64(x))


def hashfrag_table(frag_num, num_nodes):
    out = np.zeros(frag_num, dtype=np.uint32)
    check(capi.lib().swps_hashfrag_table(frag_num, num_nodes, ptr(out)))
    return out


def to_node_id(keys, frag_num, table):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.zeros(len(keys), dtype=np.int32)
    check(capi.lib().swps_to_node_id(ptr(keys), len(keys), frag_num, ptr(table), ptr(out)))
    return out


def unigram_starts(keys, counts, table_size=int(1e8)):
    """Run-length form of gen_unigram_table (host helper of libswps)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    out = np.zeros(len(keys) + 1, dtype=np.uint64)
    check(capi.lib().swps_unigram_starts(ptr(keys), ptr(counts), len(keys), table_size, ptr(out)))
    return out


def glibc_rand(n, seed=1, skip=0):
    out = np.zeros(n, dtype=np.int32)
    check(capi.lib().swps_glibc_rand(seed, skip, n, ptr(out)))
    return out


def grow_plan(capacity, max_capacity, nrows, incoming):
    """The growth policy of a table under a ceiling (swps_grow_plan, host only):
    -> (new_capacity, new_slots) before an insert of `incoming` keys."""
    nc, ns = ctypes.c_uint64(), ctypes.c_uint64()
    check(capi.lib().swps_grow_plan(capacity, max_capacity, nrows, incoming, ctypes.byref(nc), ctypes.byref(ns)))
    return nc.value, ns.value


def erase_plan(dead):
    """The compaction rule of an erase (swps_erase_plan, host only): dead[r] != 0 marks the rows to
    remove -> (survivors M, src, dst): the live rows src[k] >= M move into the dead rows dst[k] < M,
    both ascending; every other row stays."""
    d = np.ascontiguousarray(np.asarray(dead).reshape(-1) != 0, dtype=np.uint8)
    m, h = ctypes.c_uint64(), ctypes.c_uint64()
    src = np.zeros(max(len(d) // 2, 1), dtype=np.uint32)  # moves <= min(#dead, M) <= N / 2
    dst = np.zeros_like(src)
    check(capi.lib().swps_erase_plan(ptr(d), len(d), ctypes.byref(m), ptr(src), ptr(dst), len(src), ctypes.byref(h)))
    return m.value, src[:h.value], dst[:h.value]


class Config:
    """The reference's INI-like config (utils/ConfigParser.h:84-115):
    ``[section]`` headers, ``key: value`` lines, ``#`` comments, ``import path``.
    ``get(section, key)`` raises KeyError like the reference's CHECK."""

    def __init__(self, path=None):
        self.sections = {}
        if path:
            self.parse(path)

    def parse(self, path):
        cur = ""
        with open(path) as f:
            for line in f:
                line = line.strip(" \t\n\r")
                if not line or line.startswith("#"):
                    continue
                if line.startswith("import"):
                    sub = line.split(" ", 1)[1].strip()
                    if sub == path:
                        raise ValueError("recursive import")
                    self.parse(sub)
                    continue
                if line[0] == "[" and line[-1] == "]":
                    cur = line[1:-1].strip()
                    if not cur:
                        raise ValueError("empty section")
                    continue
                if ":" not in line:
                    raise ValueError(f"bad config line: {line}")
                k, v = line.split(":", 1)
                self.sections.setdefault(cur, {}).setdefault(k.strip(), v.strip())
        return self

    def get(self, section, key):
        try:
            return self.sections[section][key]
        except KeyError:
            raise KeyError(f"no such key:\t[{section}]\t{key}")

    def get_int(self, section, key):
        return int(self.get(section, key))

    def get_float(self, section, key):
        return float(self.get(section, key))


class Table:
    """One HBM parameter shard (SparseTable + server access methods)."""

    def __init__(self, layout="w2v", dim=100, capacity=1 << 20, dtype="f32", learning_rate=0.7, fudge=1e-6,
                 init="hash", seed=0, device=0, push_rule="adagrad", max_capacity=None, admit_min_count=None,
                 admit_width=1 << 20):
        """max_capacity: the ceiling under which inserts grow the shard by themselves (None / 0:
        the capacity is fixed, as in the reference-sized default); `capacity` is the starting size.
        admit_min_count / admit_width: `set_admission` at creation (None: every new id gets a row)."""
        inits = {"hash": capi.INIT_HASH, "zero": capi.INIT_ZERO, "flcg": capi.INIT_FLCG}
        rules = {"adagrad": capi.PUSH_ADAGRAD, "sgd": capi.PUSH_SGD}
        layouts = {"w2v": capi.LAYOUT_W2V, "lr": capi.LAYOUT_LR}
        dtypes = {"f32": capi.F32, "f64": capi.F64}
        for name, val, known in (("init", init, inits), ("push_rule", push_rule, rules), ("layout", layout, layouts),
                                 ("dtype", dtype, dtypes)):
            if val not in known:
                raise ValueError("unknown %s %r (one of %s)" % (name, val, ", ".join(sorted(known))))
        cfg = capi.TableCfg(device, layouts[layout], dtypes[dtype], dim, capacity, learning_rate, fudge,
                            inits[init], seed, rules[push_rule])
        h = ctypes.c_void_p()
        check(capi.lib().swps_table_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.layout, self.dim, self.dtype, self.device = layout, dim, dtype, device
        r, p, q = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        capi.lib().swps_table_row_elems(self.h, ctypes.byref(r), ctypes.byref(p), ctypes.byref(q))
        self.row_elems, self.pull_elems, self.push_elems = r.value, p.value, q.value
        self._deps = weakref.WeakSet()  # app contexts bound to this shard: closed first
        if max_capacity:
            self.set_max_capacity(max_capacity)
        if admit_min_count is not None:
            self.set_admission(admit_min_count, admit_width)

    def close(self):
        if getattr(self, "h", None):
            for d in list(getattr(self, "_deps", ())):
                d.close()
            capi.lib().swps_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except (AttributeError, TypeError):  # interpreter shutdown: modules already torn down
            pass

    @property
    def torch_dtype(self):
        import torch
        return torch.float64 if self.dtype == "f64" else torch.float32

    def size(self):
        n = ctypes.c_uint64()
        check(capi.lib().swps_table_size(self.h, ctypes.byref(n)))
        return n.value

    # ---- growth (swps_table_reserve / _set_max_capacity / _capacity) ----
    def reserve(self, keys):
        """Capacity >= keys from now on: moves the shard (every key, row and row index kept; peak
        footprint old + new) unless it already has the room.  SWPS_E_STATE while an app context
        that completed its init holds the table."""
        check(capi.lib().swps_table_reserve(self.h, keys))

    def set_max_capacity(self, max_keys):
        """The ceiling of automatic growth (0: fixed capacity)."""
        check(capi.lib().swps_table_set_max_capacity(self.h, max_keys))

    def capacity(self):
        out = np.zeros(4, dtype=np.uint64)
        check(capi.lib().swps_table_capacity(self.h, ptr(out)))
        return dict(zip(["capacity", "max_capacity", "slots", "growths"], (int(x) for x in out)))

    # ---- removal (swps_erase / swps_prune / swps_table_shrink) ----
    def erase(self, keys):
        """Remove the listed keys -> the number of distinct keys removed from the local shard.
        keys: an int64 CUDA tensor or an integer numpy array / sequence, of any shape; repeats,
        keys the table lacks and -1 (~0) are ignored.  Survivors keep their rows bit for bit but
        may change row index (`keys()` follows `erase_plan`), so SWPS_E_STATE while an app context
        holds the table.  The hash index is rebuilt on every call that removes a key (a cost
        proportional to the slot count): batch the keys.  Collective on a routed table (tensor
        keys only), where the count is this rank's shard's."""
        n = ctypes.c_uint64()
        if hasattr(keys, "data_ptr"):
            import torch
            if keys.dtype != torch.int64:
                raise TypeError("keys must be an int64 tensor")
            k = keys.contiguous().view(-1)
            if k.numel() and not k.is_cuda:
                raise TypeError("tensor keys must live on the table's device (pass a numpy array for host keys)")
            if k.numel():
                self._stream(k)  # the keys are complete before the table's own stream reads them
            check(capi.lib().swps_erase(self.h, ptr(k), k.numel(), ctypes.byref(n)))
            return n.value
        a = np.asarray(keys)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError("keys must be integers, not %s" % a.dtype)
        k = np.ascontiguousarray(self._keys_like(a.reshape(-1) if a.size else np.zeros(0, np.uint64), False, None))
        check(capi.lib().swps_erase_h(self.h, ptr(k), len(k), ctypes.byref(n)))
        return n.value

    def prune(self, max_g2=0.0):
        """Remove every key whose AdaGrad accumulators (w2v: h2sum and v2sum; lr: grad2sum) are all
        <= max_g2 -> the number removed.  0.0: the keys that never received a non-zero gradient.
        A row with a NaN accumulator is kept.  Local to the shard; otherwise as `erase`."""
        if isinstance(max_g2, bool) or not isinstance(max_g2, (int, float, np.integer, np.floating)):
            raise TypeError("max_g2 must be a real number")
        max_g2 = float(max_g2)
        if max_g2 != max_g2 or max_g2 < 0:
            raise ValueError("max_g2 must be >= 0 (the accumulators are sums of squares), not %r" % max_g2)
        n = ctypes.c_uint64()
        check(capi.lib().swps_prune(self.h, max_g2, ctypes.byref(n)))
        return n.value

    def shrink(self, keys=0):
        """Capacity = max(keys, rows held, 1) when that is below the current capacity (a move, as
        `reserve`: counted in `growths`, SWPS_E_STATE while pinned); otherwise nothing happens."""
        keys = int(keys)
        if keys < 0:
            raise ValueError("keys must be >= 0")
        check(capi.lib().swps_table_shrink(self.h, keys))

    # ---- admission by count (swps_table_set_admission / swps_admission_*) ----
    def set_admission(self, min_count, width=1 << 20):
        """Gate the inserting lookups (`lookup`, `lookup_bag`, the nn modules) on a count-min
        sketch of 4 x width counters beside the shard: an id gets a row only once it has been asked
        for `min_count` times while absent; until then it reads as a zero row (found = 0) and its
        gradient is skipped.  min_count <= 1 (or None) turns the gate off and frees the sketch.
        width: a power of two in [2^6, 2^30].  Calling it again zeroes the sketch and the counters.
        `pull`, `assign`, `load` and `restore` are never gated; not available on a routed table."""
        min_count = 0 if min_count is None else min_count
        for name, v in (("min_count", min_count), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s must be an integer" % name)
        min_count, width = int(min_count), int(width)
        if min_count < 0 or min_count >= 1 << 32:
            raise ValueError("min_count must be in [0, 2^32)")
        if min_count > 1 and (width < 1 << 6 or width > 1 << 30 or width & (width - 1)):
            raise ValueError("width must be a power of two in [2^6, 2^30], not %d" % width)
        check(capi.lib().swps_table_set_admission(self.h, min_count, width))

    def admission(self):
        """The gate's settings and counters: min_count (0: off), width, depth, and the absent keys
        tested / admitted / refused by the inserting lookups since `set_admission`."""
        out = np.zeros(6, dtype=np.uint64)
        check(capi.lib().swps_admission_info(self.h, ptr(out)))
        return dict(zip(["min_count", "width", "depth", "tested", "admitted", "refused"], (int(x) for x in out)))

    def admission_decay(self, shift=1):
        """Every counter of the sketch >>= shift (1..31); 32 clears it.  Ages old counts, so an id
        has to keep coming to be admitted."""
        if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)):
            raise TypeError("shift must be an integer")
        if not 1 <= int(shift) <= 32:
            raise ValueError("shift must be in 1..32 (32 clears)")
        check(capi.lib().swps_admission_decay(self.h, int(shift)))

    def admission_cells(self):
        """The sketch as a numpy uint32 [4, width] array (a checkpoint: `admission_load` puts it back)."""
        width = self.admission()["width"]
        out = np.zeros((capi.ADMIT_DEPTH, max(width, 1)), dtype=np.uint32)
        n = ctypes.c_uint64()
        check(capi.lib().swps_admission_cells(self.h, ptr(out), out.size, ctypes.byref(n)))
        return out

    def admission_load(self, cells):
        """Overwrite the sketch with a uint32 [4, width] array of the width set by `set_admission`."""
        a = np.asarray(cells)
        if a.dtype != np.uint32:
            raise TypeError("cells must be uint32, not %s" % a.dtype)
        if a.ndim != 2 or a.shape[0] != capi.ADMIT_DEPTH:
            raise ValueError("cells must have the shape [%d, width]" % capi.ADMIT_DEPTH)
        a = np.ascontiguousarray(a)
        check(capi.lib().swps_admission_load(self.h, ptr(a), a.size))

    def pull(self, keys):
        """keys: int64/uint64 CUDA tensor of distinct keys -> [n, pull_elems] tensor."""
        import torch
        out = torch.empty((keys.numel(), self.pull_elems), dtype=self.torch_dtype, device=keys.device)
        check(capi.lib().swps_pull(self.h, ptr(keys), keys.numel(), ptr(out)))
        return out

    def push(self, keys, grads):
        """grads: [n, push_elems] CUDA tensor, fp64 (w2v) or fp32 (lr) — the reference wire types."""
        check(capi.lib().swps_push(self.h, ptr(keys), keys.numel(), ptr(grads)))
        capi.lib().swps_table_sync(self.h)

    def assign(self, keys, rows):
        check(capi.lib().swps_assign(self.h, ptr(keys), keys.numel(), ptr(rows)))

    def export(self, keys):
        import torch
        out = torch.empty((keys.numel(), self.row_elems), dtype=self.torch_dtype, device=keys.device)
        check(capi.lib().swps_export(self.h, ptr(keys), keys.numel(), ptr(out)))
        return out

    def keys(self):
        n = self.size()
        out = np.zeros(max(n, 1), dtype=np.uint64)
        m = ctypes.c_uint64()
        check(capi.lib().swps_table_keys(self.h, ptr(out), len(out), ctypes.byref(m)))
        return out[:m.value]

    def dump(self, path):
        check(capi.lib().swps_dump(self.h, path.encode()))

    def load(self, path, frag_num=1000, world=1, node_id=0):
        check(capi.lib().swps_load(self.h, path.encode(), frag_num, world, node_id))

    def save(self, path):
        """Binary snapshot of every key and row, bit for bit (swps_save)."""
        check(capi.lib().swps_save(self.h, path.encode()))

    def restore(self, path, frag_num=1000, world=1, node_id=0):
        """Assign the rows of a swps_save snapshot (node_id's keys only when
        world > 1, as `load`); the file is verified before any row changes."""
        check(capi.lib().swps_restore(self.h, path.encode(), frag_num, world, node_id))

    # ---- key-sharded mode (swps_table_route): pull / push become collective ----
    def route(self, comm, frag_num=1000):
        check(capi.lib().swps_table_route(self.h, comm.h, frag_num))
        self._comm = comm  # the communicator must outlive the routed table

    def finish(self):
        check(capi.lib().swps_finish(self.h))

    def barrier(self):
        check(capi.lib().swps_barrier(self.h))

    def route_stats(self):
        out = np.zeros(6, dtype=np.uint64)
        check(capi.lib().swps_route_stats(self.h, ptr(out)))
        return dict(zip(["rounds", "keys_sent", "keys_remote", "bytes_sent", "bytes_remote", "keys_served"],
                        (int(x) for x in out)))

    def pull_h(self, keys):
        """Host keys (uint64) -> host pull values in the wire type (W2V fp64, LR fp32)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros((len(keys), self.pull_elems), dtype=np.float64 if self.layout == "w2v" else np.float32)
        check(capi.lib().swps_pull_h(self.h, ptr(keys), len(keys), ptr(out)))
        return out

    def push_h(self, keys, grads):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        grads = np.ascontiguousarray(grads, dtype=np.float64 if self.layout == "w2v" else np.float32)
        check(capi.lib().swps_push_h(self.h, ptr(keys), len(keys), ptr(grads)))

    # ---- repeated keys (swps_coalesce / swps_lookup / swps_push_dup) ----
    _REDUCE = {"sum": capi.REDUCE_SUM, "mean": capi.REDUCE_MEAN, 0: 0, 1: 1}

    @staticmethod
    def _stream(x):
        """torch's current stream of x's device, for the calls that take one.  Torch's default
        stream has the handle 0, which the library reads as "the table's own stream", and that
        stream (non-blocking) is not ordered after work queued on torch's default stream: wait
        for it here, so inputs a torch kernel is still writing are complete (the calls
        synchronise before they return anyway)."""
        import torch
        s = torch.cuda.current_stream(x.device)
        if not s.cuda_stream:
            s.synchronize()
        return ctypes.c_void_p(s.cuda_stream)

    def coalesce(self, keys):
        """keys: an int64 CUDA tensor of any shape; keys may repeat, -1 (~0) is padding.
        -> (uniq, inv, count): the distinct keys in first-occurrence order, for every position
        the index of its key in uniq (int64, -1 for padding; shaped like keys) and the number
        of occurrences of every distinct key (int64).  No row is read or changed."""
        import torch
        k = keys.contiguous().view(-1)
        n = k.numel()
        uniq = torch.empty(n, dtype=torch.int64, device=k.device)
        inv = torch.empty(n, dtype=torch.int32, device=k.device)
        count = torch.empty(n, dtype=torch.int32, device=k.device)
        nu = ctypes.c_uint64()
        check(capi.lib().swps_coalesce(self.h, ptr(k), n, ptr(uniq), ptr(inv), ptr(count), ctypes.byref(nu),
                                       self._stream(k)))
        return uniq[:nu.value], inv.to(torch.int64).view(keys.shape), count[:nu.value].to(torch.int64)

    def lookup(self, keys, insert=True, return_found=False):
        """The pull value of every position of `keys` (repeats allowed): an int64 CUDA tensor of any
        shape -> [*keys.shape, pull_elems] in the table dtype, on torch's current stream; a numpy
        array -> the host form (wire types: W2V fp64, LR fp32).  insert=True inserts every absent
        distinct key once, as `pull` of the distinct keys would; insert=False returns zeros for
        absent keys and padding.  return_found: also the per-position flags (uint8 / bool).  With
        admission on (`set_admission`) insert=True inserts only the ids that have come often enough;
        a refused id reads as zeros with found = 0."""
        lib = capi.lib()
        if hasattr(keys, "data_ptr"):
            import torch
            k = keys.contiguous().view(-1)
            n = k.numel()
            out = torch.empty((n, self.pull_elems), dtype=self.torch_dtype, device=k.device)
            found = torch.empty(n, dtype=torch.uint8, device=k.device) if return_found else None
            check(lib.swps_lookup(self.h, ptr(k), n, int(insert), ptr(out), ptr(found), self._stream(k)))
            out = out.view(*keys.shape, self.pull_elems)
            return (out, found.view(keys.shape)) if return_found else out
        k = self._keys_like(keys, False, None)
        shape = k.shape
        k = np.ascontiguousarray(k.reshape(-1))
        out = np.zeros((len(k), self.pull_elems), dtype=np.float64 if self.layout == "w2v" else np.float32)
        found = np.zeros(len(k), dtype=np.uint8)
        check(lib.swps_lookup_h(self.h, ptr(k), len(k), int(insert), ptr(out), ptr(found)))
        out = out.reshape(*shape, self.pull_elems)
        return (out, found.reshape(shape)) if return_found else out

    def push_dup(self, keys, grads, reduce="sum", scale=1.0):
        """One step of the push rule per DISTINCT key of `keys`, with the key's gradients combined
        in fp64 in ascending position (chunks of 128, each a chain from its first element, the chunk
        sums chained in order; reduce="mean" divides by the count once), times `scale`.  grads:
        [*keys.shape, push_elems], fp32 or fp64 (LR tables: fp32), never cast on the host.  CUDA
        tensors run on torch's current stream; numpy arrays take the host form (wire types).
        Padding (-1) positions are skipped; a key the table lacks raises SWPS_E_BADKEY after the
        other keys were applied (with admission on it is a refused id's gradient and only skipped)."""
        if reduce not in self._REDUCE:
            raise ValueError("reduce is 'sum' or 'mean'")
        lib = capi.lib()
        if hasattr(keys, "data_ptr"):
            import torch
            k = keys.contiguous().view(-1)
            g = grads.contiguous()
            if g.dtype not in (torch.float32, torch.float64):
                raise TypeError("grads must be float32 or float64")
            if g.numel() != k.numel() * self.push_elems:
                raise ValueError("grads must hold push_elems values per key")
            gd = capi.F64 if g.dtype == torch.float64 else capi.F32
            check(lib.swps_push_dup(self.h, ptr(k), k.numel(), ptr(g), gd, self._REDUCE[reduce], float(scale),
                                    self._stream(k)))
            return
        k = np.ascontiguousarray(self._keys_like(keys, False, None).reshape(-1))
        g = np.ascontiguousarray(grads, dtype=np.float64 if self.layout == "w2v" else np.float32)
        if g.size != len(k) * self.push_elems:
            raise ValueError("grads must hold push_elems values per key")
        check(lib.swps_push_dup_h(self.h, ptr(k), len(k), ptr(g), self._REDUCE[reduce], float(scale)))

    # ---- pooled lookups (swps_lookup_bag / swps_push_bag) ----
    _BAG = {"sum": capi.BAG_SUM, "mean": capi.BAG_MEAN, 0: 0, 1: 1}

    def _bag_args(self, keys, offsets, weights, mode):
        """(on_device, keys [n], offsets [nbags + 1], fp64 weights [n] or None) of the call's kind."""
        if mode not in self._BAG:
            raise ValueError("mode is 'sum' or 'mean'")
        if hasattr(keys, "data_ptr"):
            import torch
            if keys.dtype != torch.int64 or not hasattr(offsets, "data_ptr") or offsets.dtype != torch.int64:
                raise TypeError("keys and offsets must be int64 tensors")
            k = keys.contiguous().view(-1)
            off = offsets.to(k.device).contiguous().view(-1)
            w = None
            if weights is not None:
                if not weights.dtype.is_floating_point:
                    raise TypeError("weights must be a floating-point tensor")
                w = weights.to(device=k.device, dtype=torch.float64).contiguous().view(-1)  # exact; 8 n bytes
                if w.numel() != k.numel():
                    raise ValueError("weights must hold one value per key")
            if off.numel() < 1:
                raise ValueError("offsets must hold nbags + 1 entries")
            return True, k, off, w
        k = np.ascontiguousarray(self._keys_like(keys, False, None).reshape(-1))
        off = np.ascontiguousarray(np.asarray(offsets).reshape(-1)).astype(np.uint64)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if len(w) != len(k):
                raise ValueError("weights must hold one value per key")
        if len(off) < 1:
            raise ValueError("offsets must hold nbags + 1 entries")
        return False, k, off, w

    def lookup_bag(self, keys, offsets, weights=None, mode="sum", insert=True):
        """One pooled row per bag -> [nbags, pull_elems]: the sum (mode="mean": the mean over the
        bag's members) of the pull values of keys[offsets[b]:offsets[b + 1]], times weights[p] when
        given (sum only), accumulated in fp64 in the defined order of swps_lookup_bag (chunks of
        128 positions, each a chain from its first member) and cast to the table dtype once.
        offsets: nbags + 1 CSR entries (first 0, last n, never decreasing); -1 (~0) keys are padding;
        an empty bag is a zero row.  CUDA int64 tensors run on torch's current stream (weights of
        any float dtype are converted to fp64 on the device); numpy arrays take the host form
        (wire types: W2V fp64, LR fp32).  insert=True inserts every absent distinct key once, as
        `lookup` does; insert=False pools an absent key as a zero row that still counts."""
        dev, k, off, w = self._bag_args(keys, offsets, weights, mode)
        lib, nb = capi.lib(), len(off) - 1
        if dev:
            import torch
            out = torch.empty((nb, self.pull_elems), dtype=self.torch_dtype, device=k.device)
            check(lib.swps_lookup_bag(self.h, ptr(k), k.numel(), ptr(off), nb, ptr(w), self._BAG[mode], int(insert),
                                      ptr(out), self._stream(k)))
            return out
        out = np.zeros((nb, self.pull_elems), dtype=np.float64 if self.layout == "w2v" else np.float32)
        check(lib.swps_lookup_bag_h(self.h, ptr(k), len(k), ptr(off), nb, ptr(w), self._BAG[mode], int(insert),
                                    ptr(out)))
        return out

    def push_bag(self, keys, offsets, bag_grads, weights=None, mode="sum", scale=1.0):
        """The backward of `lookup_bag`: one step of the push rule per DISTINCT key.  bag_grads:
        [nbags, push_elems], fp32 or fp64 (LR tables: fp32).  Every occurrence of a key inherits
        its bag's gradient row (times weights[p]; mode="mean": divided by the bag's member count),
        and a key's terms are combined exactly as `push_dup(reduce="sum", scale)` combines the
        expanded fp64 [n, push_elems] matrix, which is never built.  Padding is skipped; a key the
        table lacks raises SWPS_E_BADKEY after the other keys were applied."""
        dev, k, off, w = self._bag_args(keys, offsets, weights, mode)
        lib, nb = capi.lib(), len(off) - 1
        if dev:
            import torch
            g = bag_grads.contiguous()
            if g.dtype not in (torch.float32, torch.float64):
                raise TypeError("bag_grads must be float32 or float64")
            if g.numel() != nb * self.push_elems:
                raise ValueError("bag_grads must hold push_elems values per bag")
            gd = capi.F64 if g.dtype == torch.float64 else capi.F32
            check(lib.swps_push_bag(self.h, ptr(k), k.numel(), ptr(off), nb, ptr(w), self._BAG[mode], ptr(g), gd,
                                    float(scale), self._stream(k)))
            return
        g = np.ascontiguousarray(bag_grads, dtype=np.float64 if self.layout == "w2v" else np.float32)
        if g.size != nb * self.push_elems:
            raise ValueError("bag_grads must hold push_elems values per bag")
        check(lib.swps_push_bag_h(self.h, ptr(k), len(k), ptr(off), nb, ptr(w), self._BAG[mode], ptr(g), float(scale)))

    # ---- top-k queries (swps_nearest / swps_analogy; collective on a routed table) ----
    _PARTS = {"h": 0, "v": 1, 0: 0, 1: 1}
    _METRICS = {"dot": capi.METRIC_DOT, "cos": capi.METRIC_COS, 0: 0, 1: 1}

    def _query_args(self, part, metric):
        # integer ids the library does not know pass through: it answers SWPS_E_CFG
        part, metric = self._PARTS.get(part, part), self._METRICS.get(metric, metric)
        if not isinstance(part, int) or not isinstance(metric, int):
            raise ValueError("part is 'h' or 'v', metric 'dot' or 'cos'")
        return part, metric

    @staticmethod
    def _keys_like(x, on_device, device):
        """x as a contiguous key array of the call's kind (None stays None)."""
        if x is None:
            return None
        if on_device:
            import torch
            if not hasattr(x, "data_ptr"):
                x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64))
            return x.to(device).contiguous()
        if hasattr(x, "data_ptr"):
            x = x.cpu().numpy()
        x = np.ascontiguousarray(x)
        return x.view(np.uint64) if x.dtype == np.int64 else x.astype(np.uint64, copy=False)

    def nearest(self, queries, k=10, part="v", metric="cos", exclude=None, candidates=None):
        """The k best rows per query under "higher score first, equal scores: smaller key first,
        NaN last" (swps_nearest).  queries: [nq, dim] fp32, a CUDA tensor or a numpy array; the
        answer (keys [nq, k], scores [nq, k]) is of the same kind (tensor keys are int64 views of
        the u64 keys).  exclude: [nq, <= 8] keys never returned for that query (~0 = unused);
        candidates: keys that restrict the search.  Fewer than k qualifying rows: the tail is key
        ~0, score -inf."""
        part, metric = self._query_args(part, metric)
        dev = hasattr(queries, "data_ptr")
        if dev:
            import torch
            q = queries.to(torch.float32).contiguous()
            nq = q.shape[0] if q.dim() == 2 else q.numel() // self.dim
            keys = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=q.device)
            scores = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=q.device)
            fn = capi.lib().swps_nearest
        else:
            q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
            nq = q.shape[0]
            keys = np.empty((nq, max(k, 0)), dtype=np.uint64)
            scores = np.empty((nq, max(k, 0)), dtype=np.float32)
            fn = capi.lib().swps_nearest_h
        excl = self._keys_like(exclude, dev, q.device if dev else None)
        cand = self._keys_like(candidates, dev, q.device if dev else None)
        nexcl = 0
        if excl is not None:
            excl = excl.reshape(nq, -1)
            nexcl = int(excl.shape[1])
        ncand = 0 if cand is None else int(cand.numel() if dev else cand.size)
        check(fn(self.h, part, metric, ptr(q), nq, k, ptr(excl), nexcl, ptr(cand), ncand, ptr(keys), ptr(scores)))
        return keys, scores

    def analogy(self, abc_keys, k=1, part="v", metric="cos", candidates=None):
        """For each (a, b, c) of abc_keys [nq, 3]: the k rows nearest to (b - a) + c (fp32, operands
        not normalised), a, b and c excluded (swps_analogy).  A CUDA tensor or a numpy array in,
        the same kind out; an unknown a / b / c raises SWPS_E_BADKEY."""
        part, metric = self._query_args(part, metric)
        dev = hasattr(abc_keys, "data_ptr")
        abc = self._keys_like(abc_keys, dev, abc_keys.device if dev else None).reshape(-1, 3)
        nq = int(abc.shape[0])
        cand = self._keys_like(candidates, dev, abc.device if dev else None)
        if dev:
            import torch
            keys = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=abc.device)
            scores = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=abc.device)
            fn = capi.lib().swps_analogy
        else:
            keys = np.empty((nq, max(k, 0)), dtype=np.uint64)
            scores = np.empty((nq, max(k, 0)), dtype=np.float32)
            fn = capi.lib().swps_analogy_h
        ncand = 0 if cand is None else int(cand.numel() if dev else cand.size)
        check(fn(self.h, part, metric, ptr(abc), nq, k, ptr(cand), ncand, ptr(keys), ptr(scores)))
        return keys, scores


KT_NAMES = ["plan", "forward", "sort", "gather", "push", "pull", "records"]


INTERMEDIATES = {False: 0, True: 1, "fp32": 0, "fp64": 1, "bfp40": 2, "bfp32": 3, 0: 0, 1: 1, 2: 2, 3: 3}


class Word2Vec:
    """CBOW negative-sampling word2vec (Word2Vec<MiniBatch>, word2vec_global.h:541-748).

    fp64_intermediates (fp32 tables): True / "fp64" = parity mode (neu1/neu1e and
    sums in fp64), False / "fp32" = fast mode (fp32 intermediates), "bfp40" /
    "bfp32" = block-floating-point neu1/neu1e rows (int32 + int8 / int32
    mantissas, one exponent per row) with fp64 sums (swps_w2v_bfp.h)."""

    def __init__(self, table, window=5, negative=5, min_sentence_length=1, minibatch=100, sample=1e-5, alpha=0.05,
                 unigram_size=int(1e8), key_mode="bkdr", init="ref", rand_seed=1, rand_offset=2, profile=False,
                 fp64_intermediates=True, minibatch_vocab=False, sampler="table", host_ingest=False):
        assert table.layout == "w2v"
        cfg = capi.W2VCfg(window, negative, min_sentence_length, minibatch, sample, alpha, unigram_size,
                          capi.KEY_ATOI if key_mode == "atoi" else capi.KEY_BKDR,
                          capi.W2V_INIT_REF if init == "ref" else capi.W2V_INIT_TABLE, rand_seed, rand_offset,
                          INTERMEDIATES[fp64_intermediates], int(profile), int(minibatch_vocab),
                          {"table": 0, "alias": 1}[sampler], int(host_ingest))
        h = ctypes.c_void_p()
        check(capi.lib().swps_w2v_create(table.h, ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        table._deps.add(self)
        self.table = table
        self.dim = table.dim
        self.key_mode = "atoi" if key_mode == "atoi" else "bkdr"

    def key_of(self, word):
        """The table key of a word string under the context's key mode (hash_fn / hash_fn2,
        word2vec_global.h:205-207, word2vec.h:221); integers are keys already."""
        if not isinstance(word, (str, bytes)):
            return int(word)
        if self.key_mode == "bkdr":
            return bkdr(word)
        import re
        m = re.match(r"\s*([+-]?\d+)", word if isinstance(word, str) else word.decode("utf-8", "replace"))
        return (int(m.group(1)) if m else 0) & 0xFFFFFFFFFFFFFFFF  # atoi

    def most_similar(self, words_or_keys, topn=10, part="v", metric="cos"):
        """The topn keys nearest to each word's own vector, the word itself excluded
        (Table.nearest on the HBM shard).  Words are strings (mapped by key_of) or keys; one word
        or a list.  Returns keys [n, topn] (uint64) — the library keeps no strings."""
        one = isinstance(words_or_keys, (str, bytes, int, np.integer))
        keys = np.array([self.key_of(w) for w in ([words_or_keys] if one else words_or_keys)], dtype=np.uint64)
        import torch
        dev = torch.device("cuda", self.table.device)
        dk = torch.from_numpy(keys.view(np.int64)).to(dev)
        D = self.dim
        off = Table._PARTS[part] * D
        q = self.table.export(dk)[:, off:off + D].to(torch.float32)
        out, _ = self.table.nearest(q, k=topn, part=part, metric=metric, exclude=dk.reshape(-1, 1))
        out = out.cpu().numpy().view(np.uint64)
        return out[0] if one else out

    def shard_comm(self, comm, frag_num=1000):
        """Library-driven key-sharded mode (swps_w2v_shard_comm): after load_*,
        init() is the first full pull and train_batches / train run lockstep
        minibatches over `comm` (collective).  The table must use init="hash"
        and this context init="table"."""
        check(capi.lib().swps_w2v_shard_comm(self.h, comm.h, frag_num))
        self._comm = comm

    def exchange_stats(self, on=-1):
        out = np.zeros(4)
        check(capi.lib().swps_w2v_exchange_stats(self.h, on, ptr(out)))
        return dict(zip(["bytes_remote", "bytes_total", "calls", "ms"], out.tolist()))

    @classmethod
    def from_config(cls, config, table_kwargs=None, **kw):
        """Build a Table + Word2Vec from the reference's demo.conf keys."""
        c = config if isinstance(config, Config) else Config(config)
        dim = c.get_int("word2vec", "len_vec")
        tk = dict(layout="w2v", dim=dim, learning_rate=c.get_float("server", "initial_learning_rate"))
        tk.update(table_kwargs or {})
        t = Table(**tk)
        args = dict(window=c.get_int("word2vec", "window"), negative=c.get_int("word2vec", "negative"),
                    min_sentence_length=c.get_int("word2vec", "min_sentence_length"),
                    minibatch=c.get_int("worker", "minibatch"), sample=c.get_float("word2vec", "sample"),
                    alpha=c.get_float("word2vec", "learning_rate"))
        args.update(kw)
        return cls(t, **args)

    def close(self):
        if getattr(self, "h", None):
            capi.lib().swps_w2v_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except (AttributeError, TypeError):  # interpreter shutdown: modules already torn down
            pass

    def load_text(self, path):
        check(capi.lib().swps_w2v_load_text(self.h, path.encode()))

    def load_tokens(self, word_ids, line_off, word_keys):
        word_ids = np.ascontiguousarray(word_ids, dtype=np.uint32)
        line_off = np.ascontiguousarray(line_off, dtype=np.uint64)
        word_keys = np.ascontiguousarray(word_keys, dtype=np.uint64)
        check(capi.lib().swps_w2v_load_tokens(self.h, ptr(word_ids), len(word_ids), ptr(line_off),
                                               len(line_off) - 1, ptr(word_keys), len(word_keys)))

    def info(self):
        o = np.zeros(8, dtype=np.uint64)
        check(capi.lib().swps_w2v_info(self.h, ptr(o)))
        return dict(zip(["vocab", "train_words", "lines", "tokens", "batches", "max_batch_tokens", "lstate",
                         "fstate"], [int(x) for x in o]))

    def vocab(self):
        V = self.info()["vocab"]
        keys = np.zeros(V, dtype=np.uint64)
        counts = np.zeros(V, dtype=np.int32)
        n = ctypes.c_uint64()
        check(capi.lib().swps_w2v_vocab(self.h, ptr(keys), ptr(counts), V, ctypes.byref(n)))
        return keys, counts

    def corpus(self):
        """(vid per token, line per token) — introspection for the ingest tests."""
        n = self.info()["tokens"]
        vid = np.zeros(max(n, 1), dtype=np.int32)
        line = np.zeros(max(n, 1), dtype=np.int32)
        check(capi.lib().swps_w2v_corpus(self.h, ptr(vid), ptr(line), len(vid)))
        return vid[:n], line[:n]

    def batch_keys(self, b):
        """(l0, l1, sorted vids of the gathered key set) of schedule batch b."""
        n = ctypes.c_uint64()
        lines = np.zeros(2, dtype=np.uint64)
        capi.lib().swps_w2v_batch_keys(self.h, b, None, 0, ctypes.byref(n), ptr(lines))
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        check(capi.lib().swps_w2v_batch_keys(self.h, b, ptr(out), len(out), ctypes.byref(n), ptr(lines)))
        return int(lines[0]), int(lines[1]), out[:n.value]

    def init(self):
        check(capi.lib().swps_w2v_init(self.h))

    def train_batches(self, count):
        check(capi.lib().swps_w2v_train_batches(self.h, count))

    def train(self, niters=1):
        check(capi.lib().swps_w2v_train_epochs(self.h, niters))

    def sync(self):
        check(capi.lib().swps_w2v_sync(self.h))

    def stats(self):
        o = np.zeros(10, dtype=np.uint64)
        check(capi.lib().swps_w2v_stats(self.h, ptr(o)))
        return dict(zip(["batches", "kept", "words", "pairs", "lstate", "fstate", "pulled", "pushed", "ctx_rows",
                         "tgt_rows"], [int(x) for x in o]))

    def gather_stats(self):
        """Cumulative gather work: gradient records summed and gather items (chunks)."""
        o = np.zeros(2, dtype=np.uint64)
        check(capi.lib().swps_w2v_gather_stats(self.h, ptr(o)))
        return {"records": int(o[0]), "items": int(o[1])}

    def sum_stats(self):
        """Cumulative gradient-sum work split by kernel: all records / items, the
        multi-chunk runs' records / items (k_gather_t's share when the push is fused),
        fused pushes and batches with sums."""
        o = np.zeros(8, dtype=np.uint64)
        check(capi.lib().swps_w2v_sum_stats(self.h, ptr(o)))
        return dict(zip(["records", "items", "multi_records", "multi_items", "fused", "batches", "fused_grads",
                         "split"], [int(x) for x in o]))

    def get_params(self):
        V = self.info()["vocab"]
        out = np.zeros((V, 4 * self.dim), dtype=np.float64)
        check(capi.lib().swps_w2v_get_params(self.h, ptr(out)))
        return out

    def set_params(self, hv):
        hv = np.ascontiguousarray(hv, dtype=np.float64)
        check(capi.lib().swps_w2v_set_params(self.h, ptr(hv)))

    def unigram_at(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.zeros(len(idx), dtype=np.uint32)
        check(capi.lib().swps_w2v_unigram_at(self.h, ptr(idx), len(idx), ptr(out)))
        return out

    def trace_negatives(self, cap):
        check(capi.lib().swps_w2v_trace_negatives(self.h, cap))

    def negatives(self, cap):
        out = np.zeros(max(cap, 1), dtype=np.int64)
        n = ctypes.c_uint64()
        check(capi.lib().swps_w2v_negatives(self.h, ptr(out), cap, ctypes.byref(n)))
        return out[:n.value]

    def kernel_times(self, reset=False):
        o = np.zeros(2 * len(KT_NAMES), dtype=np.float64)
        check(capi.lib().swps_w2v_kernel_times(self.h, ptr(o), int(reset)))
        return {k: (o[2 * i], int(o[2 * i + 1])) for i, k in enumerate(KT_NAMES)}

    def set_profile(self, on):
        check(capi.lib().swps_w2v_set_profile(self.h, int(on)))

    def stream(self):
        return capi.lib().swps_w2v_stream(self.h)

    def save_state(self, path):
        """Worker checkpoint: batch cursor, RNG streams, counters, cache."""
        check(capi.lib().swps_w2v_save_state(self.h, path.encode()))

    def restore_state(self, path):
        """Resume a fresh context (corpus loaded, not initialised) whose table
        already holds the vocab rows."""
        check(capi.lib().swps_w2v_restore_state(self.h, path.encode()))

    def save(self, prefix):
        """Exact resume point: <prefix>.table (the shard) + <prefix>.w2v."""
        self.sync()
        self.table.save(prefix + ".table")
        self.save_state(prefix + ".w2v")

    def restore(self, prefix):
        self.table.restore(prefix + ".table")
        self.restore_state(prefix + ".w2v")


class Sent2Vec:
    """Sentence vectors against frozen word vectors (Sent2Vec, sent2vec.cpp:14-195,
    on word2vec.h's MiniBatch: per-minibatch vocab and unigram table).

    glibc rand() bookkeeping (the sentence vectors and the rows of keys a pull
    misses come from it): ``rand_offset`` = calls before load_word_vector (the
    two port binds by default); ``rand_insert_extra`` = extra calls per key the
    server inserts — 0 for a map that does not construct a value on insert,
    2*dim for sparsehash's dense_hash_map::operator[] (then also add 2*dim per
    SparseTable shard to ``rand_offset`` for set_empty_key)."""

    def __init__(self, table, window=5, negative=5, min_sentence_length=1, minibatch=100, niters=1, alpha=0.05,
                 unigram_size=int(1e8), rand_seed=1, rand_offset=2, rand_insert_extra=0, profile=False):
        assert table.layout == "w2v"
        self.table = table
        self.dim = table.dim
        self.kw = dict(window=window, negative=negative, min_sentence_length=min_sentence_length,
                       minibatch=minibatch, niters=niters, alpha=alpha, unigram_size=unigram_size,
                       rand_seed=rand_seed, rand_insert_extra=rand_insert_extra, profile=int(profile))
        self.rand_offset = rand_offset
        self.h = None

    @classmethod
    def from_config(cls, config, table, niters, **kw):
        c = config if isinstance(config, Config) else Config(config)
        args = dict(window=c.get_int("word2vec", "window"), negative=c.get_int("word2vec", "negative"),
                    min_sentence_length=c.get_int("word2vec", "min_sentence_length"),
                    minibatch=c.get_int("worker", "minibatch"), alpha=c.get_float("word2vec", "learning_rate"),
                    niters=niters)
        args.update(kw)
        return cls(table, **args)

    def load_word_vector(self, path, frag_num=1000, world=1, node_id=0):
        """ClusterServer::load (server.h:49-62): one WParam (2*dim rand()) is
        constructed first, then every owned key of the dump is assigned."""
        before = self.table.size()
        self.table.load(path, frag_num, world, node_id)
        inserted = self.table.size() - before
        self.rand_offset += 2 * self.dim + self.kw["rand_insert_extra"] * inserted

    def _create(self):
        if self.h is None:
            k = self.kw
            cfg = capi.S2VCfg(k["window"], k["negative"], k["min_sentence_length"], k["minibatch"], k["niters"],
                              k["alpha"], k["unigram_size"], k["rand_seed"], self.rand_offset,
                              k["rand_insert_extra"], k["profile"])
            h = ctypes.c_void_p()
            check(capi.lib().swps_s2v_create(self.table.h, ctypes.byref(cfg), ctypes.byref(h)))
            self.h = h
            self.table._deps.add(self)
            if getattr(self, "_shard", None):
                check(capi.lib().swps_s2v_shard(self.h, *self._shard))

    def close(self):
        if getattr(self, "h", None):
            capi.lib().swps_s2v_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except (AttributeError, TypeError):  # interpreter shutdown: modules already torn down
            pass

    def load_text(self, path):
        self._create()
        check(capi.lib().swps_s2v_load_text(self.h, path.encode()))

    def load_tokens(self, tok_keys, line_off, sent_ids):
        self._create()
        tok_keys = np.ascontiguousarray(tok_keys, dtype=np.uint64)
        line_off = np.ascontiguousarray(line_off, dtype=np.uint64)
        sent_ids = np.ascontiguousarray(sent_ids, dtype=np.uint64)
        assert len(sent_ids) == len(line_off) - 1
        check(capi.lib().swps_s2v_load_tokens(self.h, ptr(tok_keys), len(tok_keys), ptr(line_off),
                                               len(line_off) - 1, ptr(sent_ids)))

    def run_tokens(self, tok_keys, line_off, sent_ids):
        """The reference's single pass (Sent2Vec::train, sent2vec.cpp:95-103): load and train every
        minibatch once, the host's per-minibatch work overlapped with the GPU's training
        (swps_s2v_run_tokens; = load_tokens + train bit for bit)."""
        self._create()
        tok_keys = np.ascontiguousarray(tok_keys, dtype=np.uint64)
        line_off = np.ascontiguousarray(line_off, dtype=np.uint64)
        sent_ids = np.ascontiguousarray(sent_ids, dtype=np.uint64)
        assert len(sent_ids) == len(line_off) - 1
        check(capi.lib().swps_s2v_run_tokens(self.h, ptr(tok_keys), len(tok_keys), ptr(line_off),
                                              len(line_off) - 1, ptr(sent_ids)))

    def shard(self, rank, world, frag_num=1000):
        """Keep only the documents BasicHashFrag assigns to `rank` (call before
        loading; config 5's doc-sharded layout, no exchange)."""
        self._shard = (rank, world, frag_num)

    def info(self):
        o = np.zeros(9, dtype=np.uint64)
        check(capi.lib().swps_s2v_info(self.h, ptr(o)))
        return dict(zip(["lines", "docs", "batches", "tokens", "inserted", "max_batch_docs", "max_batch_records",
                         "rand_calls", "lstate"], [int(x) for x in o]))

    def train(self):
        check(capi.lib().swps_s2v_train(self.h))

    def train_batches(self, count):
        check(capi.lib().swps_s2v_train_batches(self.h, count))

    def sync(self):
        check(capi.lib().swps_s2v_sync(self.h))

    def docs(self):
        """(sentence ids, vectors [n, dim] fp64, per-sentence g*g of the last pass)."""
        n = self.info()["docs"]
        ids = np.zeros(max(n, 1), dtype=np.uint64)
        vecs = np.zeros((max(n, 1), self.dim), dtype=np.float64)
        errs = np.zeros(max(n, 1), dtype=np.float32)
        m = ctypes.c_uint64()
        check(capi.lib().swps_s2v_docs(self.h, ptr(ids), ptr(vecs), ptr(errs), len(ids), ctypes.byref(m)))
        return ids[:n], vecs[:n], errs[:n]

    def error(self):
        """Error::norm() of the run (sent2vec.cpp:80,105): float mean of g*g."""
        _, _, errs = self.docs()
        acc = np.float32(0)
        for e in errs:
            acc = np.float32(acc + e)
        return float(acc / np.float32(len(errs))) if len(errs) else float("nan")

    def dump(self, path):
        check(capi.lib().swps_s2v_dump(self.h, path.encode()))

    def stats(self):
        o = np.zeros(5, dtype=np.uint64)
        check(capi.lib().swps_s2v_stats(self.h, ptr(o)))
        return dict(zip(["batches", "docs", "positions", "ctx_rows", "tgt_rows"], [int(x) for x in o]))

    def set_profile(self, on):
        check(capi.lib().swps_s2v_set_profile(self.h, int(on)))

    def kernel_times(self, reset=False):
        o = np.zeros(4, dtype=np.float64)
        check(capi.lib().swps_s2v_kernel_times(self.h, ptr(o), int(reset)))
        return {k: (o[2 * i], int(o[2 * i + 1])) for i, k in enumerate(["records", "docs"])}

    def stream(self):
        return capi.lib().swps_s2v_stream(self.h)


class LR:
    """Sparse logistic regression with server-side AdaGrad (lr.cpp:133-411)."""

    def __init__(self, table, minibatch=200, init_ref=True, profile=False, fast_sums=False, plan="step"):
        """plan: "step" builds each minibatch's index inside its step (beside the previous step,
        lr.cpp:215-227's per-minibatch gather; single GPU with fast_sums), "load" every
        minibatch's index once at load (reused each epoch).  Same results."""
        assert table.layout == "lr"
        plans = {"step": capi.LR_PLAN_STEP, "load": capi.LR_PLAN_LOAD, "none": capi.LR_PLAN_NONE}
        if plan not in plans:
            raise ValueError("unknown plan %r (step, load or none)" % (plan,))
        cfg = capi.LRCfg(minibatch, int(init_ref), int(profile), int(fast_sums), plans[plan])
        h = ctypes.c_void_p()
        check(capi.lib().swps_lr_create(table.h, ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        table._deps.add(self)
        self.table = table

    def shard_comm(self, comm, frag_num=2000):
        """Library-driven key-sharded LR (swps_lr_shard_comm): init / train /
        train_batches / predict become collective over `comm`."""
        check(capi.lib().swps_lr_shard_comm(self.h, comm.h, frag_num))
        self._comm = comm

    def exchange_stats(self, on=-1):
        """As Word2Vec.exchange_stats (swps_lr_exchange_stats)."""
        out = np.zeros(4)
        check(capi.lib().swps_lr_exchange_stats(self.h, on, ptr(out)))
        return dict(zip(["bytes_remote", "bytes_total", "calls", "ms"], out.tolist()))

    def plan_info(self):
        """swps_lr_plan_info: the plan the step runs and the fixed point's scale against its floor
        (fallback True: plan "none" was asked for, heavy-tailed x_i put the scale below the floor,
        and the load switched to plan "step", fp64 sums)."""
        o = np.zeros(5, dtype=np.int32)
        check(capi.lib().swps_lr_plan_info(self.h, ptr(o)))
        names = {0: "step", 1: "load", 2: "none"}
        return {"plan": names.get(int(o[0]), int(o[0])), "plan_asked": names.get(int(o[1]), int(o[1])),
                "fx_bits": int(o[2]), "fx_floor": int(o[3]), "fallback": bool(o[4])}

    def fx_bytes(self, batch):
        """The fixed-point step's algorithmic bytes on `batch` (swps_lr_fx_bytes): a dict with
        step / push bytes, form (1 bucketed, 2 atomic, 0 other plan), hot, buckets, blocks,
        nonhot records, distinct nonhot keys."""
        out = np.zeros(8, dtype=np.uint64)
        check(capi.lib().swps_lr_fx_bytes(self.h, batch, ptr(out)))
        return dict(zip(["step", "push", "form", "hot", "buckets", "blocks", "nonhot", "uniq"],
                        [int(x) for x in out]))

    def close(self):
        if getattr(self, "h", None):
            capi.lib().swps_lr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except (AttributeError, TypeError):  # interpreter shutdown: modules already torn down
            pass

    def load_text(self, path):
        check(capi.lib().swps_lr_load_text(self.h, path.encode()))

    def load_csr(self, labels, row_off, feat, vals):
        labels = np.ascontiguousarray(labels, dtype=np.float32)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        feat = np.ascontiguousarray(feat, dtype=np.uint32)
        vals = np.ascontiguousarray(vals, dtype=np.float32)
        check(capi.lib().swps_lr_load_csr(self.h, ptr(labels), len(labels), ptr(row_off), ptr(feat), ptr(vals)))

    def init(self):
        check(capi.lib().swps_lr_init(self.h))

    def train(self, niters):
        err = np.zeros(niters, dtype=np.float64)
        check(capi.lib().swps_lr_train(self.h, niters, ptr(err)))
        return err

    def train_batches(self, count):
        check(capi.lib().swps_lr_train_batches(self.h, count))

    def sync(self):
        check(capi.lib().swps_lr_sync(self.h))

    def info(self):
        o = np.zeros(4, dtype=np.uint64)
        check(capi.lib().swps_lr_info(self.h, ptr(o)))
        return dict(zip(["rows", "keys", "batches", "nnz"], [int(x) for x in o]))

    def predict(self):
        n = self.info()["rows"]
        p = np.zeros(n, dtype=np.float32)
        t = np.zeros(n, dtype=np.float32)
        check(capi.lib().swps_lr_predict(self.h, ptr(p), ptr(t), n))
        return p, t

    def params(self):
        n = self.info()["keys"]
        keys = np.zeros(max(n, 1), dtype=np.uint32)
        w = np.zeros(max(n, 1), dtype=np.float32)
        g2 = np.zeros(max(n, 1), dtype=np.float32)
        m = ctypes.c_uint64()
        check(capi.lib().swps_lr_params(self.h, ptr(keys), ptr(w), ptr(g2), len(keys), ctypes.byref(m)))
        return keys[:m.value], w[:m.value], g2[:m.value]

    def set_profile(self, on):
        check(capi.lib().swps_lr_set_profile(self.h, int(on)))

    def kernel_times(self, reset=False):
        o = np.zeros(8, dtype=np.float64)
        check(capi.lib().swps_lr_kernel_times(self.h, ptr(o), int(reset)))
        return {k: (o[2 * i], int(o[2 * i + 1])) for i, k in enumerate(["forward", "sort", "gather", "push"])}
