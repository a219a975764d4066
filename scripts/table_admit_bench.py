"""Time the inserting lookup of the HBM table over a stream of Zipf ids with admission by count
(swps_table_set_admission) off and on, beside another build of the library
(the parent commit's) on the same batches.  Not part of bench.py; no pass/fail bar.

    python scripts/table_admit_bench.py [--parent-lib FILE] [--out FILE] [--reps 7]

Stream: --batches batches of --n ids drawn Zipf(--zipf) from a universe of --universe ids; a W2V fp32
table at D = --dim.  Two settings: "growing" (capacity 2^14 under a ceiling of the universe: the
table moves as it fills) and "reserved" (the universe's capacity from the start: no move, so the
legs differ by the gate alone).  Legs, each a FRESH table that plays the whole stream:
  parent  swps_lookup(insert = 1) of the library given by --parent-lib (skipped without it)
  off     this build, admission off
  on      this build, swps_table_set_admission(--min-count, --width)
All legs go through the same few ctypes calls (no Python wrapper in the clock); wall time around the
stream with torch.cuda.synchronize() before each clock read; --warmup unclocked rounds, then --reps
rounds with the legs interleaved leg by leg inside every round.  Reported per leg: median, minimum
and maximum over the rounds of the time per lookup (stream time / batches), rows held and moves of
the shard at the end; off / parent and on / parent are ratios of medians, beside the legs' own
max / min spread."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Lib:
    """The few calls of the C ABI the legs need, from any build of libswps.so."""
    NAMES = ("swps_last_error", "swps_table_create", "swps_table_destroy", "swps_table_size", "swps_table_capacity",
             "swps_table_set_max_capacity", "swps_lookup")

    def __init__(self, path, admission):
        from swiftmpi_amd import capi
        self.capi = capi
        self.L = ctypes.CDLL(path)
        for name in self.NAMES + (("swps_table_set_admission",) if admission else ()):
            f = getattr(self.L, name)
            f.restype, f.argtypes = capi.PROTOS[name]

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("%d: %s" % (rc, self.L.swps_last_error().decode(errors="replace")))

    def table(self, dim, capacity, ceiling, min_count, width):
        capi = self.capi
        cfg = capi.TableCfg(0, capi.LAYOUT_W2V, capi.F32, dim, capacity, 0.7, 1e-6, capi.INIT_HASH, 1, capi.PUSH_ADAGRAD)
        h = ctypes.c_void_p()
        self.check(self.L.swps_table_create(ctypes.byref(cfg), ctypes.byref(h)))
        if ceiling:
            self.check(self.L.swps_table_set_max_capacity(h, ceiling))
        if min_count:
            self.check(self.L.swps_table_set_admission(h, min_count, width))
        return h

    def lookup(self, h, ids, out):
        self.check(self.L.swps_lookup(h, ctypes.c_void_p(ids.data_ptr()), ids.numel(), 1, ctypes.c_void_p(out.data_ptr()),
                                      None, None))

    def end(self, h):
        n = ctypes.c_uint64()
        cap = np.zeros(4, dtype=np.uint64)
        self.check(self.L.swps_table_size(h, ctypes.byref(n)))
        self.check(self.L.swps_table_capacity(h, cap.ctypes.data_as(ctypes.c_void_p)))
        self.check(self.L.swps_table_destroy(h))
        return int(n.value), int(cap[3])


def zipf_batches(universe, n, batches, s, seed):
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(1.0 / np.arange(1, universe + 1) ** s)
    cdf /= cdf[-1]
    keys = (np.arange(1, universe + 1, dtype=np.uint64) * np.uint64(2654435761)).view(np.int64)
    return [keys[np.minimum(np.searchsorted(cdf, rng.random(n)), universe - 1)] for _ in range(batches)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=1 << 17)
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--zipf", type=float, default=1.05)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--width", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    from swiftmpi_amd import capi
    assert torch.cuda.is_available(), "needs the GPU"
    new = Lib(capi.LIB_PATH, True)
    legs = [("off", new, 0), ("on", new, a.min_count)]
    if a.parent_lib:
        legs.insert(0, ("parent", Lib(a.parent_lib, False), 0))
    host = zipf_batches(a.universe, a.n, a.batches, a.zipf, 16)
    seen = np.unique(np.concatenate(host))
    stream = [torch.as_tensor(b).to("cuda") for b in host]
    out = torch.empty((a.n, 2 * a.dim), dtype=torch.float32, device="cuda")
    res = []
    for setting, cap, ceiling in (("growing", 1 << 14, a.universe), ("reserved", a.universe, 0)):
        ms = {name: [] for name, _, _ in legs}
        ends = {}
        for r in range(a.warmup + a.reps):
            for name, lib, mc in legs:
                h = lib.table(a.dim, cap, ceiling, mc, a.width)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for ids in stream:
                    lib.lookup(h, ids, out)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3 / len(stream)
                ends[name] = lib.end(h)
                if r >= a.warmup:
                    ms[name].append(dt)
        row = dict(setting=setting, n=a.n, batches=a.batches, universe=a.universe, zipf=a.zipf, dim=a.dim,
                   min_count=a.min_count, width=a.width, reps=a.reps, distinct_ids=int(len(seen)))
        for name, _, _ in legs:
            v = ms[name]
            row[name] = dict(ms_per_lookup=round(float(np.median(v)), 4), min_ms=round(float(np.min(v)), 4),
                             max_ms=round(float(np.max(v)), 4), spread=round(float(np.max(v) / np.min(v)), 3),
                             rows=ends[name][0], moves=ends[name][1])
        base = "parent" if a.parent_lib else "off"
        for name in ("off", "on"):
            if name != base:
                row[name + "_vs_" + base] = round(row[name]["ms_per_lookup"] / row[base]["ms_per_lookup"], 3)
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
