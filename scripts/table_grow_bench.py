"""Time the growth of the HBM shard (swps_table_set_max_capacity / swps_table_reserve, DESIGN.md
section 12) beside a table created at full size.  Not part of bench.py; no pass/fail bar.

    python scripts/table_grow_bench.py [--out FILE] [--reps 7]

Shapes: (w2v) V = 71 290 keys at D = 300 fp32, scripts/nearest_bench.py's table; (lr) 2^20 LR keys.
For each shape, wall time around synchronous calls (every pull ends in the table's error check,
which synchronises its stream; torch.cuda.synchronize() before each clock read), 2 warm-up runs,
median of --reps:
  grow   the table created with capacity 1024 under a ceiling, filled through pulls of 4096 keys
  full   the same pulls into a table created at full size (all the parent commit can do)
  move   the last, largest move alone: a fixed table at the capacity and row count the growing
         table had before its last move, then one swps_table_reserve to the capacity after it.
         Bytes = the row_key and rows entries copied (read + written) plus the new slot arrays
         (memset, then the rehash's scattered CAS and store per row); rate = bytes / time.
A table create and destroy are inside the grow / full times (hipMalloc and hipFree are what a user
pays too); the keys are on the device before the clock starts.
Sanity line: tables created as bench.py creates them (no ceiling) report growths == 0."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"w2v": dict(layout="w2v", dim=300, n=71290, ceiling=1 << 17),
          "lr": dict(layout="lr", dim=1, n=1 << 20, ceiling=1 << 21)}
START, CHUNK = 1024, 4096


def keys_of(n):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761)


def slots_of(capacity):
    ns = 1
    while ns < 2 * capacity:
        ns <<= 1
    return ns


def table(sw, sh, capacity, ceiling=None):
    return sw.Table(sh["layout"], dim=sh["dim"], capacity=capacity, max_capacity=ceiling, dtype="f32", init="hash",
                    seed=1)


def fill(t, chunks, trace=None):
    for c in chunks:
        before = t.capacity() if trace is not None else None
        t.pull(c)
        if trace is not None:
            after = t.capacity()
            if after["growths"] != before["growths"]:
                trace.append((before["capacity"], t.size() - c.numel(), after["capacity"], after["slots"]))


def wall(fn, reps, warmup):
    import torch
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out))


def run_shape(sw, name, reps, warmup):
    import torch
    sh = SHAPES[name]
    n = sh["n"]
    dk = torch.as_tensor(keys_of(n).view(np.int64)).to("cuda")
    chunks = [dk[a:a + CHUNK] for a in range(0, n, CHUNK)]
    row_bytes = (4 * sh["dim"] if sh["layout"] == "w2v" else 2) * 4

    trace = []
    t = table(sw, sh, START, sh["ceiling"])
    fill(t, chunks, trace)
    cap = t.capacity()
    assert t.size() == n and cap["growths"] == len(trace) and cap["capacity"] >= n, cap
    ref = table(sw, sh, n)
    fill(ref, chunks)
    probe = dk[torch.randperm(n, device="cuda")[:5000]]
    assert torch.equal(t.pull(probe), ref.pull(probe)) and ref.capacity()["growths"] == 0
    t.close()
    ref.close()

    def grow():
        x = table(sw, sh, START, sh["ceiling"])
        fill(x, chunks)
        x.close()

    def full():
        x = table(sw, sh, n)
        fill(x, chunks)
        x.close()
    g_med, g_min = wall(grow, reps, warmup)
    f_med, f_min = wall(full, reps, warmup)

    cap0, rows0, cap1, slots1 = trace[-1]
    ms = []
    for i in range(warmup + reps):
        x = table(sw, sh, cap0)
        x.pull(dk[:rows0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x.reserve(cap1)
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
        assert x.capacity()["capacity"] == cap1 and x.size() == rows0
        x.close()
    m_med = float(np.median(ms))
    copied = 2 * rows0 * (row_bytes + 8)
    index = slots1 * 12 + rows0 * (8 + 8 + 4)
    return dict(shape=name, keys=n, row_bytes=row_bytes, start=START, chunk=CHUNK, ceiling=sh["ceiling"],
                growths=len(trace), capacities=[START] + [x[2] for x in trace], final_capacity=cap["capacity"],
                grow_ms=round(g_med, 2), grow_min_ms=round(g_min, 2), full_ms=round(f_med, 2),
                full_min_ms=round(f_min, 2), ratio=round(g_med / f_med, 3),
                last_move=dict(capacity_before=cap0, rows=rows0, capacity_after=cap1, slots_after=slots1,
                               ms=round(m_med, 3), min_ms=round(float(np.min(ms)), 3), bytes=copied + index,
                               copied_bytes=copied, gb_per_s=round((copied + index) / m_med / 1e6, 1),
                               new_bytes=cap1 * (row_bytes + 8) + slots1 * 12,
                               old_bytes=cap0 * (row_bytes + 8) + slots_of(cap0) * 12))


def sanity(sw):
    """Tables as bench.py creates them: fixed capacity, hash init, no ceiling."""
    import torch
    out = {}
    for name, kw, n in (("w2v", dict(dim=300, capacity=71290), 71290), ("lr", dict(capacity=1 << 23), 1 << 20)):
        t = sw.Table(name, dtype="f32", init="hash", seed=1, **kw)
        t.pull(torch.as_tensor(keys_of(n).view(np.int64)).to("cuda"))
        c = t.capacity()
        assert c["growths"] == 0 and c["max_capacity"] == 0 and c["capacity"] == kw["capacity"], c
        out[name] = c
        t.close()
    print("sanity: bench.py-style tables (no ceiling) growths == 0:", json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="w2v,lr")
    a = ap.parse_args()
    import swiftmpi_amd as sw
    res = dict(sanity=sanity(sw), shapes=[])
    for name in a.shapes.split(","):
        r = run_shape(sw, name, a.reps, a.warmup)
        print(json.dumps(r))
        res["shapes"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
