"""Time the removal of keys from the HBM shard (swps_erase / swps_prune) beside
the only thing a caller could do before them: export the survivors, destroy the table, create it
again and assign.  Not part of bench.py; no pass/fail bar.

    python scripts/table_erase_bench.py [--out FILE] [--reps 7]

Shapes: (w2v) V = 71 290 keys at D = 300 fp32, scripts/table_grow_bench.py's table; (lr) 2^20 LR
keys fp32.  At 1 %, 10 % and 50 % of the keys removed (a seeded shuffle picks them), wall time
around synchronous calls with torch.cuda.synchronize() before each clock read, 2 warm-up runs,
median and minimum of --reps.  Every run starts from a fresh table (outside the clock): all keys
pulled, then a non-zero gradient pushed to the keys that will survive, so that prune(0) removes
exactly the keys erase is given.
  erase    Table.erase of the key list (already on the device)
  prune    Table.prune(0.0)
  rebuild  keys(), the survivors picked on the host (numpy.isin) and uploaded, export of their rows,
           close, a new table of the same capacity, assign.  This leg calls nothing newer than
           assign / export / keys, so it measures the parent commit's only remedy, not this code.
Bytes model per erase: rows moved x (row bytes + 8) x 2, the slot fill (12 B per slot), the rehash
(20 B per survivor, scattered); prune adds the accumulator half of every row read."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"w2v": dict(layout="w2v", dim=300, n=71290), "lr": dict(layout="lr", dim=1, n=1 << 20)}
SHARES = (0.01, 0.10, 0.50)


def keys_of(n):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761)


def slots_of(capacity):
    ns = 1
    while ns < 2 * capacity:
        ns <<= 1
    return ns


def run_share(sw, name, share, reps, warmup):
    import torch
    sh = SHAPES[name]
    n = sh["n"]
    keys = keys_of(n)
    gone = np.random.default_rng(15).permutation(keys)[:int(round(share * n))]
    live = keys[~np.isin(keys, gone)]
    dk = torch.as_tensor(keys.view(np.int64)).to("cuda")
    dgone = torch.as_tensor(gone.view(np.int64)).to("cuda")
    dlive = torch.as_tensor(live.view(np.int64)).to("cuda")
    w2v = sh["layout"] == "w2v"
    grads = torch.full((len(live), 2 * sh["dim"] if w2v else 1), 0.25, dtype=torch.float64 if w2v else torch.float32,
                       device="cuda")
    row_bytes = (4 * sh["dim"] if w2v else 2) * 4

    def fresh():
        t = sw.Table(sh["layout"], dim=sh["dim"], capacity=n, dtype="f32", init="hash", seed=1)
        t.pull(dk)
        t.push(dlive, grads)
        return t

    def timed(leg):
        ms, moves = [], None
        for i in range(warmup + reps):
            t = fresh()
            if moves is None and leg == "erase":
                moves = len(sw.erase_plan(np.isin(t.keys(), gone))[1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if leg == "erase":
                got = t.erase(dgone)
            elif leg == "prune":
                got = t.prune(0.0)
            else:
                ks = t.keys()
                keep = torch.as_tensor(ks[~np.isin(ks, gone)].view(np.int64)).to("cuda")
                rows = t.export(keep)
                t.close()
                t = sw.Table(sh["layout"], dim=sh["dim"], capacity=n, dtype="f32", init="hash", seed=1)
                t.assign(keep, rows)
                got = len(gone)
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            assert got == len(gone) and t.size() == len(live), (leg, got, t.size())
            t.close()
        return float(np.median(ms)), float(np.min(ms)), moves

    out = dict(shape=name, keys=n, share=share, erased=len(gone), row_bytes=row_bytes, slots=slots_of(n))
    for leg in ("erase", "prune", "rebuild"):
        med, mn, moves = timed(leg)
        out[leg + "_ms"] = round(med, 3)
        out[leg + "_min_ms"] = round(mn, 3)
        if moves is not None:
            out["moves"] = moves
    moved = 2 * out["moves"] * (row_bytes + 8)
    index = out["slots"] * 12 + len(live) * 20
    out["erase_bytes"] = moved + index
    out["moved_bytes"] = moved
    out["index_bytes"] = index
    out["prune_bytes"] = moved + index + n * row_bytes // 2
    out["rebuild_bytes"] = 2 * 2 * len(live) * (row_bytes + 8) + index  # export + assign, read + written each
    out["erase_vs_rebuild"] = round(out["erase_ms"] / out["rebuild_ms"], 3)
    out["prune_vs_rebuild"] = round(out["prune_ms"] / out["rebuild_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="w2v,lr")
    a = ap.parse_args()
    import swiftmpi_amd as sw
    res = []
    for name in a.shapes.split(","):
        for share in SHARES:
            r = run_share(sw, name, share, a.reps, a.warmup)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
