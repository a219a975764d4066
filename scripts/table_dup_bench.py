"""Time the repeated-key calls of the HBM table (swps_coalesce / swps_lookup / swps_push_dup,
DESIGN.md section 13) beside what a user composes from torch and the distinct-key calls.  Not
part of bench.py; no pass/fail bar.

    python scripts/table_dup_bench.py [--out FILE] [--reps 7]

Shapes: (w2v-zipf, w2v-uniform) scripts/nearest_bench.py's table, V = 71 290 keys at D = 300 fp32,
with n = 2^20 ids drawn Zipf(1) / uniformly; (lr) an LR table of 2^20 keys with n = 2^22 uniform
ids.  Gradients are fp32.  Every key is in the table before the clock starts (the steady state of
a training loop); `lookup_cold` is the one lookup into an empty table that inserts every key.
  fused     Table.lookup(ids) / Table.push_dup(ids, grads)
  composed  torch.unique(ids, return_inverse=True) + Table.pull(uniq)[inv]
            zeros(U, push, wire dtype).index_add_(0, inv, grads) + a device sync + Table.push(uniq, buf)
            (Table.push works on the table's own stream, not on torch's)
Wall time around synchronous calls, torch.cuda.synchronize() before each clock read, 2 warm-ups,
median of --reps, the two sides interleaved run by run in one process.  `coalesce` is
swps_coalesce alone (the sort, the scan and the first-occurrence rank); the rest of a fused call is
the find / insert of the distinct keys plus the gather.  A push runs the sort and the scan but not
the rank (it needs no first-occurrence order), so its time is not split against `coalesce`.
Bytes by the model of DESIGN.md section 13 (the sort: 8 onesweep passes reading and writing 12 n
bytes); rate = bytes / fused time, beside the 8 TB/s HBM peak."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12
SHAPES = {"w2v-zipf": dict(layout="w2v", dim=300, V=71290, n=1 << 20, zipf=True),
          "w2v-uniform": dict(layout="w2v", dim=300, V=71290, n=1 << 20, zipf=False),
          "lr": dict(layout="lr", dim=1, V=1 << 20, n=1 << 22, zipf=False)}


def keys_of(n):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761)


def draw(sh, seed):
    rng = np.random.default_rng(seed)
    V, n = sh["V"], sh["n"]
    if sh["zipf"]:
        p = 1.0 / np.arange(1, V + 1)
        return rng.choice(V, n, p=p / p.sum())
    return rng.integers(0, V, n)


def timed(fns, reps, warmup):
    """Median wall ms of each function, interleaved: one run of each per round."""
    import torch
    out = [[] for _ in fns]
    for i in range(warmup + reps):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                out[j].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(x)) for x in out]


def run_shape(sw, name, reps, warmup):
    import torch
    from swiftmpi_amd import capi
    sh = SHAPES[name]
    V, n, w2v = sh["V"], sh["n"], sh["layout"] == "w2v"
    pool = keys_of(V)
    ids = torch.as_tensor(pool[draw(sh, 1)].view(np.int64)).to("cuda")
    allk = torch.as_tensor(pool.view(np.int64)).to("cuda")

    def table():
        return sw.Table(sh["layout"], dim=sh["dim"], capacity=V, dtype="f32", init="hash", seed=1)
    a, b = table(), table()
    a.pull(allk)
    b.pull(allk)
    P = a.push_elems
    grads = torch.randn((n, P), dtype=torch.float32, device="cuda") * 0.1
    wire = torch.float64 if w2v else torch.float32

    # ---- the two sides agree ----
    uniq, inv = torch.unique(ids, return_inverse=True)
    U = int(uniq.numel())
    assert torch.equal(a.lookup(ids), b.pull(uniq)[inv])

    def push_fused():
        a.push_dup(ids, grads)

    def push_composed():
        u, iv = torch.unique(ids, return_inverse=True)
        buf = torch.zeros((u.numel(), P), dtype=wire, device="cuda")
        buf.index_add_(0, iv, grads.to(wire))
        torch.cuda.synchronize()  # Table.push runs on the table's own stream: buf must be complete
        b.push(u, buf)
    push_fused()
    push_composed()
    ra, rb = a.export(allk), b.export(allk)
    # index_add_ sums in no fixed order: the two tables agree to rounding, not in bits
    err = float(((ra.double() - rb.double()).abs() / (1 + rb.double().abs())).max())
    assert err < (1e-5 if w2v else 1e-3), err  # LR: the composed side sums in the fp32 wire type

    # ---- times ----
    out_u = torch.empty(n, dtype=torch.int64, device="cuda")
    out_i = torch.empty(n, dtype=torch.int32, device="cuda")
    out_c = torch.empty(n, dtype=torch.int32, device="cuda")
    nu = ctypes.c_uint64()
    lib = capi.lib()

    def coalesce():
        capi.check(lib.swps_coalesce(a.h, capi.ptr(ids), n, capi.ptr(out_u), capi.ptr(out_i), capi.ptr(out_c),
                                     ctypes.byref(nu), None))
    look_f, look_c, coal, uniq_ms = timed([lambda: a.lookup(ids),
                                           lambda: b.pull(torch.unique(ids, return_inverse=True)[0])[inv],
                                           coalesce,
                                           lambda: torch.unique(ids, return_inverse=True)], reps, warmup)
    push_f, push_c = timed([push_fused, push_composed], reps, warmup)
    assert nu.value == U
    cold = []
    for i in range(warmup + reps):
        x = table()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x.lookup(ids)
        torch.cuda.synchronize()
        if i >= warmup:
            cold.append((time.perf_counter() - t0) * 1e3)
        x.close()
    cold = float(np.median(cold))
    a.close()
    b.close()

    row_bytes = a.row_elems * 4
    sort_bytes = 8 * 2 * 12 * n
    push_bytes = n * P * 4 + 2 * U * row_bytes + sort_bytes
    look_bytes = n * a.pull_elems * 4 + U * a.pull_elems * 4 + sort_bytes

    def rate(nbytes, ms):
        return dict(bytes=nbytes, gb_per_s=round(nbytes / ms / 1e6, 1), of_hbm_peak=round(nbytes / ms / 1e3 / HBM * 1e6, 4))
    return dict(shape=name, n=n, keys=V, distinct=U, hottest=int(torch.bincount(inv).max()), row_bytes=row_bytes,
                lookup=dict(fused_ms=round(look_f, 3), composed_ms=round(look_c, 3), coalesce_ms=round(coal, 3),
                            find_gather_ms=round(look_f - coal, 3), cold_ms=round(cold, 3),
                            insert_ms=round(cold - look_f, 3), torch_unique_ms=round(uniq_ms, 3),
                            speedup=round(look_c / look_f, 2), **rate(look_bytes, look_f)),
                push=dict(fused_ms=round(push_f, 3), composed_ms=round(push_c, 3),
                          speedup=round(push_c / push_f, 2),
                          max_rel_diff_vs_composed=err, **rate(push_bytes, push_f)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="w2v-zipf,w2v-uniform,lr")
    a = ap.parse_args()
    import swiftmpi_amd as sw
    res = []
    for name in a.shapes.split(","):
        r = run_shape(sw, name, a.reps, a.warmup)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
