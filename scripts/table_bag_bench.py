"""Time the pooled calls of the HBM table (swps_lookup_bag / swps_push_bag)
beside what the repeated-key calls of section 13 let a user compose.  Not part of bench.py; no
pass/fail bar.

    python scripts/table_bag_bench.py [--out FILE] [--reps 7]

Shapes: (w2v-zipf, w2v-uniform) V = 71 290 keys at D = 300 fp32 with n = 2^20 ids, drawn Zipf(1) /
uniformly, in bags of 32 (sum); (lr) an LR table of 2^20 keys with n = 2^22 uniform ids in WEIGHTED
bags of 64.  Bag gradients are fp32.  Every key is in the table before the clock starts.
  fused     Table.lookup_bag(ids, offsets[, w]) / Table.push_bag(ids, offsets, G[, w])
  composed  Table.lookup(ids).view(B, L, P)[* w].sum(1)
            G[:, None, :].expand(B, L, P)[* w] made contiguous + Table.push_dup(ids, that)
  torch     (forward only) torch.nn.functional.embedding_bag on a dense [V, P] weight holding the
            same rows, indexed by the dense ids: an outside yardstick that does NO hashing, no
            coalesce and no fp64 accumulation
Wall time around synchronous calls, torch.cuda.synchronize() before each clock read, 2 warm-ups,
median of --reps, the sides interleaved run by run in one process.  Bytes by the model of DESIGN.md
section 14; rate = bytes / fused time, beside the 8 TB/s HBM peak."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12
SHAPES = {"w2v-zipf": dict(layout="w2v", dim=300, V=71290, n=1 << 20, L=32, zipf=True, weighted=False),
          "w2v-uniform": dict(layout="w2v", dim=300, V=71290, n=1 << 20, L=32, zipf=False, weighted=False),
          "lr": dict(layout="lr", dim=1, V=1 << 20, n=1 << 22, L=64, zipf=False, weighted=True)}


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
    import torch.nn.functional as F
    sh = SHAPES[name]
    V, n, L, w2v = sh["V"], sh["n"], sh["L"], sh["layout"] == "w2v"
    B = n // L
    pool = keys_of(V)
    dense = draw(sh, 1)
    ids = torch.as_tensor(pool[dense].view(np.int64)).to("cuda")
    idx = torch.as_tensor(dense).to("cuda")
    allk = torch.as_tensor(pool.view(np.int64)).to("cuda")
    off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * L
    w = (torch.rand(n, dtype=torch.float64, device="cuda") * 2 - 1) if sh["weighted"] else None

    def table():
        return sw.Table(sh["layout"], dim=sh["dim"], capacity=V, dtype="f32", init="hash", seed=1)
    a, b = table(), table()
    weight = a.pull(allk).clone()  # the dense twin of the rows, for torch's embedding_bag
    b.pull(allk)
    P, Q = a.pull_elems, a.push_elems
    G = torch.randn((B, Q), dtype=torch.float32, device="cuda") * 0.1

    def look_fused():
        return a.lookup_bag(ids, off, w)

    def look_composed():
        v = b.lookup(ids).view(B, L, P)
        if w is not None:
            v = v * w.view(B, L, 1)
        return v.sum(1)

    def look_torch():
        return F.embedding_bag(idx, weight, off[:-1], mode="sum",
                               per_sample_weights=None if w is None else w.float())

    def push_fused():
        a.push_bag(ids, off, G, w)

    def push_composed():
        g = G[:, None, :].expand(B, L, Q)
        g = (g * w.view(B, L, 1)) if w is not None else g
        b.push_dup(ids, g.reshape(n, Q).float().contiguous())

    # ---- the sides agree (to rounding: torch's sums have no defined order, and the composed sides
    # round the weighted term to fp32 where the fused ones keep fp64) ----
    f, c, t = look_fused().double(), look_composed().double(), look_torch().double()
    look_err = float(((f - c).abs() / (1 + c.abs())).max())
    torch_err = float(((f - t).abs() / (1 + t.abs())).max())
    assert look_err < 1e-4 and torch_err < 1e-4, (look_err, torch_err)
    push_fused()
    push_composed()
    ra, rb = a.export(allk).double(), b.export(allk).double()
    push_err = float(((ra - rb).abs() / (1 + rb.abs())).max())
    assert push_err < (1e-5 if not sh["weighted"] else 1e-3), push_err

    look_f, look_c, look_t = timed([look_fused, look_composed, look_torch], reps, warmup)
    push_f, push_c = timed([push_fused, push_composed], reps, warmup)
    U = int(torch.unique(ids).numel())
    a.close()
    b.close()

    # ---- bytes ----
    sort_bytes = 8 * 2 * 12 * n  # the coalesce: 8 onesweep passes reading and writing 12 n bytes
    wb = 8 * n if w is not None else 0
    look_bytes = sort_bytes + n * P * 4 + B * P * 4 + 8 * n + wb  # member rows read, bag rows written, rowp
    look_extra = 2 * n * P * 4  # the composed side writes and re-reads [n][P]
    push_bytes = sort_bytes + n * Q * 4 + 2 * U * a.row_elems * 4 + 8 * n + wb  # bag rows read per position (L2)
    push_extra = 2 * n * Q * 4

    def rate(nbytes, ms):
        return dict(bytes=nbytes, gb_per_s=round(nbytes / ms / 1e6, 1), of_hbm_peak=round(nbytes / ms / 1e3 / HBM * 1e6, 4))
    return dict(shape=name, n=n, bags=B, bag_len=L, keys=V, distinct=U, weighted=bool(sh["weighted"]),
                lookup=dict(fused_ms=round(look_f, 3), composed_ms=round(look_c, 3), torch_dense_ms=round(look_t, 3),
                            speedup=round(look_c / look_f, 2), composed_extra_bytes=look_extra,
                            max_rel_diff_vs_composed=look_err, max_rel_diff_vs_torch=torch_err,
                            **rate(look_bytes, look_f)),
                push=dict(fused_ms=round(push_f, 3), composed_ms=round(push_c, 3), speedup=round(push_c / push_f, 2),
                          composed_extra_bytes=push_extra, max_rel_diff_vs_composed=push_err,
                          **rate(push_bytes, push_f)))


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
