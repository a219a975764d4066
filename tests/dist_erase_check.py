"""Two-rank check of swps_erase on a key-sharded table (a table bound with swps_table_route) over
the host transport (gloo; both ranks on one GPU).

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \\
        --master-port 29543 tests/dist_erase_check.py

Per round every rank pulls a key set, pushes gradients to it and then erases a list WITH REPEATS,
absent keys and ~0; the ranks' sets and lists overlap (the same key named by both ranks reaches
its owner twice), in one round rank 1 passes n = 0 to the erase (it still joins the round), and
rank 1 finishes one round early: its swps_finish serves rank 0's last pull, push and erase.  Rank
0 gathers every shard and compares it, bit for bit and per key, with ONE unrouted table that per
round pulled every rank's keys, applied rank 0's push and then rank 1's, and erased the two lists
at once.  Per round the ranks' erased counts (each the count of its own shard) sum to the
unrouted table's."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 4
EMPTY_ROUND, EMPTY_RANK = 1, 1
EARLY_RANK = 1  # runs ROUNDS - 1 rounds, then finishes


def plan(world, seed, layout, D):
    """[round][rank] -> (distinct keys to pull and push, their gradients, the erase list)."""
    pool = np.arange(1, 301, dtype=np.uint64) * np.uint64(7919) + np.uint64(11)
    out = []
    for r in range(ROUNDS):
        row = []
        for src in range(world):
            rng = np.random.default_rng(seed * 1000 + r * 31 + src)
            k = pool[rng.choice(300, 120 + 20 * src, replace=False)]
            g = rng.normal(0, 0.3, (len(k), 2 * D if layout == "w2v" else 1)).astype(
                np.float64 if layout == "w2v" else np.float32)
            if r == EMPTY_ROUND and src == EMPTY_RANK:
                e = np.zeros(0, dtype=np.uint64)
            else:
                held = pool[rng.choice(300, 70, replace=False)]  # most are held by now, on either shard
                e = np.concatenate([held, held[:9], np.array([5, 2 ** 64 - 1, 2 ** 63 + 1], dtype=np.uint64)])
                e = rng.permutation(e)
            row.append((k, g, e))
        out.append(row)
    return out


def run_case(sw, comm, rank, world, dev, layout, dtype, seed):
    D = 6 if layout == "w2v" else 1
    tk = dict(dim=D, capacity=512, dtype=dtype, learning_rate=0.7 if layout == "w2v" else 0.05, init="hash",
              seed=seed, device=dev)
    cuda = "cuda:%d" % dev

    def d(a):
        a = np.ascontiguousarray(a)
        return torch.as_tensor(a.view(np.int64) if a.dtype == np.uint64 else a).to(cuda)

    t = sw.Table(layout, **tk)
    t.route(comm, frag_num=997)
    P = plan(world, seed, layout, D)
    mine = ROUNDS - 1 if rank == EARLY_RANK else ROUNDS
    counts = []
    for row in P[:mine]:
        k, g, e = row[rank]
        t.pull(d(k))
        t.push(d(k), d(g))
        counts.append(t.erase(d(e)))
    t.finish()
    keys = t.keys()
    rows = t.export(d(keys)).cpu().numpy() if len(keys) else []
    objs = [None] * world
    dist.all_gather_object(objs, (keys, rows, counts, t.size()))
    t.close()
    if rank != 0:
        return
    ref = sw.Table(layout, **tk)
    ref_counts = []
    for r, row in enumerate(P):
        live = [s for s in range(world) if not (s == EARLY_RANK and r >= ROUNDS - 1)]
        for s in live:
            ref.pull(d(row[s][0]))
        for s in live:  # rank 0's step, then rank 1's
            ref.push(d(row[s][0]), d(row[s][1]))
        ref_counts.append(ref.erase(d(np.concatenate([row[s][2] for s in live]))))
    allk = []
    for src, (keys, rows, counts, size) in enumerate(objs):
        assert size == len(keys)
        if len(keys):
            want = ref.export(d(keys)).cpu().numpy()
            assert rows.tobytes() == want.tobytes(), (layout, dtype, "shard rows differ", src)
        allk.extend(int(x) for x in keys)
    assert sorted(allk) == sorted(int(x) for x in ref.keys()), "union of the shards != reference key set"
    assert len(allk) == ref.size()
    for r in range(ROUNDS - 1):  # the rounds both ranks ran: each rank reports its own shard's count
        got = sum(o[2][r] for o in objs)
        assert got == ref_counts[r], (layout, dtype, "erased counts", r, got, ref_counts[r])
    assert min(ref_counts) > 0
    print("case ok", layout, dtype, "keys", len(allk), "erased per round", ref_counts)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    import swiftmpi_amd as sw
    from swiftmpi_amd.comm import Comm
    dev = 0
    torch.cuda.set_device(dev)
    comm = Comm.host(device=dev)
    for i, (layout, dtype) in enumerate([("w2v", "f32"), ("w2v", "f64"), ("lr", "f32")]):
        run_case(sw, comm, rank, world, dev, layout, dtype, seed=15 + i)
    comm.close()
    dist.barrier()
    if rank == 0:
        print("ERASE ROUTE OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
