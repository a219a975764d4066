"""Two-rank check of the pooled calls on a key-sharded table (swps_lookup_bag / swps_push_bag on a
table bound with swps_table_route) over the host transport (gloo; both ranks on one GPU).

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \\
        --master-port 29542 tests/dist_bag_check.py

Every rank pools and pushes bags WITH REPEATS drawn from one key pool (so keys overlap between the
ranks), and in one round rank 1 passes n = 0, nbags = 0 (it still joins the exchanges).  Each rank
coalesces its own ids; only distinct keys cross the wire, and an owner applies the ranks' reduced
pushes of a shared key as separate steps in rank order.  Rank 0 gathers every shard and compares
it, bit for bit, with ONE unrouted table that per round pooled every rank's bags and then applied
rank 0's push_bag and then rank 1's."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 4
EMPTY_ROUND, EMPTY_RANK = 2, 1
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def plan(world, seed, layout, D, gtype):
    """[round][rank] -> (ids with repeats and padding, offsets, weights, bag grads): the same on every rank."""
    pool = np.arange(1, 401, dtype=np.uint64) * np.uint64(7919) + np.uint64(11)
    p = 1.0 / np.arange(1, 401)
    p /= p.sum()
    out = []
    for r in range(ROUNDS):
        row = []
        for src in range(world):
            rng = np.random.default_rng(seed * 1000 + r * 31 + src)
            if r == EMPTY_ROUND and src == EMPTY_RANK:
                lens = np.zeros(0, dtype=np.int64)
            else:  # short bags, empty ones, and two past one chunk; Zipf: the hottest key runs past one chunk
                lens = rng.permutation(np.concatenate([rng.integers(0, 9, 150), [0, 0, 130, 400 + 50 * src]]))
            n = int(lens.sum())
            k = pool[rng.choice(400, n, p=p)]
            k[rng.random(n) < 0.03] = PAD
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            w = rng.uniform(-2, 2, n)
            g = rng.normal(0, 0.3, (len(lens), 2 * D if layout == "w2v" else 1)).astype(gtype)
            row.append((k, off, w, g))
        out.append(row)
    return out


def run_case(sw, comm, rank, world, dev, layout, dtype, rule, gtype, mode, weighted, seed):
    D = 6 if layout == "w2v" else 1
    tk = dict(dim=D, capacity=2048, dtype=dtype, learning_rate=0.7 if layout == "w2v" else 0.05, init="hash",
              seed=seed, device=dev, push_rule=rule)
    cuda = "cuda:%d" % dev

    def d(a):
        a = np.ascontiguousarray(a)
        return torch.as_tensor(a.view(np.int64) if a.dtype == np.uint64 else a).to(cuda)

    def both(t, k, off, w, g):
        w = d(w) if weighted else None
        pooled = t.lookup_bag(d(k), d(off), w, mode).cpu().numpy()
        return pooled, lambda: t.push_bag(d(k), d(off), d(g), w, mode, -1.0)

    t = sw.Table(layout, **tk)
    t.route(comm, frag_num=997)
    P = plan(world, seed, layout, D, gtype)
    pulled = []
    for row in P:
        pooled, push = both(t, *row[rank])
        pulled.append(pooled)
        push()
    t.finish()
    stats = t.route_stats()
    keys = t.keys()
    rows = t.export(d(keys)).cpu().numpy() if len(keys) else []
    objs = [None] * world
    dist.all_gather_object(objs, (keys, rows, pulled, stats))
    t.close()
    if rank != 0:
        return
    ref = sw.Table(layout, **tk)
    ref_pulled = [[] for _ in range(world)]
    for row in P:
        pushes = []
        for s in range(world):
            pooled, push = both(ref, *row[s])
            ref_pulled[s].append(pooled)
            pushes.append(push)
        for push in pushes:  # rank 0's reduced push, then rank 1's
            push()
    allk = []
    sent = 0
    for src, (keys, rows, pulled, stats) in enumerate(objs):
        for a, b in zip(pulled, ref_pulled[src]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (layout, dtype, "pooled values differ", src)
        if len(keys):
            want = ref.export(d(keys)).cpu().numpy()
            assert rows.tobytes() == want.tobytes(), (layout, dtype, rule, src)
        allk.extend(int(x) for x in keys)
        assert stats["rounds"] == 2 * ROUNDS, stats
        sent += stats["keys_sent"]
    assert sorted(allk) == sorted(int(x) for x in ref.keys()), "union of the shards != reference key set"
    # only distinct keys crossed the wire: a lookup and a push of each call's distinct keys
    distinct = sum(2 * len(np.unique(k[k != PAD])) for row in P for k, _, _, _ in row)
    assert sent == distinct, (sent, distinct)
    print("case ok", layout, dtype, rule, mode, "weighted" if weighted else "plain", "keys", len(allk),
          "distinct keys sent", sent)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    import swiftmpi_amd as sw
    from swiftmpi_amd.comm import Comm
    dev = 0
    torch.cuda.set_device(dev)
    comm = Comm.host(device=dev)
    cases = [("w2v", "f32", "adagrad", np.float32, "sum", False), ("w2v", "f64", "adagrad", np.float64, "mean", False),
             ("lr", "f32", "adagrad", np.float32, "sum", True), ("w2v", "f32", "sgd", np.float64, "sum", True)]
    for i, (layout, dtype, rule, gtype, mode, weighted) in enumerate(cases):
        run_case(sw, comm, rank, world, dev, layout, dtype, rule, gtype, mode, weighted, seed=5 + i)
    comm.close()
    dist.barrier()
    if rank == 0:
        print("BAG ROUTE OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
