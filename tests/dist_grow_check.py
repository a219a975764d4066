"""Two ranks of a key-sharded table (swps_table_route over the host transport, gloo; the ranks
share one GPU) whose shards both start at capacity 4 under a ceiling and grow on their own as
the owner side of the routed pulls inserts keys (tests/test_table_grow_gpu.py).

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \\
        --master-port 29541 tests/dist_grow_check.py

Every rank pulls and pushes overlapping Zipf key sets over three rounds.  Rank 0 then replays
the same per-source sequence on ONE unrouted table created large (per round: every rank's pull
in rank order, then every rank's push in rank order) and compares, bit for bit, every rank's
pulled values and every shard's rows.  Each shard must have grown, independently of the other."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 3
FRAG = 997


def round_keys(rng, n, V=400):
    p = 1.0 / np.arange(1, V + 1)
    p /= p.sum()
    k = np.unique(rng.choice(V, n, p=p)).astype(np.uint64) * np.uint64(7919) + np.uint64(11)
    rng.shuffle(k)
    return k


def plan(world, seed, layout, D):
    """[round][rank] -> (keys, grads): the same on every rank."""
    out = []
    for r in range(ROUNDS):
        row = []
        for src in range(world):
            rng = np.random.default_rng(seed * 1000 + r * 31 + src)
            k = round_keys(rng, 60 + 25 * src)
            if layout == "w2v":
                g = rng.normal(0, 0.3, (len(k), 2 * D))
            else:
                g = rng.normal(0, 0.3, len(k)).astype(np.float32)
            row.append((k, g))
        out.append(row)
    return out


def run_case(sw, comm, rank, world, dev, layout, dtype, seed):
    D = 12 if layout == "w2v" else 1
    tk = dict(dim=D, dtype=dtype, learning_rate=0.7 if layout == "w2v" else 0.05, init="hash", seed=seed, device=dev)
    t = sw.Table(layout, capacity=4, max_capacity=4096, **tk)
    t.route(comm, frag_num=FRAG)
    P = plan(world, seed, layout, D)
    pulled = []
    for row in P:
        k, g = row[rank]
        pulled.append(t.pull_h(k))
        t.push_h(k, g)
    t.finish()
    keys = t.keys()
    cap = t.capacity()
    assert cap["growths"] >= 1 and cap["capacity"] >= t.size() == len(keys) > 4, (rank, cap, len(keys))
    rows = []
    if len(keys):
        kk = torch.as_tensor(keys.astype(np.int64), device="cuda:%d" % dev)
        rows = t.export(kk).double().cpu().numpy()
    objs = [None] * world
    dist.all_gather_object(objs, (keys, rows, pulled, cap))
    t.close()
    if rank != 0:
        return
    ref = sw.Table(layout, capacity=8192, **tk)
    ref_pulled = [[] for _ in range(world)]
    for row in P:
        for s in range(world):
            ref_pulled[s].append(ref.pull_h(row[s][0]))
        for s in range(world):
            ref.push_h(*row[s])
    assert ref.capacity()["growths"] == 0
    allk = []
    for src, (keys, rows, pulled, cap) in enumerate(objs):
        for a, b in zip(pulled, ref_pulled[src]):
            assert a.dtype == b.dtype and np.array_equal(a, b), (layout, dtype, "pulled values differ", src)
        kk = torch.as_tensor(keys.astype(np.int64), device="cuda:%d" % dev)
        want = ref.export(kk).double().cpu().numpy()
        assert np.array_equal(rows, want), (layout, dtype, src, float(np.abs(rows - want).max()))
        allk.extend(int(x) for x in keys)
    assert sorted(allk) == sorted(int(x) for x in ref.keys()), "union of the shards != reference key set"
    ref.close()
    print("case ok", layout, dtype, "keys", len(allk), "shards", [(o[3]["capacity"], o[3]["growths"]) for o in objs])


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    import swiftmpi_amd as sw
    from swiftmpi_amd.comm import Comm
    dev = 0
    torch.cuda.set_device(dev)
    comm = Comm.host(device=dev)
    for i, (layout, dtype) in enumerate([("w2v", "f32"), ("w2v", "f64"), ("lr", "f32")]):
        run_case(sw, comm, rank, world, dev, layout, dtype, seed=5 + i)
    comm.close()
    dist.barrier()
    if rank == 0:
        print("GROW OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
