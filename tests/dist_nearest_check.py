"""Two-rank check of swps_nearest / swps_analogy on a routed table (swps_table_route) over the
host transport (gloo; both ranks share cuda:0).

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 \\
        --master-port 29543 tests/dist_nearest_check.py

Both ranks pull disjoint halves of 1031 keys into the routed table (the owners insert them), each
owner then assigns its keys' rows, and both ranks call nearest and analogy collectively with the
same arguments.  Both ranks' answers must equal each other's and the answers of ONE unrouted table
holding all rows, bit for bit, on integer-valued and on Gaussian rows; an analogy key no shard
holds fails on both ranks alike."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, NQ = 1031, 36, 70


def case(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "int":
        hv = rng.integers(-4, 5, (N, 2 * D)).astype(np.float64)
        hv[20:40] = hv[:20]  # ties across the shards: the smaller key decides
        q = rng.integers(-12, 13, (NQ, D)).astype(np.float32)
    else:
        hv = rng.normal(0, 1, (N, 2 * D)).astype(np.float32).astype(np.float64)
        q = rng.normal(0, 1, (NQ, D)).astype(np.float32)
    rows = np.concatenate([hv, np.full((N, 2 * D), 0.5)], axis=1)
    keys = rng.permutation(np.arange(1, 4 * N))[:N].astype(np.uint64) * np.uint64(7919) + np.uint64(11)
    abc = keys[np.stack([rng.choice(N, 3, replace=False) for _ in range(NQ)])]
    excl = np.stack([rng.choice(keys, 2, replace=False) for _ in range(NQ)])
    cand = rng.choice(keys, 700, replace=False)
    return keys, rows, q, abc, excl, cand


def answers(t, q, abc, excl, cand):
    out = []
    for part, metric, k in (("v", "cos", 10), ("h", "dot", 64)):
        out += list(t.nearest(q, k=k, part=part, metric=metric))
        out += list(t.nearest(q, k=k, part=part, metric=metric, exclude=excl, candidates=cand))
        out += list(t.analogy(abc, k=k, part=part, metric=metric))
    out += list(t.analogy(abc, k=1, part="v", metric="cos", candidates=cand))
    return out


def run_case(sw, comm, rank, world, dev, kind, dtype, seed):
    keys, rows, q, abc, excl, cand = case(kind, seed)
    tk = dict(dim=D, capacity=2048, dtype=dtype, init="zero", device=dev)
    t = sw.Table("w2v", **tk)
    t.route(comm, frag_num=997)
    half = np.array_split(keys, world)[rank]
    t.pull_h(half)  # collective: every key lands on its owner
    t.barrier()
    mine = t.keys()
    pos = {int(x): i for i, x in enumerate(keys)}
    own = np.array([pos[int(x)] for x in mine], dtype=np.int64)
    if len(mine):
        t.assign(torch.as_tensor(mine.view(np.int64), device="cuda:%d" % dev),
                 torch.as_tensor(rows[own], dtype=t.torch_dtype, device="cuda:%d" % dev))
    t.barrier()
    got = answers(t, q, abc, excl, cand)
    bad = abc[:3].copy()
    bad[1, 2] = np.uint64(5)  # a key no shard holds
    try:
        t.analogy(bad, k=1)
        code = 0
    except sw.SwpsError as e:
        code = e.code
    after = t.nearest(q[:2], k=3)  # the table is usable afterwards, on every rank
    t.finish()
    objs = [None] * world
    dist.all_gather_object(objs, (got, code, after, len(mine)))
    t.close()
    if rank != 0:
        return
    ref = sw.Table("w2v", **tk)
    sw.capi.check(sw.capi.lib().swps_assign_h(ref.h, sw.capi.ptr(keys), N, sw.capi.ptr(np.ascontiguousarray(rows))))
    want = answers(ref, q, abc, excl, cand)
    want_after = ref.nearest(q[:2], k=3)
    assert sum(o[3] for o in objs) == N and all(o[3] > 0 for o in objs), [o[3] for o in objs]
    for src, (g, code, after, _) in enumerate(objs):
        assert code == -2, (kind, dtype, src, code)  # SWPS_E_BADKEY
        assert len(g) == len(want)
        for i, (a, b) in enumerate(zip(g, want)):
            assert a.dtype == b.dtype and np.array_equal(a, b), (kind, dtype, "rank", src, "answer", i)
        assert np.array_equal(after[0], want_after[0]) and np.array_equal(after[1], want_after[1])
    ref.close()
    print("case ok", kind, dtype, "keys per rank", [o[3] for o in objs])


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    import swiftmpi_amd as sw
    from swiftmpi_amd.comm import Comm
    dev = 0
    torch.cuda.set_device(dev)
    comm = Comm.host(device=dev)
    for i, (kind, dtype) in enumerate([("int", "f32"), ("gauss", "f32"), ("gauss", "f64")]):
        run_case(sw, comm, rank, world, dev, kind, dtype, seed=40 + i)
    comm.close()
    dist.barrier()
    if rank == 0:
        print("NEAREST OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
