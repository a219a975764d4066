"""Time the query path (swps_analogy / swps_nearest) at a text8-like shape and put it beside two
yardsticks.  Not part of bench.py; no pass/fail bar.

    python scripts/nearest_bench.py [--out FILE]

Shapes: an fp32 W2V table of V = 71 290 Gaussian rows, D = 300 (text8's vocabulary at min_count
5 and the usual vector length); (1) 19 544 analogy questions (questions-words.txt's count), k = 1,
cosine; (2) 1000 nearest-neighbour queries, k = 40 (the `distance` tool's default).

Steps, each a child process under its own `timeout -k 10`; the first that fails ends the run:
  lib    the library calls: ms per call from HIP events on the table's stream around the call
         (which synchronises before it returns), median of --reps after a warm-up
  torch  yardstick 1: (Q @ R.T).topk(k) in torch on the exported rows, same GPU, same events
  host   yardstick 2, the capability before the query path existed: synth.analogy_accuracy (numpy
         fp64, one question at a time) on a 500-question sample, scaled to 19 544
The model kept with the numbers: FLOP = 2 nq V D against the 157 TF f32-MFMA peak; bytes = the
row blocks the scoring kernel stages, ceil(nq / 32) query tiles x V x D x 4 B (mostly served by
L2 / Infinity Cache: the table's v blocks are 86 MB), and the compulsory HBM read, V x D x 4 B
once, against the 8 TB/s HBM peak."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, D, NQ1, NQ2, K2 = 71290, 300, 19544, 1000, 40
PEAK_F32_MFMA = 157e12
PEAK_HBM = 8.0e12
QT = 32  # queries per scoring block (swps_nearest.hip kQT)


def data(v=V):
    rng = np.random.default_rng(7)
    keys = np.arange(1, v + 1, dtype=np.uint64) * np.uint64(2654435761)
    vecs = rng.normal(0, 1, (v, D)).astype(np.float32)
    abc = keys[rng.integers(0, v, (NQ1, 3))]
    q2 = rng.normal(0, 1, (NQ2, D)).astype(np.float32)
    return keys, vecs, abc, q2


def make_table(sw, keys, vecs):
    t = sw.Table("w2v", dim=D, capacity=len(keys) + 8, dtype="f32", init="zero")
    for a in range(0, len(keys), 8192):
        rows = np.zeros((min(8192, len(keys) - a), 4 * D))
        rows[:, D:2 * D] = vecs[a:a + len(rows)]
        k = np.ascontiguousarray(keys[a:a + len(rows)])
        sw.capi.check(sw.capi.lib().swps_assign_h(t.h, sw.capi.ptr(k), len(k), sw.capi.ptr(rows)))
    return t


def timed(fn, ev_stream, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ev_stream)
        fn()
        e1.record(ev_stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def model(nq):
    flop = 2.0 * nq * V * D
    staged = -(-nq // QT) * V * D * 4.0
    return flop, staged, V * D * 4.0


def step_lib(a):
    import torch
    import swiftmpi_amd as sw
    assert torch.cuda.is_available(), "needs the GPU"
    keys, vecs, abc, q2 = data()
    t = make_table(sw, keys, vecs)
    w = sw.Word2Vec(t, init="table")  # its compute stream is the table's stream
    s = torch.cuda.ExternalStream(w.stream())
    dabc = torch.as_tensor(abc.view(np.int64), device="cuda")
    dq2 = torch.as_tensor(q2, device="cuda")
    out = {}
    for name, nq, fn in (("analogy_k1", NQ1, lambda: t.analogy(dabc, k=1)),
                         ("nearest_k40", NQ2, lambda: t.nearest(dq2, k=K2))):
        med, mn = timed(fn, s, a.reps, a.warmup)
        flop, staged, hbm = model(nq)
        out[name] = dict(nq=nq, ms=med, ms_min=mn, tflops=flop / med / 1e9, mfma_peak_share=flop / (med * 1e-3) / PEAK_F32_MFMA,
                         staged_gb=staged / 1e9, staged_tbs=staged / med / 1e9, hbm_mb=hbm / 1e6,
                         hbm_floor_ms=hbm / PEAK_HBM * 1e3, mfma_floor_ms=flop / PEAK_F32_MFMA * 1e3)
    print("STEP " + json.dumps(out), flush=True)


def step_torch(a):
    import torch
    import swiftmpi_amd as sw
    keys, vecs, abc, q2 = data()
    t = make_table(sw, keys, vecs)
    dk = torch.as_tensor(keys.view(np.int64), device="cuda")
    R = t.export(dk)[:, D:2 * D].contiguous()  # exported rows, the same GPU
    t.close()
    Rn = R / R.norm(dim=1, keepdim=True)
    idx = torch.as_tensor((abc // np.uint64(2654435761)).astype(np.int64) - 1, device="cuda")
    Q1 = (R[idx[:, 1]] - R[idx[:, 0]]) + R[idx[:, 2]]
    Q2 = torch.as_tensor(q2, device="cuda")
    s = torch.cuda.current_stream()
    out = {}
    for name, Q, k in (("analogy_k1", Q1, 1), ("nearest_k40", Q2, K2)):
        med, mn = timed(lambda: (Q @ Rn.T).topk(k), s, a.reps, a.warmup)
        out[name] = dict(ms=med, ms_min=mn)
    print("STEP " + json.dumps(out), flush=True)


def step_host(a):
    from swiftmpi_amd.synth import analogy_accuracy
    keys, vecs, abc, _ = data()
    index = {int(k): i for i, k in enumerate(keys)}
    # a fourth word that differs from a, b, c: the accuracy is not the point, the time is
    quest = [(int(x[0]), int(x[1]), int(x[2]), int(x[0])) for x in abc[:500] if len(set(x.tolist())) == 3]
    t0 = time.perf_counter()
    analogy_accuracy(vecs, index, quest, [int(k) for k in keys])
    dt = time.perf_counter() - t0
    print("STEP " + json.dumps(dict(questions=len(quest), seconds=dt, scaled_ms=dt / len(quest) * NQ1 * 1e3)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["lib", "torch", "host"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        return {"lib": step_lib, "torch": step_torch, "host": step_host}[a.step](a)
    res = {"shape": dict(V=V, D=D, dtype="f32")}
    for step, limit in (("lib", 240), ("torch", 240), ("host", 300)):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-3000:], r.stderr[-3000:], file=sys.stderr)
            print(json.dumps(dict(res, failed=step, returncode=r.returncode)))
            return 1
        res[step] = json.loads(line[-1][5:])
    res["ratios"] = {
        "torch_over_lib_analogy_k1": res["torch"]["analogy_k1"]["ms"] / res["lib"]["analogy_k1"]["ms"],
        "torch_over_lib_nearest_k40": res["torch"]["nearest_k40"]["ms"] / res["lib"]["nearest_k40"]["ms"],
        "host_over_lib_analogy_k1": res["host"]["scaled_ms"] / res["lib"]["analogy_k1"]["ms"],
    }
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
