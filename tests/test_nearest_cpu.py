"""The query path's host side (no GPU): the C ABI declares and exports swps_nearest /
swps_analogy and their host forms with the prototypes capi binds, and the numpy fp64 reference
(evaluate.nearest_reference) implements the library's total order."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

ENTRY = {
    "swps_nearest": 12,
    "swps_nearest_h": 12,
    "swps_analogy": 10,
    "swps_analogy_h": 10,
}


def _header():
    src = open(os.path.join(ROOT, "include", "swps.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    for name, nargs in ENTRY.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        assert args[0].startswith("swps_table *"), (name, args[0])
    for c in ("SWPS_METRIC_DOT", "SWPS_METRIC_COS", "SWPS_NEAREST_MAX_K", "SWPS_NEAREST_MAX_EXCL"):
        assert re.search(r"#define\s+%s\b" % c, src), c


def test_library_exports_them_with_capi_prototypes(lib):
    from swiftmpi_amd import capi
    L = ctypes.CDLL(capi.LIB_PATH)
    src = _header()
    ctype_of = {"swps_table *": ctypes.c_void_p, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    for name, nargs in ENTRY.items():
        assert hasattr(L, name), name
        res, args = capi.PROTOS[name]
        assert res is ctypes.c_int and len(args) == nargs, (name, args)
        decl = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S).group(1)
        for a, got in zip(decl.split(","), args):
            a = " ".join(a.split())
            want = ctypes.c_void_p if "*" in a else ctype_of[a.rsplit(" ", 1)[0]]
            assert got is want, (name, a, got)
    assert capi.METRIC_DOT == 0 and capi.METRIC_COS == 1 and capi.NEAREST_MAX_K == 64 and capi.NEAREST_MAX_EXCL == 8


def _brute(rows, keys, queries, k, metric, exclude, candidates):
    """Per query: score every allowed row in fp64, then pick the best k one at a time."""
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    out_k = np.full((len(queries), k), empty, dtype=np.uint64)
    out_s = np.full((len(queries), k), -np.inf)
    for i, q in enumerate(queries):
        pool = []
        for r, key in zip(rows, keys):
            if candidates is not None and key not in candidates:
                continue
            if exclude is not None and key in exclude[i]:
                continue
            s = float(np.dot(q.astype(np.float64), r.astype(np.float64)))
            if metric == "cos":
                n2 = float(np.dot(r.astype(np.float64), r.astype(np.float64)))
                s = 0.0 if n2 == 0 else s / np.sqrt(n2)
            pool.append((s, int(key)))
        for j in range(k):
            if not pool:
                break
            best = pool[0]
            for c in pool[1:]:
                if c[0] > best[0] or (c[0] == best[0] and c[1] < best[1]):
                    best = c
            pool.remove(best)
            out_k[i, j], out_s[i, j] = best[1], best[0]
    return out_k, out_s


def test_reference_agrees_with_brute_force():
    from swiftmpi_amd.evaluate import nearest_reference
    rng = np.random.default_rng(5)
    rows = rng.integers(-3, 4, (50, 7)).astype(np.float64)
    rows[10:25] = rows[30:45]  # duplicate rows: equal scores, the smaller key wins
    rows[7] = 0  # a zero row scores 0 under cos
    keys = rng.permutation(np.arange(1000, 1050)).astype(np.uint64) * np.uint64(2654435761)
    queries = rng.integers(-3, 4, (9, 7)).astype(np.float64)
    excl = np.stack([rng.choice(keys, 3, replace=False) for _ in queries])
    excl[0, 1] = np.uint64(0xFFFFFFFFFFFFFFFF)  # an unused slot
    cand = set(int(x) for x in rng.choice(keys, 30, replace=False))
    for metric in ("dot", "cos"):
        for k in (1, 10, 64):  # 64 > rows: padded
            for e, c in ((None, None), (excl, None), (None, cand), (excl, cand)):
                gk, gs = nearest_reference(rows, keys, queries, k, metric, e,
                                           None if c is None else np.array(sorted(c), dtype=np.uint64))
                wk, ws = _brute(rows, keys, queries, k, metric, e, c)
                assert np.array_equal(gk, wk), (metric, k)
                assert np.array_equal(gs, ws), (metric, k)
    # ties: among the duplicated rows the smaller key comes first
    gk, gs = nearest_reference(rows, keys, queries, 50, "cos")
    for i in range(len(queries)):
        same = gs[i, 1:] == gs[i, :-1]
        assert same.sum() >= 10
        assert np.all(gk[i, 1:][same] > gk[i, :-1][same])
    # exclusions hold, k > rows pads with key ~0 / -inf
    gk, gs = nearest_reference(rows, keys, queries, 64, "dot", excl)
    assert np.all(gk[1:, 47:] == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isneginf(gs[1:, 47:]))
    assert np.all(gk[1:, :47] != np.uint64(0xFFFFFFFFFFFFFFFF))
    assert np.all(gk[0, :48] != np.uint64(0xFFFFFFFFFFFFFFFF))  # query 0 excludes two keys only
    assert np.all(gk[0, 48:] == np.uint64(0xFFFFFFFFFFFFFFFF))
    for i in range(len(queries)):
        assert not set(gk[i].tolist()) & (set(excl[i].tolist()) - {0xFFFFFFFFFFFFFFFF})


def test_reference_orders_nan_last():
    from swiftmpi_amd.evaluate import topk_order
    s = np.array([[1.0, np.nan, -np.inf, 1.0, np.nan]])
    keys = np.array([9, 4, 7, 3, 2], dtype=np.uint64)
    gk, gs = topk_order(s, keys, 6)
    assert gk[0].tolist() == [3, 9, 7, 2, 4, 0xFFFFFFFFFFFFFFFF]
    assert np.isnan(gs[0, 3]) and np.isnan(gs[0, 4]) and np.isneginf(gs[0, 5])
